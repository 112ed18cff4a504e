// The afterstate scoring of the DOG greedy agent (include/muz.h, DOG greedy agent) on one wave's registers, shared by
// dog_greedy.hip (k_dog_greedy: the one-ply agent) and dog_guided.hip (k_dog_rollout_guided: the playout turns of the
// guided rollout agent).  A wave holds the game as DogWave (dog_env.hpp: a cell, a pin, per lane); nothing here reads
// or writes LDS or memory.
#pragma once
#include <climits>

#include "dog_env.hpp"

namespace muz {

// What the features need of one player's pins, on the lanes l with (l & 3) == p: progress (calculate_progress of
// MuZero_DOG/evaluate_agent.py, an exact integer), pins in the goal, pins at home.  `pin` is DogWave's pin lane
// (lane j < 16: pins[j]); `dist` = 40 / num_players as the reference has it.  Fully unrolled: no array is indexed
// by a runtime value.
__device__ __forceinline__ void dog_player_stats(const DetConsts& c, int pin, int lane, int dist, int& prog, int& ngoal,
                                                 int& nhome) {
  const int p = lane & 3;
  const int mt = has(c.flags, R_MUST_TRAVERSE) ? 1 : 0;
  const int g0 = dgoal0(c, p);
  int r[4];
  ngoal = 0;
  nhome = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = __shfl(pin, 4 * p + k);
    r[k] = x < 0 ? x - 5 : (x < kTrack ? fmodp(x - dist * p, kTrack) - mt : kTrack + (x - g0));
    ngoal += x >= kTrack ? 1 : 0;
    nhome += x < 0 ? 1 : 0;
  }
  auto cswap = [](int& a, int& b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
  };
  cswap(r[0], r[1]);
  cswap(r[2], r[3]);
  cswap(r[0], r[2]);
  cswap(r[1], r[3]);
  cswap(r[1], r[2]);
  // greedy matching of the sorted pins (rows) to the cells 40..43 (columns): four times the smallest distance of the
  // rows and columns left, the first (row, column) in row-major order on ties
  unsigned rows = 0u, cols = 0u;
  prog = 0;
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    int best = INT_MAX, bi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = abs(r[i] - (kTrack + j));
        const bool open = !((rows >> i) & 1u) && !((cols >> j) & 1u);
        if (open && d < best) {
          best = d;
          bi = i * 4 + j;
        }
      }
    prog += best;
    rows |= 1u << (bi >> 2);
    cols |= 1u << (bi & 3);
  }
}

// the transition of a legal play-phase action on the wave's registers (dog_env_step_play_wave without the hand, the
// next player and the write-back); the root is not finished
__device__ __forceinline__ void dog_greedy_afterstate(const DetConsts& c, DogWave& W, int scp, int action) {
  const int cp = (has(c.flags, R_TEAMS) && DogWave::player_done(c, W.occupied(), scp)) ? (scp + 2) % 4 : scp;
  const int act = action % kDogBase;
  int reward = 0, done = 0;
  if (act < kDogSwaps) {
    wv_step_swap(c, W, 0, cp, act / kCells, act % kCells, reward, done);
  } else if (act < kDogNormalBase) {
    int d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = c_dists7[act - kDogSwaps][k];
    wv_step_hot7(c, W, 0, cp, d, reward, done);
  } else if (act < kDogNegBase) {
    const int na = act - kDogNormalBase;
    int mv = na % 12 + 1;
    mv += mv >= 7 ? 1 : 0;
    wv_step_normal(c, W, 0, cp, na / 12, mv, reward, done);
  } else {
    wv_capture_move(c, W, 0, cp, act - kDogNegBase, fmodp(W.pins(cp * 4 + act - kDogNegBase) - 4, kTrack), reward,
                    done);
  }
}

// The six features of the legal play-phase action `a` of the root held in R (wave-uniform, the same on every lane):
// the action's transition on a copy of R, the players' stats after it against the root's (prog0, goal0, home0: the
// root's dog_player_stats), summed over the seats of `me` (the mover's side) and the other seats of `all`.
// (k_dog_greedy keeps this sum written out in its candidate loop: built through this function it allocates 61 VGPRs
// instead of 62, and its build is kept as it was measured -- DESIGN.md.)
__device__ __forceinline__ void dog_afterstate_features(const DetConsts& c, const DogWave& R, int prog0, int goal0,
                                                        int home0, int lane, int scp, int dist, unsigned me,
                                                        unsigned all, int a, int (&f)[6]) {
  DogWave W = R;
  dog_greedy_afterstate(c, W, scp, a);
  int prog1, goal1, home1;
  dog_player_stats(c, W.pin, lane, dist, prog1, goal1, home1);
  const int dprog = prog1 - prog0, dgl = goal1 - goal0, dhome = home1 - home0;
#pragma unroll
  for (int k = 0; k < 6; ++k) f[k] = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {   // lane p holds player p's numbers
    const int dp = __builtin_amdgcn_readlane(dprog, p), dg = __builtin_amdgcn_readlane(dgl, p),
              dh = __builtin_amdgcn_readlane(dhome, p);
    if ((me >> p) & 1u) {
      f[0] -= dp;
      f[2] += dg;
      f[3] -= dh;
    } else if ((all >> p) & 1u) {
      f[1] += dp;
      f[4] += dh;
    }
  }
  const uint32_t win = W.winners(c);
  f[5] = win == 0u ? 0 : ((win & me) ? 1 : -1);
}

}  // namespace muz
