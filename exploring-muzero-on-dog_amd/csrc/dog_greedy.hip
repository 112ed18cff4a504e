// The one-ply greedy agent for DOG (include/muz.h: muz_dog_greedy_action): every legal action is tried once on the
// real environment and the board it leads to is scored by six integer features (progress gained, progress taken from
// the other side, pins in the goal, pins out of home, pins sent home, the win).  The reference has no DOG agent that
// runs, so parity with it is UNPINNED; the definition is tests/_dog_greedy.py, which this kernel equals bit for bit
// in every integer it writes (the sampled action also goes through the device's logf).
//
// One launch, one workgroup per game:
//   all waves   the root into LDS (dog_load), the base checks (dog_checks_block)
//   wave 0      the 13 mask words (dog_mask_words) expanded to the ascending candidate list in LDS
//   every wave  strides over the candidates: the root read from LDS into the registers of its 64 lanes (DogWave: a
//               cell, a pin, per lane), the candidate's transition on those registers (the wv_step_* functions of
//               dog_env.hpp) with no write-back, the features from the root's and the afterstate's pin lanes; lane 0
//               writes the score to LDS, lanes 0-5 the features to memory where asked
//   wave 0      the argmax of v(a) over the candidates (temperature 0: of the scores), ties to the smaller action
//   all waves   the row of scores to memory where asked, zero features for the actions that are not candidates
// The register step (dog_greedy_afterstate, with dog_player_stats in dog_score.hpp, which dog_guided.hip shares) is
// its own dispatch over the shared wv_step_* functions rather than a split of dog_env_step_play_wave into "compute"
// and "write back": that function is inlined into k_dog_play and k_dog_rollout,
// whose register allocation the DOG benchmark measures.  The afterstate needs neither the hands nor the
// next player (only its board and pins are scored), and a candidate's card is in the hand (it is a bit of the legal
// mask), so the hand lanes are not loaded at all.
// Loops: at most 806 candidates per game, 4 matching rounds per player.  Barriers: every wave takes the same four.
#undef MUZ_DOG_STAMPS   // the stamps build instruments k_dog_play only (its counters live in env_dog.hip)
#include <climits>
#include <cmath>

#include "dog_score.hpp"

namespace muz {

struct DogGreedyW {
  int w[6];
};

__global__ __launch_bounds__(kDogBlockThreads) void k_dog_greedy(DetConsts c, DogGreedyW wt, float temperature,
                                                                 unsigned long long seed, int turn, muz_dog_soa st,
                                                                 const int32_t* game_id, int32_t* action,
                                                                 int32_t* scores, int32_t* features, int n) {
  __shared__ DogG s;
  __shared__ int s_score[kDogActions];          // by action; INT32_MIN: not a candidate
  __shared__ unsigned short s_cand[kDogActions];
  __shared__ int s_ncand;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x;
  if (g >= n) return;   // (block-uniform; the grid is n)
  for (int a = tid; a < kDogActions; a += kDogBlockThreads) s_score[a] = INT_MIN;
  dog_load<BlockSync>(c, st, g, s, tid);
  dog_checks_block(c, s, tid);
  if (wave == 0) {
    unsigned long long m[13];
    dog_mask_words(c, s, lane, m);
    const bool over = s.done != 0;
    int base = 0;
#pragma unroll
    for (int r = 0; r < 13; ++r) {
      const unsigned long long w = over ? 0ull : m[r];
      // (bit a of the mask is set for a < 806 only, so base + rank < 806)
      if ((w >> lane) & 1ull) s_cand[base + __popcll(w & ((1ull << lane) - 1ull))] = (unsigned short)(r * 64 + lane);
      base += __popcll(w);
    }
    if (lane == 0) s_ncand = base;
  }
  __syncthreads();
  const int ncand = s_ncand;
  // a swap-phase candidate (792..805: the card to hand over) leaves the board alone: features 0, nothing stepped.
  // ncand and s.phase are block-uniform, so a swap-phase, finished or stuck root skips the loop in every wave.
  const bool stepped = s.phase == 0 && ncand > 0;
  if (stepped) {
    const int scp = s.cp;
    const int dist = kTrack / c.P;
    const bool teams = has(c.flags, R_TEAMS);
    const unsigned all = (1u << c.P) - 1u;
    const unsigned me = (teams ? ((scp & 1) ? 0xAu : 0x5u) : (1u << scp)) & all;
    DogWave R;
    R.lane = lane;
    R.cell = lane < kCells ? s.board[lane] : -1;
    R.pin = lane < 16 ? s.pins[lane] : -1;
    R.hand = 0;
    int prog0, goal0, home0;
    dog_player_stats(c, R.pin, lane, dist, prog0, goal0, home0);
    for (int i = wave; i < ncand; i += kDogBlockThreads / 64) {
      const int a = __builtin_amdgcn_readfirstlane((int)s_cand[i]);
      DogWave W = R;
      dog_greedy_afterstate(c, W, scp, a);
      int prog1, goal1, home1;
      dog_player_stats(c, W.pin, lane, dist, prog1, goal1, home1);
      const int dprog = prog1 - prog0, dgl = goal1 - goal0, dhome = home1 - home0;
      int f[6] = {0, 0, 0, 0, 0, 0};
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
      int sc = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) sc += wt.w[k] * f[k];
      if (lane == 0) s_score[a] = sc;
      if (features && lane < 6) {
        int v = f[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) v = lane == k ? f[k] : v;
        features[((size_t)g * kDogActions + a) * 6 + lane] = v;
      }
    }
  } else if (wave == 0) {
    for (int i = lane; i < ncand; i += 64) s_score[s_cand[i]] = 0;
  }
  __syncthreads();
  if (wave == 0) {
    // lane l takes candidates l, l + 64, ..: ascending actions, so "strictly greater" keeps the lane's first maximum;
    // across lanes the greater value wins and the smaller action breaks ties
    const int gid = game_id ? game_id[g] : g;
    const unsigned long long key = game_key(seed ^ kPolicyStream, gid, turn);
    const bool sample = temperature > 0.f;
    float bv = 0.f;
    int bs = 0, ba = -1;
    for (int i = lane; i < ncand; i += 64) {
      const int a = s_cand[i], sc = s_score[a];
      const float v = sample ? __fadd_rn(__fdiv_rn((float)sc, temperature), policy_gumbel(key, a)) : 0.f;
      const bool better = ba < 0 || (sample ? v > bv : sc > bs);
      if (better) {
        bv = v;
        bs = sc;
        ba = a;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int os = __shfl_xor(bs, o), oa = __shfl_xor(ba, o);
      const bool gt = sample ? ov > bv : os > bs, eq = sample ? ov == bv : os == bs;
      const bool take = oa >= 0 && (ba < 0 || gt || (eq && oa < ba));
      if (take) {
        bv = ov;
        bs = os;
        ba = oa;
      }
    }
    if (lane == 0) action[g] = ba;
  }
  if (scores || features)
    for (int a = tid; a < kDogActions; a += kDogBlockThreads) {
      const int sc = s_score[a];
      if (scores) scores[(size_t)g * kDogActions + a] = sc;
      if (features && (!stepped || sc == INT_MIN))   // (a stepped candidate's features are written above)
#pragma unroll
        for (int k = 0; k < 6; ++k) features[((size_t)g * kDogActions + a) * 6 + k] = 0;
    }
}

}  // namespace muz

using namespace muz;

extern "C" {

int muz_dog_greedy_action(const muz_rules* rules, const muz_dog_greedy_cfg* cfg, muz_dog_soa st,
                          const int32_t* game_id, int32_t* action, int32_t* scores, int32_t* features, int32_t n,
                          void* stream) {
  MUZ_HOST_CHECK(rules && cfg && n >= 0 && st.stride >= n);
  DogGreedyW wt;
  for (int k = 0; k < 6; ++k) {
    MUZ_HOST_CHECK(cfg->w[k] >= -32768 && cfg->w[k] <= 32767);
    wt.w[k] = cfg->w[k];
  }
  MUZ_HOST_CHECK(std::isfinite(cfg->temperature) && cfg->temperature >= 0.f);
  DetConsts c;
  int rc = dog_consts(rules, &c);
  if (rc) return rc;
  if (n == 0) return MUZ_OK;
  MUZ_HOST_CHECK(action != nullptr);
  MUZ_HOST_CHECK(st.board && st.pins && st.deck && st.hands && st.swap_choices && st.current_player &&
                 st.round_starter && st.phase && st.hand_size && st.reward && st.done && st.deal);
  if ((rc = dog_tables_ready())) return rc;
  k_dog_greedy<<<n, kDogBlockThreads, 0, (hipStream_t)stream>>>(c, wt, cfg->temperature, cfg->seed, cfg->turn, st,
                                                                game_id, action, scores, features, n);
  return muz_last_launch_error();
}

}  // extern "C"
