// Batched DOG environment kernels + C ABI (include/muz.h).  One wavefront per game, 4 games per
// 256-thread workgroup; the game's state is staged in LDS (dog.hpp: DogG).
#include "dog_env.hpp"

namespace muz {

__global__ __launch_bounds__(256) void k_dog_reset(DetConsts c, muz_dog_soa st, unsigned long long seed, int n) {
  __shared__ DogG sg[kDogGamesPerBlock];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.x * kDogGamesPerBlock + w;
  if (g >= n) return;
  DogG& s = sg[w];
  dog_reset_lds<WaveSync>(c, s, seed, g, 0u, lane);
  dog_store<WaveSync>(c, st, g, s, lane);
}

__global__ __launch_bounds__(kDogBlockThreads) void k_dog_legal(DetConsts c, muz_dog_soa st, uint32_t* mask, int n) {
  __shared__ DogG s;
  const int tid = threadIdx.x, g = blockIdx.x;
  dog_load<BlockSync>(c, st, g, s, tid);
  dog_checks_block(c, s, tid);
  if (tid >= 64) return;
  unsigned long long m[13];
  dog_mask_words(c, s, tid, m);
  uint32_t* out = mask + (size_t)g * kDogWords;
  if (tid < kDogWords) {
    unsigned long long x = m[0];
#pragma unroll
    for (int r = 1; r < 13; ++r)
      if ((tid >> 1) == r) x = m[r];
    out[tid] = (tid & 1) ? (uint32_t)(x >> 32) : (uint32_t)x;
  }
}

// Config (d)'s actor: `nturns` turns of one game per workgroup with the state resident in LDS --
// valid_actions -> uniform random legal action (turn0 + t) -> env_step, or no_step when nothing is legal
// -> deal if needed.  A finished game stops (action -2), or with `auto_reset` restarts in place
// (dog_reset_lds, deal counter continued) and keeps playing.  env_steps[g] (optional) accumulates the
// turns played and episodes[g] (optional) the games finished; action / reward / done (optional) are
// those of the last turn.
struct DogPlayArgs {
  DetConsts c;
  muz_dog_soa st;
  unsigned long long seed;
  int turn0, nturns, auto_reset;
  int32_t* action_out;   // optional outputs of the last turn
  int8_t* reward;
  uint8_t* done;
  uint32_t* env_steps;   // optional accumulators
  uint32_t* episodes;
  muz_dog_traj rec;      // optional per-turn records (rec.act == null: none)
};

// All arguments come in one struct that the kernel reads through the kernarg segment (kernarg0: scalar
// loads, the pointer laundered at each use), so the rule constants and the SoA pointers are reloaded where
// they are needed instead of being held live across the turn loop -- at the 64-VGPR budget that kept
// state spilled SGPRs into VGPR lanes and VGPRs into scratch.
__global__ __launch_bounds__(kDogPlayThreads) __attribute__((amdgpu_waves_per_eu(kDogPlayWPE))) void k_dog_play(
    DogPlayArgs args) {
  (void)args;
  __shared__ DogG s;
  const int tid = threadIdx.x, g = blockIdx.x;
  auto A = []() -> const DogPlayArgs& { return *(const DogPlayArgs*)kernarg0<DogPlayArgs>(); };
  if (A().st.done[g] && !A().auto_reset) {
    if (tid == 0) {
      if (A().action_out) A().action_out[g] = -2;
      if (A().reward) A().reward[g] = 0;
      if (A().done) A().done[g] = 1;
    }
    return;
  }
  dog_load<PlaySync>(A().c, A().st, g, s, tid);
#if MUZ_DOG_LEAN_CHECKS && MUZ_DOG_D7_LDS
  // the hot-7 distributions packed into LDS once per launch (the checks read them per lane every turn)
  __shared__ uint32_t s_d7[kDogHot];
  for (int i = tid; i < kDogHot; i += kDogPlayThreads)
    s_d7[i] = (uint32_t)(uint8_t)c_dists7[i][0] | ((uint32_t)(uint8_t)c_dists7[i][1] << 8) |
              ((uint32_t)(uint8_t)c_dists7[i][2] << 16) | ((uint32_t)(uint8_t)c_dists7[i][3] << 24);
  __syncthreads();
  const uint32_t* d7 = s_d7;
#else
  const uint32_t* d7 = nullptr;
#endif
#if MUZ_DOG_LEAN_CHECKS
  __shared__ DogCtx s_ctx;
  DogCtx* ctx = &s_ctx;
  if (tid == 0) dog_ctx_static(A().c, ctx);   // ordered before the first turn's reads by dog_checks_play's barrier
#else
  DogCtx* ctx = nullptr;
#endif
  const int nturns = A().nturns;
  int played = 0, finished = 0, a = -2, r = 0;
  DOG_STAMP_INIT();
  for (int t = 0; t < nturns; ++t) {
    const DogPlayArgs& P = A();
    const DetConsts& c = P.c;
    // s.done is block-uniform: its last writer (lane 0's env_step) is ordered before these reads by the
    // turn-end barrier.  When the game ended, the barrier below keeps dog_reset_lds's s.done = 0 (tid 0,
    // before its first barrier) from overtaking a wave that has not read s.done yet -- without it, such a
    // wave read 0, skipped the reset, and its barriers paired with the wrong ones of the other waves
    // (the run-to-run differences of round 1).
    if (s.done) {
      if (!P.auto_reset) break;
      const unsigned deal = s.deal;
      __syncthreads();
      dog_reset_lds<PlaySync>(c, s, P.seed, g, deal, tid);
    }
    DOG_STAMP(0);   // reset
    dog_checks_play<kDogPlayThreads>(c, s, tid, d7, ctx);
    DOG_STAMP(1);   // base checks (+ barrier)
    if (tid < 64) {
      // the turn's serial part (choice, lane 0's env_step) runs at raised wave priority: the CU's other
      // workgroups are in their VALU-heavy check phases meanwhile, and without it this wave got a small share
      // of the SIMD's issue slots
      if (MUZ_DOG_PRIO) __builtin_amdgcn_s_setprio(2);
      int nleg = 0;
      a = dog_pick(s, random_action_uniform(P.seed, g, P.turn0 + t), tid, &nleg);
      DOG_STAMP(2);   // action choice
      const int mover = s.cp;
      int need = 0;
      if (MUZ_DOG_WAVE_STEP && a >= 0 && s.phase == 0) {   // wave-uniform: the play phase on all 64 lanes
        int d = 0;
        need = dog_env_step_play_wave(c, s, a, tid, r, d);
      } else if (tid == 0) {                              // no_step and the swap phase: lane 0
        int d = s.done;
        r = 0;
        need = a < 0 ? dog_no_step(c, s) : dog_env_step(c, s, a, r, d, true);
      }
      if (tid == 0) {
        s.need_deal = need;
        if (P.rec.act) {   // the turn's record row (game lane g, row idx[g] + turns recorded this launch)
          const int row = P.rec.idx[g] + played;
          if (row < P.rec.max_steps) {
            const size_t o = (size_t)g * P.rec.max_steps + row;
            P.rec.act[o] = a;
            P.rec.player[o] = mover;
            P.rec.reward[o] = r;
            P.rec.legal[o] = nleg;
            P.rec.done[o] = (uint8_t)s.done;
          }
        }
      }
      DOG_STAMP(3);   // env_step / no_step (lane 0)
      if (MUZ_DOG_PRIO) __builtin_amdgcn_s_setprio(0);
    }
    ++played;
    __syncthreads();
    DOG_STAMP(4);   // barrier
    if (s.need_deal) dog_deal<PlaySync>(c, s, P.seed, g, tid);
    DOG_STAMP(5);   // deal
    finished += s.done;
  }
  DOG_STAMP_END();
  const DogPlayArgs& P = A();
  dog_store<PlaySync>(P.c, P.st, g, s, tid);
  if (tid == 0) {
    if (P.action_out) P.action_out[g] = a;
    if (P.reward) P.reward[g] = (int8_t)r;
    if (P.done) P.done[g] = (uint8_t)s.done;
    if (P.env_steps) P.env_steps[g] += (uint32_t)played;
    if (P.episodes) P.episodes[g] += (uint32_t)finished;
    if (P.rec.act) P.rec.idx[g] = min(P.rec.max_steps, P.rec.idx[g] + played);
  }
}

// mode 0: env_step(action[g]); mode 1: no_step.  action < 0 with mode 0 = no_step as well.
// restart != 0 (the MuZero self-play loop, muz_dog_step_restart): a game the step finished restarts in place after
// it (dog_reset_lds with the deal counter continued, as k_dog_play's auto reset) and episodes[g] counts it.
__global__ __launch_bounds__(256) void k_dog_step(DetConsts c, muz_dog_soa st, const int32_t* action, int mode,
                                                  unsigned long long seed, int8_t* reward, uint8_t* done, int n,
                                                  int restart = 0, uint32_t* episodes = nullptr) {
  __shared__ DogG sg[kDogGamesPerBlock];
  __shared__ int need_deal[kDogGamesPerBlock];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.x * kDogGamesPerBlock + w;
  if (g >= n) return;
  DogG& s = sg[w];
  dog_load<WaveSync>(c, st, g, s, lane);
  if (lane == 0) {
    int r = 0, d = s.done;
    int deal;
    if (mode == 1 || action[g] < 0) {
      deal = dog_no_step(c, s);
      r = 0;
      d = s.done;
    } else {
      deal = dog_env_step(c, s, action[g], r, d);
    }
    need_deal[w] = deal;
    if (reward) reward[g] = (int8_t)r;
    if (done) done[g] = (uint8_t)d;
  }
  wave_sync();
  if (need_deal[w]) dog_deal<WaveSync>(c, s, seed, g, lane);
  if (restart && s.done) {   // (one wave: every lane has read s.done before dog_reset_lds clears it)
    if (episodes && lane == 0) episodes[g] += 1u;
    dog_reset_lds<WaveSync>(c, s, seed, g, s.deal, lane);
  }
  dog_store<WaveSync>(c, st, g, s, lane);
}

// ---- DOG MuZero self-play records (config (e) as MuZero_DOG/train.py trains: play_n_games_v3's buffer dict) ------
// MuZero_DOG/game_agent.py:52-57 is `pass`; the det loop it copies (MuZero_det_MADN/game_agent.py:64-141) defines the
// record of a turn: obs (zeros on a no-move turn), action (-1), reward class {0: -1, 1: 0, 2: +1} of a game-ending
// step, root value, the search's action weights (zeros), mask (1 search turn, 0 no-move turn), the player and team
// BEFORE the move, and the discount class (1 terminal or no-move turn, 2 same team moves next, 0 the other team).
// One wave per lane (game in flight): the turn's record goes to row idx[slot] of the lane's trajectory slot
// (lane_game[g]; < 0: an idle lane, left untouched), then env_step / no_step as k_dog_step; a game that ended (done,
// or its max_steps-th record) restarts in place (deal counter continued) and sets ended[g] for k_dog_sp_assign.
constexpr int kDogObsBytes = 34 * kCells;   // (dog_nets.hpp kDogC x 56)

struct DogSpArgs {
  DetConsts c;
  muz_dog_soa st;
  const float* obs;         // [n][34][56] this turn's encode_board (the networks' input)
  const int32_t* action;    // [n] (-1: no legal action -> no_step)
  const float* weights;     // [n][806]
  const float* root_value;  // [n]
  unsigned long long seed;
  muz_traj traj;            // [num_games][T], obs int8 [34][56], pol [806]
  int32_t* lane_game;       // [n] trajectory slot of the lane's game, -1 idle
  int32_t* ended;           // [n] out: 1 when the lane's game ended this turn
  uint32_t* episodes;       // [n] nullable: finished (done) games per lane
  int n;
};

__global__ __launch_bounds__(256) void k_dog_sp_record_step(DogSpArgs P) {
  __shared__ DogG sg[kDogGamesPerBlock];
  __shared__ int sh_deal[kDogGamesPerBlock], sh_end[kDogGamesPerBlock];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.x * kDogGamesPerBlock + w;
  if (g >= P.n) return;
  const int slot = P.lane_game[g];
  if (slot < 0) {
    if (lane == 0) P.ended[g] = 0;
    return;
  }
  const DetConsts& c = P.c;
  DogG& s = sg[w];
  dog_load<WaveSync>(c, P.st, g, s, lane);
  const int T = P.traj.max_steps;
  const int t = P.traj.idx[slot];
  const int a = P.action[g];
  const int cp0 = s.cp;
  const size_t row = (size_t)slot * T + t;
  {   // the observation (int8, exact: values 0..110) and the policy of the turn
    const float* src = P.obs + (size_t)g * kDogObsBytes;
    int8_t* o = P.traj.obs + row * kDogObsBytes;
    for (int i = lane; i < kDogObsBytes; i += 64) o[i] = a >= 0 ? (int8_t)src[i] : (int8_t)0;
    const float* ws = P.weights + (size_t)g * kDogActions;
    float* pp = P.traj.pol + row * kDogActions;
    for (int i = lane; i < kDogActions; i += 64) pp[i] = a >= 0 ? ws[i] : 0.f;
  }
  int r = 0, d = 0;
  if (lane == 0) {
    int deal;
    if (a < 0) {
      deal = dog_no_step(c, s);
      d = s.done;
    } else {
      deal = dog_env_step(c, s, a, r, d);
    }
    sh_deal[w] = deal;
  }
  wave_sync();
  if (sh_deal[w]) dog_deal<WaveSync>(c, s, P.seed, g, lane);
  if (lane == 0) {
    const int cp1 = s.cp;     // next_env.current_player (after the step's deal)
    const bool teams = has(c.flags, R_TEAMS);
    const muz_traj& tr = P.traj;
    int rew = 1, disc = 1;
    if (a >= 0) {
      rew = (d && r > 0) ? 2 : ((d && r < 0) ? 0 : 1);
      disc = d ? 1 : ((teams ? (cp0 & 1) == (cp1 & 1) : cp0 == cp1) ? 2 : 0);
    }
    tr.act[row] = a >= 0 ? a : -1;
    tr.rew[row] = rew;
    tr.val[row] = a >= 0 ? P.root_value[g] : 0.f;
    tr.mask[row] = a >= 0 ? 1.f : 0.f;
    tr.player[row] = cp0;
    tr.team[row] = teams ? (cp0 & 1) : -1;
    tr.discount[row] = disc;
    tr.idx[slot] = t + 1;
    const int end = (d || t + 1 >= T) ? 1 : 0;
    P.ended[g] = end;
    sh_end[w] = end;
    if (P.episodes && d) P.episodes[g] += 1u;
  }
  wave_sync();
  if (sh_end[w]) dog_reset_lds<WaveSync>(c, s, P.seed, g, s.deal, lane);   // (every lane has read s.done / cp)
  dog_store<WaveSync>(c, P.st, g, s, lane);
}

// The lanes whose game ended take the next game numbers in lane order (one workgroup, deterministic): ctr[0] = next
// game number, ctr[1] = num_games, ctr[2] (out) = lanes still holding a game.  A lane past num_games goes idle.
__global__ __launch_bounds__(1024) void k_dog_sp_assign(int32_t* lane_game, const int32_t* ended, int32_t* idx,
                                                        int32_t* ctr, int n) {
  __shared__ int wsum[16];
  __shared__ int base_s, active_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) base_s = ctr[0], active_s = 0;
  __syncthreads();
  const int ng = ctr[1];
  for (int l0 = 0; l0 < n; l0 += 1024) {
    const int l = l0 + tid;
    const bool fin = l < n && lane_game[l] >= 0 && ended[l];
    const unsigned long long b = __ballot(fin);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int off = base_s;
    for (int k = 0; k < w; ++k) off += wsum[k];
    if (fin) {
      const int slot = off + pre;
      lane_game[l] = slot < ng ? slot : -1;
      if (slot < ng) idx[slot] = 0;
    }
    const int act = (l < n && lane_game[l] >= 0) ? 1 : 0;
    const int wa = __popcll(__ballot(act));
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int k = 0; k < 16; ++k) tot += wsum[k];
      base_s += tot;
    }
    if (lane == 0 && wa) atomicAdd(&active_s, wa);
    __syncthreads();
  }
  if (tid == 0) {
    ctr[0] = base_s;
    ctr[2] = active_s;
  }
}

// One step_* function of dog.py on its own (the form DOG/test.py calls): kind 0 step_swap(pin, pos),
// 1 step_normal_move(pin, move), 2 step_neg_move(pin, move), 3 step_hot_7(d0..d3).  Board and pins change;
// hands, turn and the state's reward / done fields do not (the reference returns them separately).
__global__ __launch_bounds__(256) void k_dog_step_move(DetConsts c, muz_dog_soa st, const int32_t* kind,
                                                       const int32_t* args, int8_t* reward, uint8_t* done, int n) {
  __shared__ DogG sg[kDogGamesPerBlock];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.x * kDogGamesPerBlock + w;
  if (g >= n) return;
  DogG& s = sg[w];
  dog_load<WaveSync>(c, st, g, s, lane);
  if (lane == 0) {
    const int cp = dog_sub(c, s);
    const int k = kind[g];
    const int a0 = args[4 * g], a1 = args[4 * g + 1];
    int r = 0, d = s.done;
    if (k == 0) {
      dog_step_swap(c, s, cp, a0 < 0 ? 0 : (a0 > 3 ? 3 : a0), a1 < 0 ? 0 : (a1 > kCells - 1 ? kCells - 1 : a1), r, d);
    } else if (k == 1) {
      dog_step_normal(c, s, cp, a0 & 3, a1, r, d);
    } else if (k == 2) {
      dog_step_neg(c, s, cp, a0 & 3, r, d, a1);
    } else {
      const int dd[4] = {args[4 * g], args[4 * g + 1], args[4 * g + 2], args[4 * g + 3]};
      dog_step_hot7(c, s, cp, dd, r, d);
    }
    if (reward) reward[g] = (int8_t)r;
    if (done) done[g] = (uint8_t)d;
  }
  dog_store<WaveSync>(c, st, g, s, lane);
}

// Uniform random legal action (config (d)'s policy): the k-th set bit, k = floor(u * popcount); -1 if none.
__global__ __launch_bounds__(256) void k_dog_random_action(const uint32_t* mask, const float* uniform,
                                                           unsigned long long seed, int turn, int32_t* action, int n) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint32_t* m = mask + (size_t)g * kDogWords;
  int tot = 0;
  for (int i = 0; i < kDogWords; ++i) tot += __popc(m[i]);
  if (tot == 0) {
    action[g] = -1;
    return;
  }
  const float u = uniform ? uniform[g] : random_action_uniform(seed, g, turn);
  int k = (int)(u * (float)tot);
  k = k >= tot ? tot - 1 : k;
  int a = -1;
  for (int i = 0; i < kDogWords && a < 0; ++i) {
    const int pc = __popc(m[i]);
    if (k < pc) {
      uint32_t x = m[i];
      for (int j = 0; j < k; ++j) x &= x - 1;   // drop the k lowest set bits
      a = i * 32 + __ffs(x) - 1;
    } else {
      k -= pc;
    }
  }
  action[g] = a;
}

}  // namespace muz

using namespace muz;

static inline unsigned dog_blocks(int n) { return (unsigned)((n + kDogGamesPerBlock - 1) / kDogGamesPerBlock); }

#define DOG_PROLOGUE(extra)                           \
  DetConsts c;                                        \
  int rc = dog_consts(rules, &c);                     \
  if (rc) return rc;                                  \
  MUZ_HOST_CHECK(n >= 0 && st.stride >= n && extra);  \
  if ((rc = dog_tables_ready())) return rc;           \
  if (n == 0) return MUZ_OK;

extern "C" {

#ifdef MUZ_DOG_STAMPS
int muz_diag_dog_stamps(unsigned long long* host_out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dog_stamps), sizeof(unsigned long long) * 8);
  if (e != hipSuccess) return (int)e;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_dog_stamps), z, sizeof(z));
  }
  return (int)e;
}
// per-wave check passes (dog_checks_play): host_out[24] (slot layout at g_dog_wave_stamps)
int muz_diag_dog_wave_stamps(unsigned long long* host_out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dog_wave_stamps), sizeof(unsigned long long) * 24);
  if (e != hipSuccess) return (int)e;
  if (reset) {
    unsigned long long z[24] = {0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_dog_wave_stamps), z, sizeof(z));
  }
  return (int)e;
}
#endif

int muz_dog_reset(const muz_rules* rules, muz_dog_soa st, uint64_t seed, int32_t n, void* stream) {
  DOG_PROLOGUE(true)
  k_dog_reset<<<dog_blocks(n), 256, 0, (hipStream_t)stream>>>(c, st, seed, n);
  return muz_last_launch_error();
}

int muz_dog_legal(const muz_rules* rules, muz_dog_soa st, uint32_t* mask, int32_t n, void* stream) {
  DOG_PROLOGUE(mask != nullptr)
  k_dog_legal<<<n, kDogBlockThreads, 0, (hipStream_t)stream>>>(c, st, mask, n);
  return muz_last_launch_error();
}

int muz_dog_step(const muz_rules* rules, muz_dog_soa st, const int32_t* action, uint64_t seed, int8_t* reward,
                 uint8_t* done, int32_t n, void* stream) {
  DOG_PROLOGUE(action != nullptr)
  k_dog_step<<<dog_blocks(n), 256, 0, (hipStream_t)stream>>>(c, st, action, 0, seed, reward, done, n);
  return muz_last_launch_error();
}

int muz_dog_step_restart(const muz_rules* rules, muz_dog_soa st, const int32_t* action, uint64_t seed, int8_t* reward,
                         uint8_t* done, uint32_t* episodes, int32_t n, void* stream) {
  DOG_PROLOGUE(action != nullptr)
  k_dog_step<<<dog_blocks(n), 256, 0, (hipStream_t)stream>>>(c, st, action, 0, seed, reward, done, n, 1, episodes);
  return muz_last_launch_error();
}

int muz_dog_sp_record_step(const muz_rules* rules, muz_dog_soa st, const float* obs, const int32_t* action,
                           const float* action_weights, const float* root_value, uint64_t seed, muz_traj traj,
                           int32_t* lane_game, int32_t* ended, uint32_t* episodes, int32_t n, void* stream) {
  DOG_PROLOGUE(obs && action && action_weights && root_value && lane_game && ended)
  MUZ_HOST_CHECK(c.P == 4 && traj.max_steps > 0 && traj.obs && traj.act && traj.rew && traj.val && traj.pol &&
                 traj.mask && traj.player && traj.team && traj.discount && traj.idx);
  k_dog_sp_record_step<<<dog_blocks(n), 256, 0, (hipStream_t)stream>>>(
      DogSpArgs{c, st, obs, action, action_weights, root_value, seed, traj, lane_game, ended, episodes, n});
  return muz_last_launch_error();
}

int muz_dog_sp_assign(int32_t* lane_game, const int32_t* ended, int32_t* traj_idx, int32_t* counters, int32_t n,
                      void* stream) {
  MUZ_HOST_CHECK(n >= 0 && lane_game && ended && traj_idx && counters);
  k_dog_sp_assign<<<1, 1024, 0, (hipStream_t)stream>>>(lane_game, ended, traj_idx, counters, n);
  return muz_last_launch_error();
}

int muz_dog_nostep(const muz_rules* rules, muz_dog_soa st, uint64_t seed, int8_t* reward, uint8_t* done, int32_t n,
                   void* stream) {
  DOG_PROLOGUE(true)
  k_dog_step<<<dog_blocks(n), 256, 0, (hipStream_t)stream>>>(c, st, nullptr, 1, seed, reward, done, n);
  return muz_last_launch_error();
}

int muz_dog_step_move(const muz_rules* rules, muz_dog_soa st, const int32_t* kind, const int32_t* args,
                      int8_t* reward, uint8_t* done, int32_t n, void* stream) {
  DOG_PROLOGUE(kind != nullptr && args != nullptr)
  k_dog_step_move<<<dog_blocks(n), 256, 0, (hipStream_t)stream>>>(c, st, kind, args, reward, done, n);
  return muz_last_launch_error();
}

int muz_dog_random_turn(const muz_rules* rules, muz_dog_soa st, uint64_t seed, int32_t turn, int32_t* action,
                        int8_t* reward, uint8_t* done, int32_t n, void* stream) {
  DOG_PROLOGUE(true)
  k_dog_play<<<n, kDogPlayThreads, 0, (hipStream_t)stream>>>(
      DogPlayArgs{c, st, seed, turn, 1, 0, action, reward, done, nullptr, nullptr});
  return muz_last_launch_error();
}

int muz_dog_random_play(const muz_rules* rules, muz_dog_soa st, uint64_t seed, int32_t turn0, int32_t nturns,
                        int32_t auto_reset, uint32_t* env_steps, uint32_t* episodes, int32_t n, void* stream) {
  DOG_PROLOGUE(nturns >= 0)
  if (nturns == 0) return MUZ_OK;
  k_dog_play<<<n, kDogPlayThreads, 0, (hipStream_t)stream>>>(
      DogPlayArgs{c, st, seed, turn0, nturns, auto_reset ? 1 : 0, nullptr, nullptr, nullptr, env_steps, episodes,
                  muz_dog_traj{}});
  return muz_last_launch_error();
}

int muz_dog_random_play_record(const muz_rules* rules, muz_dog_soa st, uint64_t seed, int32_t turn0, int32_t nturns,
                               int32_t auto_reset, uint32_t* env_steps, uint32_t* episodes, muz_dog_traj rec, int32_t n,
                               void* stream) {
  DOG_PROLOGUE(nturns >= 0)
  MUZ_HOST_CHECK(rec.act && rec.player && rec.reward && rec.legal && rec.done && rec.idx && rec.max_steps > 0);
  if (nturns == 0) return MUZ_OK;
  k_dog_play<<<n, kDogPlayThreads, 0, (hipStream_t)stream>>>(
      DogPlayArgs{c, st, seed, turn0, nturns, auto_reset ? 1 : 0, nullptr, nullptr, nullptr, env_steps, episodes, rec});
  return muz_last_launch_error();
}

int muz_dog_random_action(const uint32_t* mask, const float* uniform, uint64_t seed, int32_t turn, int32_t* action,
                          int32_t n, void* stream) {
  MUZ_HOST_CHECK(n >= 0 && mask && action);
  if (n == 0) return MUZ_OK;
  k_dog_random_action<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(mask, uniform, seed, turn, action, n);
  return muz_last_launch_error();
}

}  // extern "C"
