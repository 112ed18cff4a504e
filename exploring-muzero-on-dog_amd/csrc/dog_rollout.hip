// The network-free rollout agent for DOG (include/muz.h: muz_dog_rollout_search): a root-level Monte-Carlo search.
// Every legal root action is tried on copies of the game whose hidden cards are re-drawn, each copy is played out
// with the engine's random policy, and the root actions are thinned by sequential halving on their win counts.  The
// reference has no DOG agent, so parity with it is UNPINNED; the definition is tests/_dog_rollout.py, which these
// kernels equal bit for bit (every result is an integer sum, the same in any execution order).
//
// Launches of one search, all on the caller's stream and with no host synchronisation:
//   k_dog_rollout_init           per game: the candidate list C0 (the bits of muz_dog_legal's mask, ascending), zeroed
//                                wins / visits, and the answer of a forced game (done, nothing legal, one legal action)
//   per phase p = 0 .. max_phases - 1:
//     k_dog_rollout_plan         one workgroup: prefix sums of the candidate counts of the games still searching
//     k_dog_rollout              a fixed grid striding over the phase's (game, candidate, rollout) items; one
//                                workgroup plays one item with the copied game in LDS -- k_dog_play's turn loop, built
//                                from the same device functions (dog_env.hpp)
//     k_dog_rollout_rank         per game: ranks the candidates by (wins desc, action asc), keeps ceil(m / 2), writes
//                                the best one's action and value
// The turn loop is written out here rather than shared with k_dog_play as one function: k_dog_play's loop also resets,
// records and counts episodes, and its register allocation is what the DOG benchmark measures.
// The streams, the determinization and the item lookup are in dog_rollout.hpp, shared with dog_guided.hip, whose search
// is this one with its own rollout kernel: dog_rollout_check / dog_rollout_launch below take the phase's launch as a
// function.
#undef MUZ_DOG_STAMPS   // the stamps build instruments k_dog_play only (its counters live in env_dog.hip)
#include "dog_rollout.hpp"

namespace muz {

// ---- the candidate lists -----------------------------------------------------------------------------------------
// One workgroup per game, as k_dog_legal.  cand[g][0 .. ncand[g]) = the legal actions ascending; a finished game has
// none.  A game with fewer than two candidates is answered here and never searched.
__global__ __launch_bounds__(kDogBlockThreads) void k_dog_rollout_init(DetConsts c, muz_dog_soa st, int32_t* cand,
                                                                       int32_t* ncand, int32_t* wins, int32_t* visits,
                                                                       uint32_t* turns, int32_t* action, float* value,
                                                                       int n) {
  __shared__ DogG s;
  const int tid = threadIdx.x, g = blockIdx.x;
  for (int i = tid; i < kDogActions; i += kDogBlockThreads) {
    wins[(size_t)g * kDogActions + i] = 0;
    visits[(size_t)g * kDogActions + i] = 0;
  }
  dog_load<BlockSync>(c, st, g, s, tid);
  dog_checks_block(c, s, tid);
  if (tid >= 64) return;
  unsigned long long m[13];
  dog_mask_words(c, s, tid, m);
  const bool over = s.done != 0;
  int base = 0;
  int32_t* out = cand + (size_t)g * kDogActions;
#pragma unroll
  for (int r = 0; r < 13; ++r) {
    const unsigned long long w = over ? 0ull : m[r];
    if ((w >> tid) & 1ull) out[base + __popcll(w & ((1ull << tid) - 1ull))] = r * 64 + tid;
    base += __popcll(w);
  }
  if (tid == 0) {
    ncand[g] = base;
    turns[g] = 0u;
    value[g] = 0.f;
    action[g] = base == 1 ? kth_legal(m, 0.f) : -1;   // two or more: k_dog_rollout_rank writes it
  }
}

// Exclusive prefix sums of the candidate counts of the games still searching (ncand >= 2): off[g], off[n] = the sum.
constexpr int kPlanThreads = 1024;
__global__ __launch_bounds__(kPlanThreads) void k_dog_rollout_plan(const int32_t* ncand, int32_t* off, int n) {
  __shared__ int part[kPlanThreads];
  const int t = threadIdx.x;
  const int chunk = (n + kPlanThreads - 1) / kPlanThreads;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  int cnt = 0;
  for (int g = lo; g < hi; ++g) {
    const int m = ncand[g];
    cnt += m >= 2 ? m : 0;
  }
  part[t] = cnt;
  __syncthreads();
  for (int o = 1; o < kPlanThreads; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int pos = part[t] - cnt;
  for (int g = lo; g < hi; ++g) {
    off[g] = pos;
    const int m = ncand[g];
    pos += m >= 2 ? m : 0;
  }
  if (t == kPlanThreads - 1) off[n] = part[t];
}

// ---- the rollouts ------------------------------------------------------------------------------------------------
// Item i of a phase: candidate slot i / R of the phase's concatenated lists, rollout i % R of the phase.  The
// workgroup copies the root into LDS, determinizes it, applies the candidate (turn -1) and plays k_dog_play's turn
// until the game ends or `steps` turns are played.  Barriers: every wave takes the same ones.  The only exit from the
// turn loop is the s.done test of turns t >= 0 (see there); turn -1 always runs to its turn-end barrier.  s.done and
// s.need_deal are written by wave 0 after the check barrier (turn -1: after the barrier that follows the
// determinization) and before the turn-end barrier, and read by every wave after the turn-end barrier; the next
// item's load writes LDS only after the barrier at the head of the item loop, which every wave reaches after its last
// read of this item.  At most `steps` <= 1000 turns per item and off[n] * R < 2^31 - 2048 items per launch (the host
// checks n * 806 * R): the kernel always ends.
__global__ __launch_bounds__(kDogPlayThreads) __attribute__((amdgpu_waves_per_eu(kDogPlayWPE))) void k_dog_rollout(
    DogRolloutArgs args) {
  (void)args;
  __shared__ DogG s;
  __shared__ DogItem it;
  const int tid = threadIdx.x;
  auto A = []() -> const DogRolloutArgs& { return *(const DogRolloutArgs*)kernarg0<DogRolloutArgs>(); };
#if MUZ_DOG_LEAN_CHECKS && MUZ_DOG_D7_LDS
  __shared__ uint32_t s_d7[kDogHot];
  for (int i = tid; i < kDogHot; i += kDogPlayThreads)
    s_d7[i] = (uint32_t)(uint8_t)c_dists7[i][0] | ((uint32_t)(uint8_t)c_dists7[i][1] << 8) |
              ((uint32_t)(uint8_t)c_dists7[i][2] << 16) | ((uint32_t)(uint8_t)c_dists7[i][3] << 24);
  const uint32_t* d7 = s_d7;
#else
  const uint32_t* d7 = nullptr;
#endif
#if MUZ_DOG_LEAN_CHECKS
  __shared__ DogCtx s_ctx;
  DogCtx* ctx = &s_ctx;
  if (tid == 0) dog_ctx_static(A().c, ctx);   // read by wave 0 itself (dog_ctx_turn), after the item's barriers
#else
  DogCtx* ctx = nullptr;
#endif
  const int items = A().off[A().n] * A().R;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    if (tid == 0) dog_rollout_item(A(), item, it);
    __syncthreads();   // (also: every wave is done with the previous item's LDS state)
    dog_load<PlaySync>(A().c, A().st, it.g, s, tid);
    if (tid == 0) {
      it.side = has(A().c.flags, R_TEAMS) ? (s.cp & 1) : s.cp;   // the root mover's, before anything moves
      if (A().determinize) dog_determinize(A().c, s, it.rseed);
    }
    __syncthreads();
    // turn -1 is the root action (legal in the root; the determinization leaves the mover's hand and the board
    // alone), turns 0 .. steps - 1 are k_dog_play's
    const int steps = A().steps;
    int t = -1, r = 0;
    for (; t < steps; ++t) {
      const DetConsts& c = A().c;
      // s.done is tested from turn 0 on only.  At turn -1 no barrier lies between this point and wave 0's root step
      // (which writes s.done), so a late wave could see the new value, leave alone and pair its barriers with the
      // wrong ones of the others; and there is nothing to test: k_dog_rollout_init queues no finished root.  From
      // turn 0 on the read is ordered after the last write by the turn-end barrier (or the deal's closing one) and
      // before the next by the check barrier, so the exit is block-uniform.
      if (t >= 0 && s.done) break;
      if (t >= 0) dog_checks_play<kDogPlayThreads>(c, s, tid, d7, ctx);
      if (tid < 64) {
        if (MUZ_DOG_PRIO) __builtin_amdgcn_s_setprio(2);
        const int a = t < 0 ? it.a0 : dog_pick(s, random_action_uniform(it.rseed, it.gid, t), tid);
        int need = 0;
        if (MUZ_DOG_WAVE_STEP && a >= 0 && s.phase == 0) {
          int d = 0;
          need = dog_env_step_play_wave(c, s, a, tid, r, d);
        } else if (tid == 0) {
          int d = s.done;
          need = a < 0 ? dog_no_step(c, s) : dog_env_step(c, s, a, r, d, true);
        }
        if (tid == 0) s.need_deal = need;
        if (MUZ_DOG_PRIO) __builtin_amdgcn_s_setprio(0);
      }
      __syncthreads();
      if (s.need_deal) dog_deal<PlaySync>(c, s, it.rseed, it.gid, tid);
    }
    if (tid == 0) {   // the outcome for the root mover's side: +1 won, -1 somebody else won, 0 nobody (or the cap)
      const uint32_t w = dog_winners(A().c, s.board);
      const int z = w == 0u ? 0 : (((w >> it.side) & 1u) ? 1 : -1);
      if (z) atomicAdd(&A().wins[(size_t)it.g * kDogActions + it.a0], z);
      if (t > 0) atomicAdd(&A().turns[it.g], (uint32_t)t);   // random turns played (the root action is not one)
    }
  }
}

// ---- ranking -----------------------------------------------------------------------------------------------------
// One workgroup per game still searching: every candidate of the phase got R more visits; rank by (wins desc, action
// asc) by counting, keep the best ceil(m / 2) in rank order, and write the best one's action and value (the last
// ranking of a game is its answer).  value = float32(wins) / float32(visits), one IEEE division.
constexpr int kRankThreads = 256;
__global__ __launch_bounds__(kRankThreads) void k_dog_rollout_rank(int32_t* cand, int32_t* ncand, const int32_t* wins,
                                                                   int32_t* visits, int32_t* action, float* value,
                                                                   int R, int n) {
  __shared__ int sa[kDogActions], sw[kDogActions];
  const int tid = threadIdx.x, g = blockIdx.x;
  int m = ncand[g];
  if (m < 2) return;   // block-uniform: ncand[g] is written after the barrier below
  m = m > kDogActions ? kDogActions : m;
  const size_t row = (size_t)g * kDogActions;
  for (int i = tid; i < m; i += kRankThreads) {
    int a = cand[row + i];
    a = a < 0 ? 0 : (a >= kDogActions ? kDogActions - 1 : a);
    sa[i] = a;
    sw[i] = wins[row + a];
    visits[row + a] += R;
  }
  __syncthreads();
  const int keep = (m + 1) / 2;
  for (int i = tid; i < m; i += kRankThreads) {
    const int a = sa[i], w = sw[i];
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += (sw[j] > w) || (sw[j] == w && sa[j] < a);
    if (rank < keep) cand[row + rank] = a;
    if (rank == 0) {
      action[g] = a;
      value[g] = __fdiv_rn((float)w, (float)visits[row + a]);
    }
  }
  if (tid == 0) ncand[g] = keep;
}

static inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

static void dog_rollout_phase(unsigned grid, hipStream_t s, const DogRolloutArgs& args, const void*) {
  k_dog_rollout<<<grid, kDogPlayThreads, 0, s>>>(args);
}

int dog_rollout_check(const muz_rules* rules, const muz_dog_rollout_cfg* cfg, const muz_dog_soa& st,
                      const int32_t* action, const float* value, int32_t n, const void* ws, int64_t ws_bytes,
                      DetConsts* c, bool* go) {
  *go = false;
  MUZ_HOST_CHECK(rules && cfg && n >= 0 && st.stride >= n);
  MUZ_HOST_CHECK(cfg->rollouts >= 1 && cfg->rollouts <= 64 && cfg->max_phases >= 1 && cfg->max_phases <= 10 &&
                 cfg->rollout_steps >= 1 && cfg->rollout_steps <= 1000);
  // the item index of a phase (at most n * 806 * R, advanced by the grid's stride) and the prefix sums of the
  // candidate counts are int32
  MUZ_HOST_CHECK((int64_t)n * kDogActions * cfg->rollouts <= (int64_t)INT32_MAX - kRolloutGrid);
  int rc = dog_consts(rules, c);
  if (rc) return rc;
  if (n == 0) return MUZ_OK;
  MUZ_HOST_CHECK(action && value && ws && ((uintptr_t)ws & 15u) == 0 && ws_bytes >= muz_dog_rollout_bytes(n));
  MUZ_HOST_CHECK(st.board && st.pins && st.deck && st.hands && st.swap_choices && st.current_player &&
                 st.round_starter && st.phase && st.hand_size && st.reward && st.done && st.deal);
  if ((rc = dog_tables_ready())) return rc;
  *go = true;
  return MUZ_OK;
}

int dog_rollout_launch(const DetConsts& c, const muz_dog_rollout_cfg* cfg, muz_dog_soa st, const int32_t* game_id,
                       int32_t* action, float* value, int32_t* visits, int32_t* wins, uint32_t* rollout_turns,
                       int32_t n, void* ws, void* stream, DogRolloutPhase phase, const void* extra) {
  char* p = (char*)ws;
  const int64_t rows = up256((int64_t)n * kDogActions * 4);
  int32_t* w_wins = (int32_t*)p;
  int32_t* w_visits = (int32_t*)(p + rows);
  int32_t* cand = (int32_t*)(p + 2 * rows);
  int32_t* ncand = (int32_t*)(p + 3 * rows);
  uint32_t* w_turns = (uint32_t*)(p + 3 * rows + up256((int64_t)n * 4));
  int32_t* off = (int32_t*)(p + 3 * rows + 2 * up256((int64_t)n * 4));
  if (!wins) wins = w_wins;
  if (!visits) visits = w_visits;
  if (!rollout_turns) rollout_turns = w_turns;
  hipStream_t s = (hipStream_t)stream;
  k_dog_rollout_init<<<n, kDogBlockThreads, 0, s>>>(c, st, cand, ncand, wins, visits, rollout_turns, action, value, n);
  // a fixed grid: 8 workgroups per CU of a 256-CU device (4 resident, k_dog_play's budget), fewer for a small batch
  const int64_t most = (int64_t)n * kDogActions * cfg->rollouts;
  const unsigned grid = (unsigned)(most < kRolloutGrid ? most : kRolloutGrid);
  for (int ph = 0; ph < cfg->max_phases; ++ph) {
    k_dog_rollout_plan<<<1, kPlanThreads, 0, s>>>(ncand, off, n);
    phase(grid, s, DogRolloutArgs{c, st, game_id, cfg->seed, cfg->turn, ph, cfg->rollouts, cfg->rollout_steps,
                                  cfg->determinize ? 1 : 0, cand, off, wins, rollout_turns, n}, extra);
    k_dog_rollout_rank<<<n, kRankThreads, 0, s>>>(cand, ncand, wins, visits, action, value, cfg->rollouts, n);
  }
  return muz_last_launch_error();
}

}  // namespace muz

using namespace muz;

extern "C" {

// wins, visits and the candidate lists [n][806] int32, then the candidate counts [n], the rollout turns [n] and the
// item offsets [n + 1], each block rounded up to 256 bytes
int64_t muz_dog_rollout_bytes(int32_t n) {
  if (n < 0) return -1;
  const int64_t rows = up256((int64_t)n * kDogActions * 4);
  return 3 * rows + 2 * up256((int64_t)n * 4) + up256(((int64_t)n + 1) * 4);
}

int muz_dog_rollout_search(const muz_rules* rules, const muz_dog_rollout_cfg* cfg, muz_dog_soa st,
                           const int32_t* game_id, int32_t* action, float* value, int32_t* visits, int32_t* wins,
                           uint32_t* rollout_turns, int32_t n, void* ws, int64_t ws_bytes, void* stream) {
  DetConsts c;
  bool go = false;
  const int rc = dog_rollout_check(rules, cfg, st, action, value, n, ws, ws_bytes, &c, &go);
  if (rc || !go) return rc;
  return dog_rollout_launch(c, cfg, st, game_id, action, value, visits, wins, rollout_turns, n, ws, stream,
                            dog_rollout_phase, nullptr);
}

}  // extern "C"
