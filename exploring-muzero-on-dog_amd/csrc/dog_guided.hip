// The DOG rollout agent with greedy-guided playouts (include/muz.h: muz_dog_guided_rollout_search): the rollout agent's
// search (dog_rollout.hip: candidates, phases, sequential halving, determinization, streams) whose playout turns pick
// among the actions the greedy agent scores best instead of among all legal ones.  The reference has no DOG agent that
// runs, so parity with it is UNPINNED; the definition is tests/_dog_guided.py, which this kernel equals bit for bit
// (integer scores; the two float32 operations of a turn are the engine's own).
//
// One search is dog_rollout.hip's launches with k_dog_rollout_guided in k_dog_rollout's place (dog_rollout_launch).
// k_dog_rollout_guided is k_dog_rollout's item loop; a playout turn t >= 0 of a game that is not done:
//   all waves   read s.done, s.phase and the turn's explore flag (block-uniform, see the kernel), dog_checks_play
//   an explore or swap-phase turn is k_dog_rollout's from here: wave 0 picks the floor(u_t |C|)-th legal action
//   wave 0      the legal words s.wj / s.wr expanded to the ascending candidate list in LDS          | a greedy turn
//   -- barrier --                                                                                   |
//   every wave  with two candidates or more: strides over them -- the playout state read from LDS   |
//               into its 64 lanes' registers (DogWave), the candidate's transition on them with no  |
//               write-back, the six features, lane 0 writes the score to LDS (dog_score.hpp)        |
//   -- barrier (two candidates or more) --                                                          |
//   wave 0      the greatest score, the size of its argmax set M, the floor(u_t |M|)-th member      |
//   wave 0      the step (dog_env_step_play_wave / dog_env_step / dog_no_step), then the deal, as k_dog_rollout
// The turn loop is written out here rather than shared with k_dog_rollout as one function: k_dog_rollout's register
// allocation is what the rollout agent's numbers were measured with.
#undef MUZ_DOG_STAMPS   // the stamps build instruments k_dog_play only (its counters live in env_dog.hip)
#include <climits>
#include <cmath>

#include "dog_rollout.hpp"
#include "dog_score.hpp"

namespace muz {

// The explore draw of playout turn t (include/muz.h, DOG guided rollout agent): its own stream under the rollout's
// seed, so a turn's u_t (random_action_uniform) is the random playout's whether the turn explores or not.
constexpr unsigned long long kDogExploreStream = 0xE9B10AE0D6ull;

__device__ __forceinline__ float dog_explore_uniform(unsigned long long rseed, int gid, int turn) {
  return u24(mix64(game_key(rseed ^ kDogExploreStream, gid, turn)));
}

struct DogGuidedArgs {
  DogRolloutArgs r;
  int w[6];            // the greedy agent's weights
  float epsilon;       // a turn explores iff its explore draw < epsilon
  uint32_t* decided;   // [n], null: not counted
};

// k_dog_rollout (dog_rollout.hip) with the guided turn; its barrier argument holds for everything the two share.
// What the guided turn adds: `greedy` decides whether a wave takes the candidate-list barrier, `nc >= 2` whether it
// takes the scoring pass's.  Both are block-uniform:
//   explore   a function of the kernel arguments, t, and it.rseed / it.gid, which thread 0 writes before the barrier at
//             the head of the item loop and nobody writes again before the next item's;
//   s.phase   read where s.done is read, under the same argument: wave 0 writes it in its step or the deal writes it,
//             both before the turn-end barrier (the deal's closing one) of the turn before and, in this turn, only
//             after dog_checks_play's closing barrier, which every wave reaches after this read (dog_checks_play
//             reads s.phase at the same point itself);
//   nc        s_ncand, which wave 0 writes in a greedy turn before the candidate-list barrier, read after that barrier;
//             its next write follows the turn-end barrier.
// s_cand and s_score are written before the barrier their readers wait at (wave 0: the list; lane 0 of every wave: its
// candidates' scores) and not again before the turn-end barrier.  Loops: at most 792 candidates per turn (s.wj / s.wr
// hold 14 x 64 bits of which dog_checks_play sets the 2 x 396 checking slots at most), 13 ballot rounds in the pick.
__global__ __launch_bounds__(kDogPlayThreads) __attribute__((amdgpu_waves_per_eu(kDogPlayWPE)))
void k_dog_rollout_guided(DogGuidedArgs args) {
  (void)args;
  __shared__ DogG s;
  __shared__ DogItem it;
  __shared__ int s_score[kDogPlay];              // by position in the candidate list (at most 792 play actions)
  __shared__ unsigned short s_cand[kDogPlay];    // the legal actions of a greedy turn, ascending
  __shared__ int s_ncand;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto G = []() -> const DogGuidedArgs& { return *(const DogGuidedArgs*)kernarg0<DogGuidedArgs>(); };
  auto A = []() -> const DogRolloutArgs& { return ((const DogGuidedArgs*)kernarg0<DogGuidedArgs>())->r; };
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
    const int steps = A().steps;
    int t = -1, r = 0;
    for (; t < steps; ++t) {
      const DetConsts& c = A().c;
      // (s.done from turn 0 on only, and block-uniform there: k_dog_rollout)
      if (t >= 0 && s.done) break;
      bool greedy = false;
      if (t >= 0 && s.phase == 0) {   // the draw on scalar values: it.rseed / it.gid are the same in every lane
        const unsigned long long rs = it.rseed;
        const unsigned long long srs = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(rs >> 32)) << 32) |
                                       (unsigned)__builtin_amdgcn_readfirstlane((int)rs);
        greedy = !(dog_explore_uniform(srs, __builtin_amdgcn_readfirstlane(it.gid), t) < G().epsilon);
      }
      if (t >= 0) {
        // the checks' per-lane constants (table addresses, the lane's check) are recomputed every turn: hoisted out
        // of the turn loop they stay live across the scoring pass and cost it VGPRs it does not have
        int ctid = tid;
        asm volatile("" : "+v"(ctid));
        dog_checks_play<kDogPlayThreads>(c, s, ctid, d7, ctx);
      }
      int nc = 0;
      if (greedy) {
        if (wave == 0) {   // slot order is action order (dog_checks_play): joker copies, then real-card copies
          int base = 0;
#pragma unroll
          for (int wd = 0; wd < 14; ++wd) {
            const unsigned long long x = wd < 7 ? s.wj[wd] : s.wr[wd - 7];
            const int sl = (wd % 7) * 64 + lane;
            // (dog_checks_play sets the bits of the 396 checking slots only, so base + rank < 792)
            if ((x >> lane) & 1ull)
              s_cand[base + __popcll(x & ((1ull << lane) - 1ull))] =
                  (unsigned short)((wd < 7 ? 0 : kDogBase) + dog_base_of_slot(sl));
            base += __popcll(x);
          }
          if (lane == 0) s_ncand = base;
        }
        __syncthreads();
        nc = s_ncand;
        nc = nc > kDogPlay ? kDogPlay : nc;
        if (nc >= 2) {
          const int scp = s.cp;
          const int dist = kTrack / c.P;
          const unsigned all = (1u << c.P) - 1u;
          const unsigned me = (has(c.flags, R_TEAMS) ? ((scp & 1) ? 0xAu : 0x5u) : (1u << scp)) & all;
          DogWave R;
          R.lane = lane;
          R.cell = lane < kCells ? s.board[lane] : -1;
          R.pin = lane < 16 ? s.pins[lane] : -1;
          R.hand = 0;
          int prog0, goal0, home0;
          dog_player_stats(c, R.pin, lane, dist, prog0, goal0, home0);
          for (int i = wave; i < nc; i += kDogPlayThreads / 64) {
            const int a = __builtin_amdgcn_readfirstlane((int)s_cand[i]);
            int f[6];
            dog_afterstate_features(c, R, prog0, goal0, home0, lane, scp, dist, me, all, a, f);
            int sc = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) sc += G().w[k] * f[k];
            if (lane == 0) s_score[i] = sc;
          }
          __syncthreads();
        }
      }
      if (tid < 64) {
        if (MUZ_DOG_PRIO) __builtin_amdgcn_s_setprio(2);
        const float u = t < 0 ? 0.f : random_action_uniform(it.rseed, it.gid, t);
        int a;
        if (t < 0) {
          a = it.a0;
        } else if (!greedy) {
          a = dog_pick(s, u, tid);
        } else if (nc < 2) {
          a = nc == 1 ? (int)s_cand[0] : -1;
        } else {
          // M = the candidates with the greatest score; its floor(u |M|)-th member in list (= action) order
          int best = INT_MIN;
          for (int i = lane; i < nc; i += 64) best = max(best, s_score[i]);
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
          int cnt = 0;
          for (int b0 = 0; b0 < nc; b0 += 64)
            cnt += __popcll(__ballot(b0 + lane < nc && s_score[b0 + lane < nc ? b0 + lane : 0] == best));
          int k = (int)(u * (float)cnt);
          k = k >= cnt ? cnt - 1 : k;
          int idx = 0, seen = 0;
          bool found = false;
          for (int b0 = 0; b0 < nc; b0 += 64) {
            const bool hit = b0 + lane < nc && s_score[b0 + lane < nc ? b0 + lane : 0] == best;
            const unsigned long long x = __ballot(hit);
            const int pc = __popcll(x);
            if (!found && k < seen + pc) {
              const int before = __popcll(x & ((1ull << lane) - 1ull));
              idx = b0 + __ffsll((long long)__ballot(hit && before == k - seen)) - 1;
              found = true;
            }
            seen += pc;
          }
          idx = idx < 0 ? 0 : (idx >= nc ? nc - 1 : idx);
          a = (int)s_cand[idx];
        }
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
      if (z && G().decided) atomicAdd(&G().decided[it.g], 1u);
      if (t > 0) atomicAdd(&A().turns[it.g], (uint32_t)t);   // playout turns played (the root action is not one)
    }
  }
}

static void dog_guided_phase(unsigned grid, hipStream_t s, const DogRolloutArgs& args, const void* extra) {
  DogGuidedArgs g = *(const DogGuidedArgs*)extra;
  g.r = args;
  k_dog_rollout_guided<<<grid, kDogPlayThreads, 0, s>>>(g);
}

}  // namespace muz

using namespace muz;

extern "C" {

int muz_dog_guided_rollout_search(const muz_rules* rules, const muz_dog_guided_cfg* cfg, muz_dog_soa st,
                                  const int32_t* game_id, int32_t* action, float* value, int32_t* visits,
                                  int32_t* wins, uint32_t* rollout_turns, uint32_t* decided, int32_t n, void* ws,
                                  int64_t ws_bytes, void* stream) {
  MUZ_HOST_CHECK(cfg != nullptr);
  DogGuidedArgs g{};
  for (int k = 0; k < 6; ++k) {
    MUZ_HOST_CHECK(cfg->w[k] >= -32768 && cfg->w[k] <= 32767);
    g.w[k] = cfg->w[k];
  }
  MUZ_HOST_CHECK(cfg->epsilon >= 0.f && cfg->epsilon <= 1.f);   // (false for a NaN)
  g.epsilon = cfg->epsilon;
  g.decided = decided;
  DetConsts c;
  bool go = false;
  int rc = dog_rollout_check(rules, &cfg->rollout, st, action, value, n, ws, ws_bytes, &c, &go);
  if (rc || !go) return rc;
  if ((rc = dog_tables_ready())) return rc;   // this translation unit's own c_dists7 (dog_env.hpp)
  if (decided) MUZ_HIP_RET(hipMemsetAsync(decided, 0, (size_t)n * sizeof(uint32_t), (hipStream_t)stream));
  return dog_rollout_launch(c, &cfg->rollout, st, game_id, action, value, visits, wins, rollout_turns, n, ws, stream,
                            dog_guided_phase, &g);
}

}  // extern "C"
