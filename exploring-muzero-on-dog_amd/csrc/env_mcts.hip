// Network-free MCTS agent for det-MADN: mctx muzero_policy whose model is the environment itself, with random-rollout
// leaf values (MADN/deterministic_madn.py:481-589 winning_action / policy_function / rollout / value_function /
// root_fn / recurrent_fn, driven by MADN/simulate_deterministicMADN.py:12-35; the same construction as
// TicTacToe/mcts.py:9-23) as ONE persistent kernel per batched search.
//
// The geometry and the simulation body are k_puct_search's (tree.hpp): a workgroup owns 16 games for the whole search,
// 32 lanes per game, lane a holds child a; root children in registers, node statistics and the path in SearchLds, the
// children arrays in the workspace.  What differs is the expansion: instead of Dyn4 + Pred4 a node's embedding is its
// 48-byte state row (kStateRow, kept in 64 B per node), the transition is env_step plus the no-move passes on the
// game's LDS rows, the prior is 100 legal + 200 wins, and the value a random rollout on a second LDS copy.  A game
// never leaves its half wave, so the simulation loop has no workgroup barrier: the two games of a wave run in
// lockstep, every other wave at its own pace (a rollout's length varies from 0 to rollout_steps turns).
//
// The semantics the reference leaves open (its rollout returns a shape-(4,) array and cannot run; its discount is -1
// even when the same side moves again) are fixed in tests/_env_mcts.py, which this kernel equals bit for bit:
//   node mask   valid_action of the node's state; a finished node, or one still without a legal action after the
//               passes, has mask 0 and counts as all 24 actions legal (a step there: reward 0 or -1, as env_step)
//   transition  env_step, then no_step while the state is not done and has no legal action (at most kMaxPasses)
//   discount    0 if done, +1 if the side to move is the side that moved, else -1
//   value       0 if done, else the rollout's outcome seen from the side to move (+1 / -1 / 0 at the cap)
//   rollout     a uniform pick among the winning actions if any, else among the legal ones: the k-th set bit,
//               k = min(floor(u count), count - 1), u from the counter RNG of (seed, game, turn, node, rollout turn)
#include "detmadn.hpp"
#include "host_consts.hpp"
#include "rng.hpp"
#include "tree.hpp"

namespace muz {

namespace {

constexpr int kMaxPasses = 4;       // the turn head's fast-forward cap (selfplay.hip)
constexpr int kNodeRow = 64;        // bytes of a node's state row in the workspace (kStateRow used)
constexpr int kMaxRollout = 1000;
constexpr unsigned long long kRolloutStream = 0x7011007D1CEull;
constexpr uint32_t kAllActions = 0xFFFFFFu;

// The tree's own carve: each game's count of rollout turns [n] (int32, read by the caller after the search), the six
// children arrays of NarrowTree<32>, then 64 B per node for its state row.  No latent slots.
struct EnvArrays : TreeArrays {
  int8_t* rows;
  int32_t* turns;
};
struct EnvTree : NarrowTree<32, EnvArrays> {
  __device__ __forceinline__ AS1 uint32_t* row(int g, int node) const {
    return reinterpret_cast<AS1 uint32_t*>(gpw(this->rows) + ((size_t)g * N + node) * kNodeRow);
  }
  static size_t head_bytes(int64_t n) { return ((size_t)n * 4 + 255) & ~(size_t)255; }
  static size_t bytes(int64_t n, int N) { return head_bytes(n) + 6 * child_bytes(n, N) + (size_t)n * N * kNodeRow; }
  static EnvTree carve(void* ws, int n, int N) {
    char* p = (char*)ws;
    EnvTree t;
    t.turns = (int32_t*)p;
    p += head_bytes(n);
    const size_t cb = child_bytes(n, N);
    t.c_index = (int32_t*)p;
    t.c_prior = (float*)(p + cb);
    t.c_value = (float*)(p + 2 * cb);
    t.c_visits = (int32_t*)(p + 3 * cb);
    t.c_reward = (float*)(p + 4 * cb);
    t.c_disc = (float*)(p + 5 * cb);
    t.emb = nullptr;
    t.rows = (int8_t*)(p + 6 * cb);
    t.N = N;
    return t;
  }
};

// A game's lanes hand LDS rows and tree words to each other inside their wave only: LDS and vector memory operations
// of one wave complete in order, so the compiler alone has to be held (no cache action, no wait).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The LDS rows of one game: its state row and its board
struct GameRows {
  int8_t* st;
  int8_t* bd;
  __device__ __forceinline__ BoardView board() const { return BoardView{bd, 1}; }
  __device__ __forceinline__ LdsLane lane() const { return LdsLane{st, st[40], st[41], st[42]}; }
};

__device__ __forceinline__ int side_of(const DetConsts& c, int p) { return has(c.flags, R_TEAMS) ? (p & 1) : p; }

// set_pins_on_board by the game's 32 lanes (rebuild_board's result: no two pins share a cell)
__device__ __forceinline__ void rebuild_board_g(const DetConsts& c, const GameRows& r, int a) {
  for (int cell = a; cell < kCells; cell += kRowLanes) r.bd[cell] = -1;
  wave_sync();
  if (a < 4 * c.P) {
    const int pos = r.st[a];
    if (pos >= 0 && pos < kCells) r.bd[pos] = (int8_t)(a >> 2);
  }
  wave_sync();
}

// wins(s): bit a set iff action a is legal and env_step(s, a) returns reward 1.  Only the move that brings the
// mover's (substituted player's) last pin from the track onto one of its goal cells can complete its goal -- pins in
// the goal are never hit -- so lane a evaluates env_step's landing cell of action a (det_step_masked's new_pos) and
// get_winner on the board with the mover's goal full.  tests/test_env_mcts_host.py compares this formulation with
// the trial steps.
__device__ __forceinline__ uint32_t det_wins_g(const DetConsts& c, const LdsLane& s, const BoardView& b, int a, int t,
                                               uint32_t legal) {
  const uint32_t F = c.flags;
  const int cp = sub_player(c, b, s.cp);
  const int g0 = goal_of(c, cp, 0), g3 = goal_of(c, cp, 3);
  int ng = 0, out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pos = pin_of(s, cp, k);
    const bool in = pos >= g0 && pos <= g3;
    ng += in ? 1 : 0;
    out = in ? out : k;
  }
  const int i = a / 6, m = a % 6 + 1;
  bool win = a < 24 && ((legal >> a) & 1u) && ng == 3 && i == out;
  if (win) {
    const int cur = pin_of(s, cp, i);
    const int tgt = cst(c.target, cp);
    const int x = cur + m - tgt - (has(F, R_MUST_TRAVERSE) ? 1 : 0);
    const int gx = goal_of(c, cp, jidx(x - 1, 4));
    const bool A = (b.at(gx) != cp) && (has(F, R_JUMP_GOAL) || goal_path_free(c, b, cp, -1, x));
    win = cur != -1 && 4 >= x && x > 0 && A && cur <= tgt;
    // get_winner with player cp done as well
    uint32_t d = 1u << cp;
#pragma unroll
    for (int p = 0; p < 4; ++p) d |= player_done(c, b, p) ? (1u << p) : 0u;
    if (has(F, R_TEAMS)) {
      const bool t0 = (d & 1u) && (d & 4u), t1 = (d & 2u) && (d & 8u);
      d = ((t0 && t1) || !(t0 || t1)) ? 0u : (t0 ? 0x5u : 0xAu);
    }
    win = win && ((d >> cp) & 1u);
  }
  const unsigned long long bal = __ballot(win);
  return (uint32_t)(bal >> (kRowLanes * ((t & 63) / kRowLanes))) & kAllActions;
}

// The mask of a node's state: valid_action, 0 for a finished game
__device__ __forceinline__ uint32_t node_legal(const DetConsts& c, const GameRows& r, int a, int t) {
  const LdsLane s = r.lane();
  const uint32_t lm = det_legal_g<kRowLanes>(c, s, r.board(), a, t);
  return s.done ? 0u : lm;
}

// A random rollout from the state in `from` (not finished), played on the copy `r` by the game's 32 lanes: lane a
// checks action a's legality and whether it wins, lane 0 picks and steps.  Returns the outcome seen from the side to
// move in `from`; `turns` counts the turns played.
__device__ __forceinline__ float rollout(const DetConsts& c, const GameRows& from, const GameRows& r, int a, int t,
                                         unsigned long long key, int node_key, int steps, int& turns) {
  if (a < kStateRow / 4) reinterpret_cast<uint32_t*>(r.st)[a] = reinterpret_cast<const uint32_t*>(from.st)[a];
  if (a < kCells / 4) reinterpret_cast<uint32_t*>(r.bd)[a] = reinterpret_cast<const uint32_t*>(from.bd)[a];
  wave_sync();
  const BoardView b = r.board();
  const int side0 = side_of(c, r.st[40]);
  for (int i = 0; i < steps; ++i) {
    LdsLane s = r.lane();
    if (s.done) break;   // uniform over the game's lanes
    const uint32_t lm = det_legal_g<kRowLanes>(c, s, b, a, t);
    const uint32_t wm = det_wins_g(c, s, b, a, t, lm);
    wave_sync();         // every lane has read the state the step below changes
    if (a == 0) {
      if (lm == 0u) {
        det_nostep(c, s);
      } else {
        const uint32_t cand = wm ? wm : lm;
        const int cnt = __popc(cand);
        const float u = u24(mix64(key ^ mix64(((unsigned long long)(unsigned)node_key << 16) | (unsigned)i)));
        int k = (int)(u * (float)cnt);
        k = k >= cnt ? cnt - 1 : k;
        uint32_t x = cand;
        for (int j = 0; j < k; ++j) x &= x - 1;   // drop the k lowest set bits
        const int act = __ffs(x) - 1;
        det_step_masked(c, s, b, act / 6, act % 6 + 1, lm);
      }
      r.st[40] = (int8_t)s.cp;
      r.st[41] = (int8_t)s.done;
      r.st[42] = (int8_t)s.reward;
    }
    ++turns;
    wave_sync();
  }
  const uint32_t w = winners(c, b);
  bool mine = false;
#pragma unroll
  for (int p = 0; p < 4; ++p) mine |= ((w >> p) & 1u) && side_of(c, p) == side0;
  return mine ? 1.f : (w ? -1.f : 0.f);
}

template <int QT>
__global__ __launch_bounds__(kThreads) void k_env_mcts(DetConsts c, PuctArgs pa, int rollout_steps,
                                                       muz_detmadn_soa st, const float* __restrict__ dirichlet_in,
                                                       const float* __restrict__ gumbel_in,
                                                       const int32_t* __restrict__ game_id, int n, EnvTree T,
                                                       int32_t* out_action, float* out_weights, float* out_value,
                                                       int32_t* out_visits, float* out_q) {
  // tree arithmetic exactly as written
#pragma clang fp contract(off)
  __shared__ SearchLds L;
  __shared__ float s_pbtab[kMaxNodes + 1];   // sqrt(N) * pb_c(N) for a node's visit count N = 0..S+1
  __shared__ uint32_t s_legal[kRows][kMaxNodes];   // every node's mask
  // the node being expanded (the root's state first) and the rollout's copy
  __shared__ __attribute__((aligned(16))) int8_t s_board[kRows][kCells], s_state[kRows][kStateRow];
  __shared__ __attribute__((aligned(16))) int8_t r_board[kRows][kCells], r_state[kRows][kStateRow];

  constexpr int A = MUZ_DET_ACTIONS;
  const int row = trow(), a = tsub();      // this lane holds action `a` of game `row`
  const int t = (int)tid();
  const int g0 = blockIdx.x * kRows;
  const int g = g0 + row;
  const bool valid = g < n;
  const bool ok = a < A;
  const int ai = ok ? a : 0;              // in-bounds alias for lanes a >= A
  const GameRows cur{s_state[row], s_board[row]}, roll{r_state[row], r_board[row]};

  if (tid() <= kMaxNodes) {
    const float N = (float)tid();
    const float pb_c = pa.pb_c_init + log_cr((N + pa.pb_c_base + 1.0f) / pa.pb_c_base);
    s_pbtab[tid()] = sqrtf(N) * pb_c;
  }
  det_rows_load<kRows>(c, st, g0, min(kRows, n - g0), s_board, s_state, t, kThreads);
  __syncthreads();

  // ---------------- root (root_fn: prior 100 legal + 200 wins, value a rollout; then policies.py muzero_policy:
  // _add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions, instantiate_tree_from_root)
  int gid = 0, turns = 0;
  unsigned long long rkey = 0;
  Kid rk;   // the root's children, in registers for the whole search (prior: the probability)
  rk.ok = ok;
  rk.prior = 0.f;
  rk.value = 0.f;
  rk.reward = 0.f;
  rk.disc = 0.f;
  rk.visits = 0;
  rk.index = -1;
  bool live = false;   // a root that is finished or has no legal action is not searched
  if (valid) {
    gid = game_id ? game_id[g] : g;
    rkey = game_key(pa.seed ^ kRolloutStream, gid, pa.turn);
    const uint32_t lm = node_legal(c, cur, a, t);
    const uint32_t wm = det_wins_g(c, cur.lane(), cur.board(), a, t, lm);
    live = lm != 0u;
    if (live) {
      if (a < kStateRow / 4) tree_st(T.row(g, 0) + a, reinterpret_cast<const uint32_t*>(cur.st)[a]);
      const float v = rollout(c, cur, roll, a, t, rkey, 0, rollout_steps, turns);
      const bool inv = !ok || ((lm >> a) & 1u) == 0u;
      const float lgt = 100.f * (float)((lm >> ai) & 1u) + 200.f * (float)((wm >> ai) & 1u);
      const float pr = row_softmax24(ok ? lgt : 0.f, ok);
      float dn = 0.f;
      if (dirichlet_in) {
        dn = ok ? dirichlet_in[(size_t)g * A + ai] : 0.f;
      } else if (pa.dir_frac != 0.f) {
        dn = row_softmax24(ok ? root_noise_log_gamma(pa.dir_alpha, pa.seed, gid, pa.turn, a) : 0.f, ok);
      }
      const float noisy = (1.f - pa.dir_frac) * pr + pa.dir_frac * dn;
      float lg = ok ? log_cr(fmaxf(noisy, kTinyF)) : -INFINITY;
      lg = lg - row_max(lg);
      rk.prior = row_softmax24(inv ? kFMin : lg, ok);
      if (a == 0) {
        s_legal[row][0] = lm;
        L.visits[row][0] = 1;
        L.val[row][0] = v;
      }
    }
  }
  wave_sync();

#pragma unroll 1
  for (int sim = 0; sim < pa.S; ++sim) {
    if (live) {
      // ---------------- simulate (search.py simulate): walk from the root
      const WalkEnd w = walk(T, L, rk, pa.D, [&](const Kid& k, int node, int depth) -> float {
        // muzero_action_selection: value_score + policy_score + 1e-7 U, masked by the node's mask
        const uint32_t nm = s_legal[row][node];
        const bool inv = !ok || (((nm ? nm : kAllActions) >> a) & 1u) == 0u;
        const float vs = value_score<QT>(k, L.val[row][node], pa);
        const float ps = s_pbtab[L.visits[row][node]] * k.prior / (float)(k.visits + 1);
        const float tb = tiebreak_uniform(pa.seed, gid, pa.turn, sim, depth, ai);
        return inv ? -INFINITY : vs + ps + 1e-7f * tb;
      });
      if (a == 0) L.hand_off(row, w, sim);
    }
    wave_sync();
    if (live) {
      // ---------------- expand (search.py expand): recurrent_fn is the environment
      const int par = L.parent[row], act = L.act[row], nx = L.next[row];
      if (a < kStateRow / 4) reinterpret_cast<uint32_t*>(cur.st)[a] = tree_ld(T.row(g, par) + a);
      wave_sync();
      rebuild_board_g(c, cur, a);
      const int side_p = side_of(c, cur.st[40]);
      wave_sync();   // every lane has read the mover before the step changes it
      if (a == 0) {
        LdsLane s = cur.lane();
        det_step_masked(c, s, cur.board(), act / 6, act % 6 + 1, s_legal[row][par]);
        cur.st[40] = (int8_t)s.cp;
        cur.st[41] = (int8_t)s.done;
        cur.st[42] = (int8_t)s.reward;
      }
      wave_sync();
      const float rw = (float)cur.st[42];
      uint32_t lm = node_legal(c, cur, a, t);
      for (int pass = 0; pass < kMaxPasses && !cur.st[41] && lm == 0u; ++pass) {   // uniform over the game's lanes
        wave_sync();
        if (a == 0) {
          LdsLane s = cur.lane();
          det_nostep(c, s);
          cur.st[40] = (int8_t)s.cp;
        }
        wave_sync();
        lm = node_legal(c, cur, a, t);
      }
      const bool fin = cur.st[41] != 0;
      const uint32_t wm = det_wins_g(c, cur.lane(), cur.board(), a, t, lm);
      const float dc = fin ? 0.f : (side_of(c, cur.st[40]) == side_p ? 1.f : -1.f);
      if (a < kStateRow / 4) tree_st(T.row(g, nx) + a, reinterpret_cast<const uint32_t*>(cur.st)[a]);
      if (a == 0) s_legal[row][nx] = lm;
      float v = 0.f;
      if (!fin) v = rollout(c, cur, roll, a, t, rkey, sim + 1, rollout_steps, turns);
      // the new node keeps its prior probabilities
      const bool inv = !ok || (((lm ? lm : kAllActions) >> a) & 1u) == 0u;
      const float lgt = 100.f * (float)((lm >> ai) & 1u) + 200.f * (float)((wm >> ai) & 1u);
      commit_expansion(T, L, rk, sim, row_softmax24(inv ? kFMin : lgt, ok), v, rw, dc);
      // ---------------- backward (search.py backward) along the recorded path
      commit_backup(T, L, rk, v, rw, dc);
    }
    wave_sync();
  }

  // ---------------- tail (policies.py muzero_policy: summary().visit_probs, _apply_temperature, categorical as
  // argmax(logits + Gumbel); summary().visit_counts / qvalues)
  if (!valid) return;
  const int vc = ok ? rk.visits : 0;
  const int tot = row_isum(vc);
  const float w = (float)vc / (float)max(tot, 1);
  float lw = ok ? log_cr(w) : -INFINITY;
  lw = (lw - row_max(lw)) / fmaxf(kTinyF, pa.temperature);
  const float gmb =
      ok ? (gumbel_in ? gumbel_in[(size_t)g * A + ai] : gumbel_noise(pa.seed ^ 0xC2B2AE3D27D4EB4Full, gid, pa.turn, ai))
         : 0.f;
  float sc = ok ? lw + gmb : -INFINITY;
  int bi = a;
  row_argmax(sc, bi);
  if (ok) {
    out_weights[(size_t)g * A + a] = live ? w : 0.f;
    if (out_visits) out_visits[(size_t)g * A + a] = vc;
    if (out_q) out_q[(size_t)g * A + a] = rk.reward + rk.disc * rk.value;
  }
  if (a == 0) {
    out_action[g] = live ? bi : -1;
    out_value[g] = live ? L.val[row][0] : 0.f;
    T.turns[g] = turns;
  }
}

}  // namespace

}  // namespace muz

using namespace muz;

extern "C" {

int64_t muz_detmadn_mcts_tree_bytes(int32_t n, const muz_puct_cfg* cfg) {
  if (!cfg || n < 0 || check_search_limits(cfg->num_simulations, cfg->max_depth)) return -1;
  return (int64_t)EnvTree::bytes(n, cfg->num_simulations + 1);
}

int muz_detmadn_mcts(const muz_rules* rules, const muz_puct_cfg* cfg, const muz_env_mcts_cfg* mcfg,
                     muz_detmadn_soa state, const float* dirichlet, const float* gumbel, const int32_t* game_id,
                     int32_t n, void* workspace, int64_t workspace_bytes, int32_t* action, float* action_weights,
                     float* root_value, int32_t* visit_counts, float* qvalues, void* stream) {
  if (!rules || !cfg || !mcfg) return MUZ_E_INVALID;
  DetConsts c;
  const int rc = make_det_consts(rules, &c);
  if (rc) return rc;
  if (check_puct_cfg(*cfg) || check_search_limits(cfg->num_simulations, cfg->max_depth)) return MUZ_E_UNSUPPORTED;
  if (mcfg->rollout_steps < 0 || mcfg->rollout_steps > kMaxRollout) return MUZ_E_UNSUPPORTED;
  MUZ_HOST_CHECK(n >= 0 && state.stride >= n && workspace && action && action_weights && root_value);
  MUZ_HOST_CHECK(state.board && state.pins && state.action_set && state.current_player && state.done && state.reward);
  MUZ_HOST_CHECK(((uintptr_t)workspace & 15u) == 0 &&
                 workspace_bytes >= (int64_t)EnvTree::bytes(n, cfg->num_simulations + 1));
  if (n == 0) return MUZ_OK;
  const PuctArgs pa = make_puct_args(*cfg);
  const EnvTree T = EnvTree::carve(workspace, n, pa.S + 1);
  const dim3 grid((n + kRows - 1) / kRows);
  hipStream_t s = (hipStream_t)stream;
  if (pa.qtransform == MUZ_QT_MIN_MAX)
    k_env_mcts<MUZ_QT_MIN_MAX><<<grid, kThreads, 0, s>>>(c, pa, mcfg->rollout_steps, state, dirichlet, gumbel, game_id,
                                                         n, T, action, action_weights, root_value, visit_counts,
                                                         qvalues);
  else
    k_env_mcts<MUZ_QT_PARENT_SIBLINGS><<<grid, kThreads, 0, s>>>(c, pa, mcfg->rollout_steps, state, dirichlet, gumbel,
                                                                 game_id, n, T, action, action_weights, root_value,
                                                                 visit_counts, qvalues);
  return muz_last_launch_error();
}

}  // extern "C"
