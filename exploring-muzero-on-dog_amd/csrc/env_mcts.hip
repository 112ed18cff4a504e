// Network-free MCTS agent for det-MADN: mctx muzero_policy whose model is the environment itself, with random-rollout
// leaf values (MADN/deterministic_madn.py:481-589 winning_action / policy_function / rollout / value_function /
// root_fn / recurrent_fn, driven by MADN/simulate_deterministicMADN.py:12-35; the same construction as
// TicTacToe/mcts.py:9-23) as ONE persistent kernel per batched search.
//
// The geometry, the simulation body and the muzero_policy frame around it (pb_c table, noisy masked root prior, PUCT
// score, visit-count tail) are k_puct_search's (tree.hpp): a workgroup owns 16 games for the whole search,
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
#include "env_model.hpp"

namespace muz {

namespace {

// (EnvTree, GameRows, det_wins_g, node_legal, env_prior_logit, env_expand and rollout -- the environment as the
// search's model: env_model.hpp, shared with k_env_gumbel; its toolkit also with k_classic_env_mcts)

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

  fill_pb_table(s_pbtab, pa);
  det_rows_load<kRows>(c, st, g0, min(kRows, n - g0), s_board, s_state, t, kThreads);
  __syncthreads();

  // ---------------- root (root_fn: prior 100 legal + 200 wins, value a rollout; then policies.py muzero_policy:
  // _add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions, instantiate_tree_from_root)
  int gid = 0, turns = 0;
  unsigned long long rkey = 0;
  Kid rk = empty_kid(ok, 0.f);   // the root's children, in registers for the whole search (prior: the probability)
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
      const float pr = row_softmax24(ok ? env_prior_logit(lm, wm, ai) : 0.f, ok);
      const float dn = root_noise_share(dirichlet_in, (size_t)g * A + ai, ok, ok, pa, gid, pa.turn, a);
      rk.prior = root_prior(pr, dn, pa.dir_frac, inv, ok);
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
        // muzero_action_selection, masked by the node's mask
        const uint32_t nm = s_legal[row][node];
        const bool inv = !ok || (((nm ? nm : kAllActions) >> a) & 1u) == 0u;
        const float tb = tiebreak_uniform(pa.seed, gid, pa.turn, sim, depth, ai);
        return puct_score<QT>(k, L.val[row][node], L.visits[row][node], s_pbtab, tb, inv, pa);
      });
      if (a == 0) L.hand_off(row, w, sim);
    }
    wave_sync();
    if (live) {
      // ---------------- expand (search.py expand): recurrent_fn is the environment
      const int par = L.parent[row], nx = L.next[row];
      const EnvEdge e = env_expand(c, T, cur, g, par, L.act[row], nx, s_legal[row], a, t);
      const uint32_t lm = e.legal, wm = e.wins;
      const float rw = e.reward, dc = e.disc;
      if (a == 0) s_legal[row][nx] = lm;
      float v = 0.f;
      if (!e.done) v = rollout(c, cur, roll, a, t, rkey, sim + 1, rollout_steps, turns);
      // the new node keeps its prior probabilities
      const bool inv = !ok || (((lm ? lm : kAllActions) >> a) & 1u) == 0u;
      commit_expansion(T, L, rk, sim, row_softmax24(inv ? kFMin : env_prior_logit(lm, wm, ai), ok), v, rw, dc);
      // ---------------- backward (search.py backward) along the recorded path
      commit_backup(T, L, rk, v, rw, dc);
    }
    wave_sync();
  }

  // ---------------- tail (policies.py muzero_policy: summary().visit_probs, _apply_temperature, categorical as
  // argmax(logits + Gumbel); summary().visit_counts / qvalues)
  if (!valid) return;
  const float gmb = final_gumbel(gumbel_in, (size_t)g * A + ai, ok, pa.seed, gid, pa.turn, ai);
  const PolicyDraw pd = visit_policy(rk.visits, ok, pa.temperature, gmb);
  if (ok) {
    out_weights[(size_t)g * A + a] = live ? pd.weight : 0.f;
    if (out_visits) out_visits[(size_t)g * A + a] = rk.visits;
    if (out_q) out_q[(size_t)g * A + a] = rk.reward + rk.disc * rk.value;
  }
  if (a == 0) {
    out_action[g] = live ? pd.action : -1;
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
