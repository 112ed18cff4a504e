// Gumbel network-free MCTS agent for det-MADN: mctx gumbel_muzero_policy whose model is the environment itself, with
// random-rollout leaf values -- the call the reference drives (MADN/simulate_deterministicMADN.py:12-35 run_gumbel:
// mctx.gumbel_muzero_policy over root_fn / recurrent_fn of MADN/deterministic_madn.py:481-589 with
// qtransform_by_min_max(-1, 1)) -- as ONE persistent kernel per batched search.
//
// Two kernels joined: the geometry, the model and the expansion are k_env_mcts's (env_model.hpp: a workgroup owns 16
// games, 32 lanes per game, lane a holds child a; a node's embedding is its state row, the transition env_step plus
// the no-move passes, the prior 100 legal + 200 wins, the value a random rollout keyed by (seed, game, turn, node,
// rollout turn)); the search is k_gumbel_search's (tree.hpp: sequential halving at the root, completed-Q, softmax -
// visit share inside, no Dirichlet noise, no tie-break uniform, every argmax the first maximum).  A game never leaves
// its half wave, so the simulation loop has no workgroup barrier, only wave_sync().  The root's empty children
// (empty_kid) are tree.hpp's and the prior logit (env_prior_logit) env_model.hpp's, as in k_env_mcts.
//
// What the two parents leave open is fixed in tests/_env_gumbel.py, which this kernel equals bit for bit:
//   mask        every node is masked as in k_env_mcts (mctx masks the root only): the prior logit is FMIN outside the
//               node's mask and the interior score -inf there -- a legal child's softmax - visit share can be
//               negative, and an illegal unvisited child would score 0 and win.  A node with mask 0 (finished, or
//               still without a legal action after the passes) counts as all 24 actions legal.
//   priors      the tree keeps prior logits (k_gumbel_search), not probabilities (k_env_mcts); the root's are the
//               masked logits minus their maximum
//   qtransform  QT = MUZ_QT_COMPLETED_MIX: qtransform_completed_by_mix_value (completed_q, prior_probs of tree.hpp);
//               QT = MUZ_QT_MIN_MAX: qtransform_by_min_max(min_value, max_value) (value_score of tree.hpp), the
//               reference's call
//   raw values  a node's raw value is its rollout's outcome, -1, 0 or +1: an int8 per node in LDS
//   not searched  a root that is finished or has no legal action: action -1, weights 0, value 0
#include "env_model.hpp"

namespace muz {

namespace {

struct EnvGumbelArgs {
  int rollout_steps;
  float min_value, max_value;
};

template <int QT>
__global__ __launch_bounds__(kThreads, 4) void k_env_gumbel(DetConsts c, SearchArgs sa, EnvGumbelArgs ea,
                                                         muz_detmadn_soa st, const float* __restrict__ gumbel_in,
                                                         const int32_t* __restrict__ game_id, int n, EnvTree T,
                                                         int32_t* out_action, float* out_weights, float* out_value,
                                                         int32_t* out_visits, float* out_q) {
  // tree arithmetic exactly as written
#pragma clang fp contract(off)
  static_assert(QT == MUZ_QT_COMPLETED_MIX || QT == MUZ_QT_MIN_MAX, "k_env_gumbel: completed-by-mix or min-max");
  __shared__ SearchLds L;
  __shared__ uint32_t s_legal[kRows][kMaxNodes];   // every node's mask
  __shared__ int8_t s_raw[kRows][kMaxNodes];       // every node's raw value: its rollout's outcome
  __shared__ uint8_t s_cv[kRows][kMaxSims];        // the game's sequence of considered visits
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
  PuctArgs mm;                            // value_score<MUZ_QT_MIN_MAX> reads the two bounds only
  mm.min_value = ea.min_value;
  mm.max_value = ea.max_value;

  det_rows_load<kRows>(c, st, g0, min(kRows, n - g0), s_board, s_state, t, kThreads);
  __syncthreads();

  // ---------------- root (root_fn: prior 100 legal + 200 wins, value a rollout; then policies.py
  // gumbel_muzero_policy: _mask_invalid_actions, instantiate_tree_from_root)
  int turns = 0;
  unsigned long long rkey = 0;
  uint32_t lb = 0;                        // the root's mask
  float gum = 0.f;
  float rpp = 0.f, rpm = 0.f;             // prior_probs of the root's children and its largest prior
  Kid rk = empty_kid(ok, kFMin);   // the root's children, in registers for the whole search (prior: the logit)
  bool live = false;   // a root that is finished or has no legal action is not searched
  if (valid) {
    const int gid = game_id ? game_id[g] : g;
    rkey = game_key(sa.seed ^ kRolloutStream, gid, sa.turn);
    lb = node_legal(c, cur, a, t);
    const uint32_t wm = det_wins_g(c, cur.lane(), cur.board(), a, t, lb);
    live = lb != 0u;
    if (live) {
      if (a < kStateRow / 4) tree_st(T.row(g, 0) + a, reinterpret_cast<const uint32_t*>(cur.st)[a]);
      const float v = rollout(c, cur, roll, a, t, rkey, 0, ea.rollout_steps, turns);
      const bool inv = !ok || ((lb >> a) & 1u) == 0u;
      const float l = ok ? env_prior_logit(lb, wm, ai) : -INFINITY;
      const float lm = row_max(l);
      rk.prior = inv ? kFMin : l - lm;
      if (ok)
        gum = gumbel_in ? gumbel_in[(size_t)g * A + ai] : sa.gumbel_scale * gumbel_noise(sa.seed, gid, sa.turn, ai);
      rpp = prior_probs(rk.prior, ok, rpm);
      // (read by this row's lanes only, one wave)
      fill_considered_visits(s_cv[row], min(sa.max_considered, __popc(lb)), sa.S, a, kRowLanes);
      if (a == 0) {
        s_legal[row][0] = lb;
        L.visits[row][0] = 1;
        s_raw[row][0] = (int8_t)v;
        L.val[row][0] = v;
      }
    }
  }
  wave_sync();

  // this lane's completed Q-value of node `node`'s child k (pp: prior_probs of the node's children, used by the
  // completed-by-mix form only); sumv: the children's visits summed
  auto cq_of = [&](const Kid& k, float pp, int node, int& sumv) -> float {
    if constexpr (QT == MUZ_QT_MIN_MAX) {
      sumv = row_isum(k.ok ? k.visits : 0);
      return value_score<MUZ_QT_MIN_MAX>(k, 0.f, mm);
    } else {
      return completed_q(k, pp, (float)s_raw[row][node], sa, sumv);
    }
  };

#pragma unroll 1
  for (int sim = 0; sim < sa.S; ++sim) {
    if (live) {
      // ---------------- simulate (search.py simulate): walk from the root
      const WalkEnd w = walk(T, L, rk, sa.D, [&](const Kid& k, int node, int depth) -> float {
        int sumv;
        if (depth == 0) {
          // gumbel_muzero_root_action_selection: score_considered + masked_argmax (sumv: this simulation's index)
          const float cq = cq_of(k, rpp, 0, sumv);
          const int cv = s_cv[row][sumv];
          const float s = fmaxf(-1e9f, gum + (k.prior - rpm) + cq) + (k.visits == cv ? 0.f : -INFINITY);
          return (!ok || ((lb >> a) & 1u) == 0u) ? -INFINITY : s;
        }
        // gumbel_muzero_interior_action_selection: softmax(prior + cq) - N / (1 + sum N), masked by the node's mask
        const uint32_t nm = s_legal[row][node];
        const bool inv = !ok || (((nm ? nm : kAllActions) >> a) & 1u) == 0u;
        float pp = 0.f;
        if constexpr (QT != MUZ_QT_MIN_MAX) {
          float pmax;
          pp = prior_probs(k.prior, k.ok, pmax);
        }
        const float cq = cq_of(k, pp, node, sumv);
        const float z = k.prior + cq;
        const float zm = row_max(ok ? z : -INFINITY);
        const float ez = ok ? exp_cr(z - zm) : 0.f;
        const float zs = row_sum24(ez);
        return inv ? -INFINITY : (ez / zs - (float)k.visits / (float)(1 + sumv));
      });
      if (a == 0) L.hand_off(row, w, sim);
    }
    wave_sync();
    if (live) {
      // ---------------- expand (search.py expand): recurrent_fn is the environment
      const int par = L.parent[row], nx = L.next[row];
      const EnvEdge e = env_expand(c, T, cur, g, par, L.act[row], nx, s_legal[row], a, t);
      if (a == 0) s_legal[row][nx] = e.legal;
      float v = 0.f;
      if (!e.done) v = rollout(c, cur, roll, a, t, rkey, sim + 1, ea.rollout_steps, turns);
      // the new node keeps its prior logits
      const bool inv = !ok || (((e.legal ? e.legal : kAllActions) >> a) & 1u) == 0u;
      commit_expansion(T, L, rk, sim, inv ? kFMin : env_prior_logit(e.legal, e.wins, ai), v, e.reward, e.disc);
      if (a == 0) s_raw[row][nx] = (int8_t)v;
      // ---------------- backward (search.py backward) along the recorded path
      commit_backup(T, L, rk, v, e.reward, e.disc);
    }
    wave_sync();
  }

  // ---------------- final action + action_weights (policies.py gumbel_muzero_policy tail); summary().visit_counts /
  // qvalues
  if (!valid) return;
  int bi = -1;
  float wgt = 0.f;
  if (live) {
    int sumv;
    const float cq = cq_of(rk, rpp, 0, sumv);
    const bool inv = !ok || ((lb >> a) & 1u) == 0u;
    const int cv = row_imax(rk.visits);   // considered_visit = max(visit_counts)
    float sc = fmaxf(-1e9f, gum + (rk.prior - rpm) + cq) + (rk.visits == cv ? 0.f : -INFINITY);
    sc = inv ? -INFINITY : sc;
    bi = a;
    row_argmax(sc, bi);
    // action_weights = softmax(_mask_invalid_actions(prior + completed_q))
    const float z = rk.prior + cq;
    const float zm = row_max(ok ? z : -INFINITY);
    const float zz = inv ? kFMin : z - zm;
    const float m2 = row_max(ok ? zz : -INFINITY);
    const float ez = ok ? exp_cr(zz - m2) : 0.f;
    const float zs = row_sum24(ez);
    wgt = ez / zs;
  }
  if (ok) {
    out_weights[(size_t)g * A + a] = wgt;
    if (out_visits) out_visits[(size_t)g * A + a] = rk.visits;
    if (out_q) out_q[(size_t)g * A + a] = rk.reward + rk.disc * rk.value;
  }
  if (a == 0) {
    out_action[g] = bi;
    out_value[g] = live ? L.val[row][0] : 0.f;
    T.turns[g] = turns;
  }
}

}  // namespace

}  // namespace muz

using namespace muz;

extern "C" {

int muz_detmadn_gumbel_mcts(const muz_rules* rules, const muz_search_cfg* cfg, const muz_env_gumbel_cfg* gcfg,
                            muz_detmadn_soa state, const float* gumbel, const int32_t* game_id, int32_t n,
                            void* workspace, int64_t workspace_bytes, int32_t* action, float* action_weights,
                            float* root_value, int32_t* visit_counts, float* qvalues, void* stream) {
  if (!rules || !cfg || !gcfg) return MUZ_E_INVALID;
  DetConsts c;
  const int rc = make_det_consts(rules, &c);
  if (rc) return rc;
  if (check_search_limits(cfg->num_simulations, cfg->max_depth) || cfg->max_num_considered < 1)
    return MUZ_E_UNSUPPORTED;
  // (written so that a NaN is refused too)
  if (!(cfg->gumbel_scale >= 0.f) || !(cfg->value_scale >= 0.f) || !(cfg->maxvisit_init >= 0.f))
    return MUZ_E_UNSUPPORTED;
  if (gcfg->rollout_steps < 0 || gcfg->rollout_steps > kMaxRollout) return MUZ_E_UNSUPPORTED;
  if (gcfg->qtransform != MUZ_QT_MIN_MAX && gcfg->qtransform != MUZ_QT_COMPLETED_MIX) return MUZ_E_UNSUPPORTED;
  if (!(gcfg->max_value > gcfg->min_value)) return MUZ_E_UNSUPPORTED;
  MUZ_HOST_CHECK(n >= 0 && state.stride >= n && workspace && action && action_weights && root_value);
  MUZ_HOST_CHECK(state.board && state.pins && state.action_set && state.current_player && state.done && state.reward);
  MUZ_HOST_CHECK(((uintptr_t)workspace & 15u) == 0 &&
                 workspace_bytes >= (int64_t)EnvTree::bytes(n, cfg->num_simulations + 1));
  if (n == 0) return MUZ_OK;
  const SearchArgs sa = make_search_args(*cfg);
  const EnvGumbelArgs ea{gcfg->rollout_steps, gcfg->min_value, gcfg->max_value};
  const EnvTree T = EnvTree::carve(workspace, n, sa.S + 1);
  const dim3 grid((n + kRows - 1) / kRows);
  hipStream_t s = (hipStream_t)stream;
  if (gcfg->qtransform == MUZ_QT_MIN_MAX)
    k_env_gumbel<MUZ_QT_MIN_MAX><<<grid, kThreads, 0, s>>>(c, sa, ea, state, gumbel, game_id, n, T, action,
                                                           action_weights, root_value, visit_counts, qvalues);
  else
    k_env_gumbel<MUZ_QT_COMPLETED_MIX><<<grid, kThreads, 0, s>>>(c, sa, ea, state, gumbel, game_id, n, T, action,
                                                                 action_weights, root_value, visit_counts, qvalues);
  return muz_last_launch_error();
}

}  // extern "C"
