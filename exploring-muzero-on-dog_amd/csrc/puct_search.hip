// Batched PUCT MuZero search for det-MADN (mctx 0.0.6 muzero_policy: the call run_muzero_mcts keeps commented beside
// the Gumbel one, MuZero_det_MADN/muzero_deterministic_madn.py:685-697) as ONE persistent kernel per search.
//
// The geometry and the expansion are k_gumbel_search's (search.hip), the simulation body (walk, expansion and backup
// commits) the one both take from tree.hpp: a workgroup owns 16 games for the whole search, 32 lanes per game, lane a
// holds child a; root children in registers, node scalars and the path in LDS, children arrays and node embeddings in
// the workspace; Dyn4 + Pred4 on MFMA over the 16-row tile.  What differs:
//   root    -- Dirichlet noise mixed into softmax(root_logits), log, mask (policies.py muzero_policy);
//   select  -- muzero_action_selection at every level: qtransform + sqrt(N) pb_c(N) softmax(prior) / (n + 1) + 1e-7 U,
//              the root mask at depth 0;
//   tail    -- visit-count action weights, temperature, Gumbel-max draw (as k_stochastic_search's).
// A node's children keep softmax(prior logits) instead of the logits (c_prior, written once at expansion): the walks
// read the probabilities only.  sqrt(N) pb_c(N) is tabulated once per search for every visit count a node can reach.
// The root prior, the score and the tail are tree.hpp's muzero_policy frame (fill_pb_table, root_noise_share,
// root_prior, puct_score, final_gumbel, visit_policy), shared with k_env_mcts and k_classic_env_mcts; the noise is
// not drawn at dirichlet_fraction 0, where its share is multiplied by 0.
#include "tree.hpp"

namespace muz {

namespace {

template <int QT>
__global__ __launch_bounds__(kThreads, 1) void k_puct_search(
    muz_net_w Wt, PuctArgs pa, const float* __restrict__ root_logits, const float* __restrict__ root_value,
    const float* __restrict__ root_emb, const uint32_t* __restrict__ legal, const float* __restrict__ dirichlet_in,
    const float* __restrict__ gumbel_in, const int32_t* __restrict__ game_id, int n, const int* __restrict__ n_dev,
    TreeWs T, int32_t* out_action, float* out_weights, float* out_value) {
  // tree arithmetic exactly as written; the networks (nn.hpp) keep their own contraction
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float smem[kArenaFloats];
  __shared__ SearchLds L;
  __shared__ float s_pbtab[kMaxNodes + 1];   // sqrt(N) * pb_c(N) for a node's visit count N = 0..S+1

  if (n_dev) n = *n_dev;
  if ((int)blockIdx.x * kRows >= n) return;
  const Arena ar = Arena::carve(smem);
  const int A = Wt.num_actions;
  const int row = trow(), a = tsub();      // this lane holds action `a` of game `row`
  const int g = blockIdx.x * kRows + row;
  const bool valid = g < n;
  const bool ok = a < A;
  const int ai = ok ? a : 0;              // in-bounds alias for lanes a >= A

  fill_pb_table(s_pbtab, pa);

  // ---------------- root (policies.py muzero_policy: _add_dirichlet_noise, _get_logits_from_probs,
  // _mask_invalid_actions; then instantiate_tree_from_root)
  unsigned lb = 0;
  int gid = 0, gturn = pa.turn;
  Kid rk = empty_kid(ok, 0.f);   // the root's children, in registers for the whole search (prior: the probability)
  bool inv = true;
  if (valid) {
    lb = legal[g];
    // the noise keys of every draw below (see SearchArgs): the game's number and its own step count
    const int lane = game_id ? game_id[g] : g;
    gid = pa.key_game ? pa.key_game[lane] : lane;
    gturn = pa.key_turn ? pa.key_turn[gid] : pa.turn;
    inv = !ok || ((lb >> a) & 1u) == 0u;
    const float pr = row_softmax24(ok ? root_logits[(size_t)g * A + ai] : 0.f, ok);
    const float dn = root_noise_share(dirichlet_in, (size_t)g * A + ai, ok, ok, pa, gid, gturn, a);
    rk.prior = root_prior(pr, dn, pa.dir_frac, inv, ok);
    AS1 float* e0 = T.e(g, 0);
    for (int c = a; c < LAT; c += kRowLanes) e0[c] = root_emb[(size_t)g * LAT + c];
    if (a == 0) {
      const float v = root_value[g];
      L.visits[row][0] = 1;
      L.val[row][0] = v;
    }
  }
  __syncthreads();

  st_begin();
  Pf pf;   // first k-blocks of the next dense layer (crosses the select / expand phases)
  pf_issue<NT256>(pf, &kernarg0<muz_net_w>()->dyn.d3, LAT, LAT);
#pragma unroll 1
  for (int sim = 0; sim < pa.S; ++sim) {
    st_sim(sim);
    const AS4 muz_net_w* wl = kernarg0<muz_net_w>();   // (see k_gumbel_search)
    DynIn din;
    int dact = 0;
    // ---------------- simulate (search.py simulate): walk from the root
    if (valid) {
      const WalkEnd w = walk(T, L, rk, pa.D, [&](const Kid& k, int node, int depth) -> float {
        // muzero_action_selection, masked at the root
        const float tb = tiebreak_uniform(pa.seed, gid, gturn, sim, depth, ai);
        return puct_score<QT>(k, L.val[row][node], L.visits[row][node], s_pbtab, tb, !ok || (depth == 0 && inv), pa);
      });
      // expand's inputs (parent embedding, FiLM rows of the action): issued by the game's own lanes now
      din = dyn_load(wl->dyn, A, T.e(g, w.node), w.act);
      dact = w.act;
      if (a == 0) L.hand_off(row, w, sim);
    } else {
      din = dyn_load(wl->dyn, A, nullptr, 0);
      if (a == 0) L.act[row] = 0;
    }
    ST(ST_SEL);
    SYNC();
    // ---------------- expand (search.py expand): recurrent_fn on the 16 parents, as k_gumbel_search does
    const int nx = L.next[row];
    dyn16<NT256, true, kLateHeads>(wl->dyn, A, din, dact, ar, pf, &wl->pred.rb[0].d0, LAT, LAT, &wl->pred.ln0,
                                   valid ? T.e(g, nx) : nullptr);
    pred16<NT256, true, kLateHeads, kSplitkLogits>(wl->pred, A, ar.T, ar, pf, &wl->dyn.d3, LAT, LAT, &wl->dyn, dact);
    if (valid) {
      // the new node keeps its prior probabilities
      const float v = ar.v0[row], rw = ar.v1[row], dc = ar.v2[row];
      commit_expansion(T, L, rk, sim, row_softmax24(ar.U[row * LD + ai], ok), v, rw, dc);
      // ---------------- backward (search.py backward) along the recorded path
      commit_backup(T, L, rk, v, rw, dc);
    }
    ST(ST_TREE);
    SYNC();
  }
  st_end();

  // ---------------- tail (policies.py muzero_policy: summary().visit_probs, _apply_temperature, categorical as
  // argmax(logits + Gumbel))
  if (valid) {
    const float gmb = final_gumbel(gumbel_in, (size_t)g * A + ai, ok, pa.seed, gid, gturn, ai);
    const PolicyDraw pd = visit_policy(rk.visits, ok, pa.temperature, gmb);
    if (ok) out_weights[(size_t)g * A + a] = pd.weight;
    if (a == 0) {
      out_action[g] = pd.action;
      out_value[g] = L.val[row][0];
    }
  }
}

}  // namespace

int launch_puct_search(const muz_net_w& w, const PuctArgs& pa, const float* root_logits, const float* root_value,
                       const float* root_emb, const uint32_t* legal, const float* dirichlet, const float* gumbel,
                       const int32_t* game_id, int n, const int* n_dev, void* workspace, int32_t* action,
                       float* weights, float* value, hipStream_t s) {
  const TreeWs T = TreeWs::carve(workspace, n, pa.S + 1);
  const dim3 grid((n + kRows - 1) / kRows);
  if (pa.qtransform == MUZ_QT_MIN_MAX)
    k_puct_search<MUZ_QT_MIN_MAX><<<grid, kThreads, 0, s>>>(w, pa, root_logits, root_value, root_emb, legal, dirichlet,
                                                            gumbel, game_id, n, n_dev, T, action, weights, value);
  else
    k_puct_search<MUZ_QT_PARENT_SIBLINGS><<<grid, kThreads, 0, s>>>(w, pa, root_logits, root_value, root_emb, legal,
                                                                    dirichlet, gumbel, game_id, n, n_dev, T, action,
                                                                    weights, value);
  return muz_last_launch_error();
}

}  // namespace muz

using namespace muz;

extern "C" {

int muz_puct_search(const muz_net_w* w, const muz_puct_cfg* cfg, const float* root_logits, const float* root_value,
                    const float* root_embedding, const uint32_t* legal_bits, const float* dirichlet,
                    const float* gumbel, const int32_t* game_id, int32_t n, void* workspace, int64_t workspace_bytes,
                    int32_t* action, float* action_weights, float* root_value_out, void* stream) {
  if (!w || !cfg) return MUZ_E_INVALID;
  if (w->num_actions != MUZ_DET_ACTIONS) return MUZ_E_UNSUPPORTED;
  if (check_puct_cfg(*cfg)) return MUZ_E_UNSUPPORTED;
  const int rc = check_search_call(cfg->num_simulations, cfg->max_depth, n, root_logits, root_value, root_embedding,
                                   legal_bits, workspace, workspace_bytes, search_workspace_bytes, action,
                                   action_weights, root_value_out);
  if (rc || n == 0) return rc;
  return launch_puct_search(*w, make_puct_args(*cfg), root_logits, root_value, root_embedding, legal_bits, dirichlet,
                            gumbel, game_id, n, nullptr, workspace, action, action_weights, root_value_out,
                            (hipStream_t)stream);
}

}  // extern "C"
