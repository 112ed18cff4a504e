// Batched Gumbel MuZero search (mctx 0.0.6 gumbel_muzero_policy, as called by
// MuZero_det_MADN/muzero_deterministic_madn.py:663-704) as ONE persistent kernel per search.
//
// A workgroup owns 16 games for the whole search: for every simulation it walks the 16 trees
// (32 lanes per game, one action per lane, wavefront shuffles for every reduction), gathers the
// 16 parent embeddings into LDS, runs DynamicsNetwork4 + PredictionNetwork4 on MFMA over the
// 16-row tile, expands, and backs up.  No kernel boundary between simulations and no
// inter-workgroup traffic (games are independent).  Node scalars (visits, raw value, value) and
// the current path live in LDS; children arrays and node embeddings live in the workspace (HBM,
// L2/MALL resident), written lazily when a node is created.
#include "rng.hpp"
#include "tree.hpp"

namespace muz {

// Diagnostic build only (make DIAG=1): per-phase shader-clock totals of the search kernel.
#ifdef MUZ_STAMPS
__device__ unsigned long long g_muz_stamps[8];
#define MUZ_STAMP(i)                                                          \
  do {                                                                        \
    if (threadIdx.x == 0) {                                                   \
      const unsigned long long _t = __builtin_amdgcn_s_memtime();             \
      st_acc[i] += _t - st_last;                                              \
      st_last = _t;                                                           \
    }                                                                         \
  } while (0)
#else
#define MUZ_STAMP(i) \
  do {               \
  } while (0)
#endif

// Two of the ~31 workgroup barriers per simulation are not needed for correctness (see the uses); removing
// them measured within noise on MI355X (B=4096 S=50: +-1 %), so they stay.  A static s_setprio 1 for
// waves 4-7 also measured within noise (profiles/r1e_prio_ab.log).

// (kLateHeads, kBackupChunk and the det-MADN tree TreeWs: tree.hpp)

// ---- the tree arithmetic, bit for bit like the NumPy restatement (oracle/mctx_gumbel.py) -------------------
// With identical network outputs on both sides the search's floats then agree exactly (tests/_parity.py):
//  * no fma contraction (q = r + d * v, the mixed value and the backup round twice, like numpy);
//  * a sum over the 24 actions in numpy's pairwise order for a contiguous row of 24: r_j = (a_j + a_{j+8}) +
//    a_{j+16} for j < 8, then ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
//  * exp correctly rounded: evaluated in float64 and rounded once (numpy's float32 exp and the device's expf
//    are each ~1 ulp off in different places; the oracle rounds the float64 exp the same way).
// (row_sum24 and Kid: tree.hpp, shared with k_puct_search)

// The select phase's invariants (kernel template argument PARTS).  What a walk level computes from a node's priors
// alone -- prior_probs below: one float64 exp, two row reductions, one division -- never changes once the node is
// expanded, and the root's considered-visit count is a function of (the game's number of considered actions, S, the
// simulation's index).  Each can be evaluated once instead of at every level:
//  kSelRoot   the root's prior_probs and largest prior before the simulation loop, kept in registers;
//  kSelTable  the considered-visit sequence before the loop, a byte table per game in LDS;
//  kSelNode   a node's prior_probs at its expansion, kept beside its priors (GumbelTree) and loaded with the node's
//             other words.
// The expressions are the same functions in every form, so the results are bit for bit the same
// (tests/test_gpu_select_invariants.py).  MUZ_SELECT_INVARIANTS, read per launch, chooses: unset or 1 -- kSelDefault,
// the root's two; 0 -- none (the form before these, for A/B runs); 2 -- all three.  kSelNode is off by default: in the
// stamp build it left the select phase as long as it was and cost 0.8 k cycles per simulation at the expansion
// (profiles/select_invariants_ab.log).
// make EXTRA=-DMUZ_SELECT_PARTS=m builds the default form with other parts (a stamp run of one part alone); no
// committed test builds that variant.
enum { kSelNode = 1, kSelRoot = 2, kSelTable = 4, kSelAll = 7 };
#ifndef MUZ_SELECT_PARTS
#define MUZ_SELECT_PARTS (kSelRoot | kSelTable)
#endif
constexpr int kSelDefault = MUZ_SELECT_PARTS;

// The det-MADN tree with prior_probs per child.  Lane a's word lies in the node's pad slots (24..31 of 32) of c_prior
// (a < 8), c_reward (a < 16) or c_disc: slots nothing else touches, in cache lines the walk loads anyway.
struct GumbelTree : TreeWs {
  static_assert(3 * (32 - MUZ_DET_ACTIONS) >= MUZ_DET_ACTIONS, "24 words in the pad slots of three arrays");
  __device__ __forceinline__ AS1 float* pp(int g, int node, int a) const {
    AS1 float* const base = a < 8 ? prior() : a < 16 ? reward() : disc();
    return base + ca(g, node, MUZ_DET_ACTIONS + (a & 7));
  }
};

// (prior_probs and completed_q, qtransform_completed_by_mix_value's two halves: tree.hpp, shared with k_env_gumbel)

// SB: the dense layers' weight addressing (nn.hpp; MUZ_RING_ADDR, read per launch, for the default form of PARTS)
template <int PARTS, bool SB = true>
__global__ __launch_bounds__(kThreads, 1) void k_gumbel_search(
    muz_net_w Wt, SearchArgs sa, const float* __restrict__ root_logits, const float* __restrict__ root_value,
    const float* __restrict__ root_emb, const uint32_t* __restrict__ legal, const float* __restrict__ gumbel_in,
    const int32_t* __restrict__ game_id, int n, const int* __restrict__ n_dev, GumbelTree T, int32_t* out_action,
    float* out_weights, float* out_value) {
  // tree arithmetic exactly as written (see row_sum24); the networks (nn.hpp) keep their own contraction
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float smem[kArenaFloats];
  __shared__ SearchLds L;
  __shared__ float s_raw[kRows][kMaxNodes];
  __shared__ uint8_t s_cv[kRows][kMaxSims];   // (CV_TAB) the game's sequence of considered visits
  constexpr bool NODE_PP = PARTS & kSelNode, ROOT_PP = PARTS & kSelRoot, CV_TAB = PARTS & kSelTable;

  if (n_dev) n = *n_dev;
  if ((int)blockIdx.x * kRows >= n) return;
  const Arena ar = Arena::carve(smem);
  const int A = Wt.num_actions;
  const int row = trow(), a = tsub();      // this lane holds action `a` of game `row`
  const int g = blockIdx.x * kRows + row;
  const bool valid = g < n;
  const bool ok = a < A;
  const int ai = ok ? a : 0;              // in-bounds alias for lanes a >= A
#ifdef MUZ_STAMPS
  unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif

  // ---------------- root: instantiate_tree_from_root with masked logits (policies.py _mask_invalid_actions)
  unsigned lb = 0;
  int ncons = 0;
  float gum = 0.f;
  // The root's children live in registers (lane a holds child a) for the whole search: the root is
  // visited by every simulation, so its edge data never goes through HBM.
  Kid rk;
  rk.ok = ok;
  rk.prior = kFMin;
  rk.value = 0.f;
  rk.reward = 0.f;
  rk.disc = 0.f;
  rk.visits = 0;
  rk.index = -1;
  float rpp = 0.f, rpm = 0.f;   // (ROOT_PP) prior_probs of the root's children and its largest prior
  if (valid) {
    lb = legal[g];
    const int lane = game_id ? game_id[g] : g;
    const int gid = sa.key_game ? sa.key_game[lane] : lane;
    const int gturn = sa.key_turn ? sa.key_turn[gid] : sa.turn;
    const float l = ok ? root_logits[(size_t)g * A + ai] : -INFINITY;
    const float lm = row_max(l);
    const bool inv = !ok || ((lb >> a) & 1u) == 0u;
    rk.prior = inv ? kFMin : l - lm;
    if (ok) gum = gumbel_in ? gumbel_in[(size_t)g * A + ai] : sa.gumbel_scale * gumbel_noise(sa.seed, gid, gturn, ai);
    AS1 float* e0 = T.e(g, 0);
    for (int c = a; c < LAT; c += kRowLanes) e0[c] = root_emb[(size_t)g * LAT + c];
    ncons = min(sa.max_considered, __popc(lb & ((1u << A) - 1u)));
    if constexpr (ROOT_PP) rpp = prior_probs(rk.prior, ok, rpm);
    // (read by this row's lanes only, one wave)
    if constexpr (CV_TAB) fill_considered_visits(s_cv[row], ncons, sa.S, a, kRowLanes);
    if (a == 0) {
      const float v = root_value[g];
      L.visits[row][0] = 1;
      s_raw[row][0] = v;
      L.val[row][0] = v;
    }
  }
  __syncthreads();

  // CV_TAB: a zero the optimiser cannot see through, for the m of the walk's considered_visit call.  That call's loop
  // nest is never entered then, but it has to stay in the walk: how the compiler lays out the rest of this kernel
  // depends on it.  With a plain table read in its place 166 hunks of the networks' MFMA loops come out differently
  // (pointer arithmetic as add / add-with-carry pairs between the MFMAs) and a launch is 0.5-0.8 % slower than with no
  // table at all; with the call kept the MFMA loops are instruction for instruction those of the form without the
  // table and a launch is 1.3-1.9 % faster (B = 4096, S = 50: profiles/select_invariants_ab.log;
  // profiles/mfma_loop_diff.py counts the hunks).
  int cv_m0 = 0;
  if constexpr (CV_TAB) asm volatile("" : "+v"(cv_m0));
  st_begin();
  PfT<SB> pf;   // first k-blocks of the next dense layer (crosses the select / expand phases)
  pf_issue<NT256>(pf, &kernarg0<muz_net_w>()->dyn.d3, LAT, LAT);
#pragma unroll 1
  for (int sim = 0; sim < sa.S; ++sim) {
    MUZ_STAMP(0);
    st_sim(sim);
    // Weight table = kernel argument 0, read through the kernarg segment and laundered once per
    // simulation so the compiler re-derives the layer addresses inside the loop.
    const AS4 muz_net_w* wl = kernarg0<muz_net_w>();
    DynIn din;
    int dact = 0;
    // ---------------- simulate (search.py simulate): walk from the root
    if (valid) {
      const WalkEnd w = walk(T, L, rk, sa.D, [&](const Kid& k, int node, int depth) -> float {
        int sumv;
        float pmax = rpm, pp = rpp;
        if (depth == 0 ? !ROOT_PP : !NODE_PP) {
          pp = prior_probs(k.prior, k.ok, pmax);
        } else if (depth != 0) {
          pp = tree_ld(T.pp(g, node, ai));   // (beside the node's other six words: no dependent round trip)
        }
        const float cq = completed_q(k, pp, s_raw[row][node], sa, sumv);
        if (depth == 0) {
          // gumbel_muzero_root_action_selection: score_considered + masked_argmax (sumv: this simulation's index)
          // CV_TAB: the table's entry, passed through considered_visit (m = 0 returns the index at its first line)
          const int cv = considered_visit(CV_TAB ? cv_m0 : ncons, sa.S, CV_TAB ? (int)s_cv[row][sumv] : sumv);
          const float s = fmaxf(-1e9f, gum + (k.prior - pmax) + cq) + (k.visits == cv ? 0.f : -INFINITY);
          return (!ok || ((lb >> a) & 1u) == 0u) ? -INFINITY : s;
        }
        // gumbel_muzero_interior_action_selection: softmax(prior + cq) - N / (1 + sum N)
        const float z = k.prior + cq;
        const float zm = row_max(ok ? z : -INFINITY);
        const float ez = ok ? exp_cr(z - zm) : 0.f;
        const float zs = row_sum24(ez);
        return ok ? (ez / zs - (float)k.visits / (float)(1 + sumv)) : -INFINITY;
      });
      // expand's inputs (parent embedding, FiLM rows of the action): issued by the game's own lanes now,
      // they land while the other games finish their walks
      din = dyn_load(wl->dyn, A, T.e(g, w.node), w.act);
      dact = w.act;
      if (a == 0) L.hand_off(row, w, sim);
    } else {
      din = dyn_load(wl->dyn, A, nullptr, 0);
      if (a == 0) L.act[row] = 0;
    }
    ST(ST_SEL);
    // (Dyn4's first pass -- LayerNorm_0 + FiLM of the parent latent -- only reads this row's own registers
    // and writes this row of the arena: this barrier is not needed for correctness, see above)
    SYNC();
    MUZ_STAMP(1);   // select
    // ---------------- expand (search.py expand): recurrent_fn on the 16 parents
    // the new node's embedding goes to the tree and Pred4's LayerNorm_0 into ar.X straight from Dyn4's
    // min-max pass (registers), so Pred4 starts with its first ResBlock
    const int nx = L.next[row];
    dyn16<NT256, true, kLateHeads>(wl->dyn, A, din, dact, ar, pf, &wl->pred.rb[0].d0, LAT, LAT, &wl->pred.ln0,
                                   valid ? T.e(g, nx) : nullptr);
    MUZ_STAMP(3);   // dynamics
    MUZ_STAMP(4);   // embedding write (fused)
    pred16<NT256, true, kLateHeads, kSplitkLogits>(wl->pred, A, ar.T, ar, pf, &wl->dyn.d3, LAT, LAT, &wl->dyn, dact);
    MUZ_STAMP(5);   // prediction
    if (valid) {
      // the new node keeps its prior logits
      const float v = ar.v0[row], rw = ar.v1[row], dc = ar.v2[row];
      const float prior = ar.U[row * LD + ai];
      commit_expansion(T, L, rk, sim, prior, v, rw, dc);
      if constexpr (NODE_PP) {   // ... and their prior_probs, for every later walk through it
        float pm;
        const float pp = prior_probs(prior, ok, pm);
        if (ok) tree_st(T.pp(g, nx, a), pp);
      }
      if (a == 0) s_raw[row][nx] = v;
      // ---------------- backward (search.py backward) along the recorded path
      commit_backup(T, L, rk, v, rw, dc);
    }
    ST(ST_TREE);
    // (The next walk of row r reads only what row r's own lanes -- one wave -- wrote here: this barrier is
    // not needed for correctness either)
    SYNC();
    MUZ_STAMP(6);   // expand + backward
  }
#ifdef MUZ_STAMPS
  if (threadIdx.x == 0)
    for (int i = 0; i < 8; ++i) atomicAdd(&g_muz_stamps[i], st_acc[i]);
#endif
  st_end();

  // ---------------- final action + action_weights (policies.py gumbel_muzero_policy tail)
  if (valid) {
    const Kid& k = rk;
    int sumv;
    float pmax = rpm, pp = rpp;
    if constexpr (!ROOT_PP) pp = prior_probs(k.prior, k.ok, pmax);
    const float cq = completed_q(k, pp, s_raw[row][0], sa, sumv);
    const bool inv = !ok || ((lb >> a) & 1u) == 0u;
    const int cv = row_imax(k.visits);   // considered_visit = max(visit_counts)
    float sc = fmaxf(-1e9f, gum + (k.prior - pmax) + cq) + (k.visits == cv ? 0.f : -INFINITY);
    sc = inv ? -INFINITY : sc;
    int bi = a;
    row_argmax(sc, bi);
    // action_weights = softmax(_mask_invalid_actions(prior + completed_q))
    const float z = k.prior + cq;
    const float zm = row_max(ok ? z : -INFINITY);
    const float zz = inv ? kFMin : z - zm;
    const float mm = row_max(ok ? zz : -INFINITY);
    const float ez = ok ? exp_cr(zz - mm) : 0.f;
    const float zs = row_sum24(ez);
    if (ok) out_weights[(size_t)g * A + a] = ez / zs;
    if (a == 0) {
      out_action[g] = bi;
      out_value[g] = L.val[row][0];
    }
  }
}

int64_t search_workspace_bytes(int n, int S) { return (int64_t)TreeWs::bytes(n, S + 1); }

// MUZ_SELECT_INVARIANTS (read per launch): which of the select phase's invariants are evaluated once (see kSelDefault)
static int select_form() {
  const char* e = getenv("MUZ_SELECT_INVARIANTS");
  return e ? atoi(e) : 1;
}

int launch_gumbel_search(const muz_net_w& w, const SearchArgs& sa, const float* root_logits, const float* root_value,
                         const float* root_emb, const uint32_t* legal, const float* gumbel, const int32_t* game_id,
                         int n, const int* n_dev, void* workspace, int32_t* action, float* weights, float* value,
                         hipStream_t s) {
  const GumbelTree T{TreeWs::carve(workspace, n, sa.S + 1)};
  const dim3 grid((n + kRows - 1) / kRows);
  switch (select_form()) {
    case 0:
      k_gumbel_search<0><<<grid, kThreads, 0, s>>>(w, sa, root_logits, root_value, root_emb, legal, gumbel, game_id, n,
                                                   n_dev, T, action, weights, value);
      break;
    case 2:
      k_gumbel_search<kSelAll><<<grid, kThreads, 0, s>>>(w, sa, root_logits, root_value, root_emb, legal, gumbel,
                                                         game_id, n, n_dev, T, action, weights, value);
      break;
    default:
      if (ring_scalar_base())
        k_gumbel_search<kSelDefault, true><<<grid, kThreads, 0, s>>>(w, sa, root_logits, root_value, root_emb, legal,
                                                                     gumbel, game_id, n, n_dev, T, action, weights,
                                                                     value);
      else
        k_gumbel_search<kSelDefault, false><<<grid, kThreads, 0, s>>>(w, sa, root_logits, root_value, root_emb, legal,
                                                                      gumbel, game_id, n, n_dev, T, action, weights,
                                                                      value);
  }
  return muz_last_launch_error();
}

}  // namespace muz

using namespace muz;

extern "C" {

int64_t muz_search_workspace_bytes(int32_t n, const muz_search_cfg* cfg) {
  if (!cfg || n < 0) return -1;
  return search_workspace_bytes(n, cfg->num_simulations);
}

int muz_gumbel_search(const muz_net_w* w, const muz_search_cfg* cfg, const float* root_logits, const float* root_value,
                      const float* root_embedding, const uint32_t* legal_bits, const float* gumbel,
                      const int32_t* game_id, int32_t n, void* workspace, int64_t workspace_bytes, int32_t* action,
                      float* action_weights, float* root_value_out, void* stream) {
  if (!w || !cfg) return MUZ_E_INVALID;
  if (w->num_actions != MUZ_DET_ACTIONS) return MUZ_E_UNSUPPORTED;
  if (cfg->max_num_considered < 1) return MUZ_E_UNSUPPORTED;
  const int rc = check_search_call(cfg->num_simulations, cfg->max_depth, n, root_logits, root_value, root_embedding,
                                   legal_bits, workspace, workspace_bytes, search_workspace_bytes, action,
                                   action_weights, root_value_out);
  if (rc || n == 0) return rc;
  return launch_gumbel_search(*w, make_search_args(*cfg), root_logits, root_value, root_embedding, legal_bits, gumbel, game_id, n, nullptr,
                              workspace, action, action_weights, root_value_out, (hipStream_t)stream);
}

int muz_considered_visits(int32_t num_considered, int32_t num_simulations, uint8_t* out) {
  if (!out || num_considered < 0) return MUZ_E_INVALID;
  if (num_simulations < 1 || num_simulations > kMaxSims) return MUZ_E_UNSUPPORTED;
  fill_considered_visits(out, num_considered, num_simulations, 0, 1);
  return MUZ_OK;
}

#ifdef MUZ_STAMPS2
int muz_diag_stamps2(unsigned long long* host_out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_st2), sizeof(unsigned long long) * ST_N);
  if (e != hipSuccess) return (int)e;
  if (reset) {
    unsigned long long z[ST_N] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_st2), z, sizeof(z));
  }
  return (int)e;
}
#endif

#ifdef MUZ_TIMELINE
// out: kWaves x kTlMax records then kWaves counts (reset: zero the counts after the copy)
int muz_diag_timeline(unsigned long long* host_out, unsigned int* host_n, int reset) {
  hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tl), sizeof(unsigned long long) * kWaves * kTlMax);
  if (e == hipSuccess) e = hipMemcpyFromSymbol(host_n, HIP_SYMBOL(g_tl_n), sizeof(unsigned int) * kWaves);
  if (e == hipSuccess && reset) {
    unsigned int z[kWaves] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_tl_n), z, sizeof(z));
  }
  return (int)e;
}
#endif

#ifdef MUZ_STAMPS
int muz_diag_stamps(unsigned long long* host_out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_muz_stamps), sizeof(unsigned long long) * 8);
  if (e != hipSuccess) return (int)e;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_muz_stamps), z, sizeof(z));
  }
  return (int)e;
}
#endif

}  // extern "C"
