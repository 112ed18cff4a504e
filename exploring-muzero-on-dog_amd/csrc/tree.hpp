// The tree machinery the persistent search kernels share: one game per kRowLanes lanes, node scalars and the current
// path in LDS, children arrays and node embeddings in the workspace.  k_gumbel_search and k_puct_search are built from
// one simulation body -- SearchLds (the per-row LDS state), NarrowTree::kid (a node's children), walk (the selection
// loop around the kernel's score), commit_expansion and commit_backup -- and differ in their root, score and tail.
// k_env_mcts (env_mcts.hip) is k_puct_search's body and score (value_score, row_softmax24 below) around an expansion
// that steps the environment instead of the networks, on a carve of its own.  The muzero_policy frame around the body
// -- the pb_c table, the noisy masked root prior, the PUCT score and the visit-count tail (fill_pb_table,
// root_noise_share, root_prior, puct_score, final_gumbel, visit_policy below) -- is one definition for k_puct_search,
// k_env_mcts and k_classic_env_mcts (classic_env_mcts.hip).
// k_env_gumbel (env_gumbel.hip) is that expansion (env_model.hpp) under k_gumbel_search's scores (prior_probs,
// completed_q below).
// k_stochastic_search shares the tree layout and row_argmax and keeps its own walk, expansion and one-lane backup
// written out (on the shared body it was 0.3 % slower per classic self-play step, and needed 247 VGPRs with
// commit_backup: profiles/search_body_refactor.log); k_dog_search (806 children per node, its own walk and backup)
// shares row_argmax and exp_cr.  The limits (kMaxSims, kMaxNodes, kMaxDepth) sit beside SearchArgs in launch.hpp, where
// the host entry points read them too.
#pragma once
#include "launch.hpp"
#include "rng.hpp"
#include "nn.hpp"

namespace muz {
inline namespace MUZ_NN_NS {   // (built on tid(): see the note at the top of nn.hpp)

constexpr float kFMin = -3.4028234663852886e38f;   // jnp.finfo(float32).min

// Dyn4's reward / discount trunk inside Pred4's Dense_1 phase (nn.hpp pred16 LATE_HEADS)
#ifndef MUZ_LATE_HEADS
#define MUZ_LATE_HEADS 0
#endif
constexpr bool kLateHeads = MUZ_LATE_HEADS != 0;
// levels per backup chunk (one per lane; backup_lanes).  A smaller value (make EXTRA=-DMUZ_BACKUP_CHUNK=4) runs the
// chunked path of max_depth > 32 at ordinary depths; no committed test builds that variant
#ifndef MUZ_BACKUP_CHUNK
#define MUZ_BACKUP_CHUNK kRowLanes
#endif
constexpr int kBackupChunk = MUZ_BACKUP_CHUNK;

// (value, index) argmax across the row's lanes under the order "larger value, then smaller index" (jnp.argmax
// tie-break: the first index)
__device__ __forceinline__ void row_argmax(float& v, int& i) {
  auto pick = [](float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  };
  pick(v, i, dpp<DPP_XOR1>(v), dpp<DPP_XOR1>(i));
  pick(v, i, dpp<DPP_XOR2>(v), dpp<DPP_XOR2>(i));
  pick(v, i, dpp<DPP_HALF_MIRROR>(v), dpp<DPP_HALF_MIRROR>(i));
  pick(v, i, dpp<DPP_MIRROR>(v), dpp<DPP_MIRROR>(i));
  {
    const LoHi<float> pv = swap16(v);
    const LoHi<int> pi = swap16(i);
    v = pv.lo;
    i = pi.lo;
    pick(v, i, pv.hi, pi.hi);
  }
  if constexpr (kRowLanes == 64) {
    const LoHi<float> pv = swap32(v);
    const LoHi<int> pi = swap32(i);
    v = pv.lo;
    i = pi.lo;
    pick(v, i, pv.hi, pi.hi);
  }
}

// exp correctly rounded: evaluated in float64 and rounded once, like oracle/mctx_gumbel.py exp_cr (numpy's float32
// exp and the device's expf are each ~1 ulp off in different places)
// (A/B, profiles/r4k_dog_ab.log: a float __expf in its place -- wrong rounding -- was 22-27 % faster per DOG search)
__device__ __forceinline__ float exp_cr(float x) { return (float)exp((double)x); }
// log correctly rounded, the same way (k_puct_search: the root's noisy logits, pb_c, the final temperature logits)
__device__ __forceinline__ float log_cr(float x) { return (float)log((double)x); }

// A sum over the 24 det-MADN actions in numpy's pairwise order for a contiguous row of 24 (see search.hip's note on
// the tree arithmetic), and one child edge of a node (k_gumbel_search, k_puct_search)
enum { DPP_ROW_ROR8 = 0x128 };
__device__ __forceinline__ float row_sum24(float v) {
  static_assert(kRowLanes == 32, "row_sum24: one game per 32 lanes");
  if (tsub() >= 24) v = -0.0f;                  // the additive identity for every x, -0 included
  v = v + dpp<DPP_ROW_ROR8>(v);                 // a_j + a_{j+8} (lanes 16..23: a_{16+j} + -0)
  const LoHi<float> p = swap16(v);
  v = p.lo + p.hi;                              // r_j = (a_j + a_{j+8}) + a_{j+16} in lanes j, j+8, j+16, j+24
  v = v + dpp<DPP_XOR1>(v);                     // r0 + r1 | r2 + r3 | ...
  v = v + dpp<DPP_XOR2>(v);                     // (r0 + r1) + (r2 + r3) | (r4 + r5) + (r6 + r7)
  return v + dpp<DPP_HALF_MIRROR>(v);           // lane i <-> 7 - i: the two halves
}

// One child edge of the current node, held by lane `a` of the game's 32 lanes (ok: a real child slot, a < A).
struct Kid {
  float prior, value, reward, disc;
  int visits, index;
  bool ok;
};

// ---- the tree arithmetic, bit for bit like the NumPy restatement (tests/_mctx_muzero.py) ---------------------------
// As in search.hip: no fma contraction, sums over the 24 actions in row_sum24's order, exp and log correctly rounded
// (exp_cr, log_cr), fp32 sqrt and division as IEEE operations.

// muzero_action_selection's value score of child k: qtransform_by_min_max (the reference's commented call) or
// qtransform_by_parent_and_siblings (mctx's default, eps 1e-8; nv: the node's value)
template <int QT>
__device__ __forceinline__ float value_score(const Kid& k, float nv, const PuctArgs& pa) {
#pragma clang fp contract(off)
  const float q = k.reward + k.disc * k.value;
  const bool vis = k.ok && k.visits > 0;
  if constexpr (QT == MUZ_QT_MIN_MAX) {
    return ((vis ? q : pa.min_value) - pa.min_value) / (pa.max_value - pa.min_value);
  } else {
    const float safe = vis ? q : nv;
    const float lo = fminf(nv, row_min(k.ok ? safe : INFINITY));
    const float hi = fmaxf(nv, row_max(k.ok ? safe : -INFINITY));
    return ((vis ? q : lo) - lo) / fmaxf(hi - lo, 1e-8f);
  }
}

// softmax over the row's A actions (lanes a >= A: 0)
__device__ __forceinline__ float row_softmax24(float x, bool ok) {
#pragma clang fp contract(off)
  const float m = row_max(ok ? x : -INFINITY);
  const float e = ok ? exp_cr(x - m) : 0.f;
  return e / row_sum24(e);
}

// ---- the muzero_policy frame of the PUCT kernels (k_puct_search, k_env_mcts, k_classic_env_mcts): what surrounds the
// simulation body.  ok: the lane holds one of the policy's actions (classic: a pin lane).  The helpers take the noise
// keys (gid, turn) as arguments -- k_puct_search's turn is per game -- and each call site keeps its own control flow
// around them: row_max, row_softmax24, row_isum and row_argmax are collectives over the game's lanes.

// A root child before the first simulation
__device__ __forceinline__ Kid empty_kid(bool ok, float prior) { return Kid{prior, 0.f, 0.f, 0.f, 0, -1, ok}; }

// tab[N] = sqrt(N) * pb_c(N) for every visit count N = 0..kMaxNodes a node can reach, once per search (by the
// workgroup's first threads; the caller's barrier follows)
__device__ __forceinline__ void fill_pb_table(float* tab, const PuctArgs& pa) {
#pragma clang fp contract(off)
  if (tid() <= kMaxNodes) {
    const float N = (float)tid();
    const float pb_c = pa.pb_c_init + log_cr((N + pa.pb_c_base + 1.0f) / pa.pb_c_base);
    tab[tid()] = sqrtf(N) * pb_c;
  }
}

// This lane's share of the root's Dirichlet noise: the caller's array (read by the lanes with `rd`) or, drawn on the
// device, the softmax of the row's log-gammas.  No draw at fraction 0: root_prior multiplies the share by it, and
// 0 * (a softmax term, finite and >= 0) is the +0 that 0 * 0 is.
__device__ __forceinline__ float root_noise_share(const float* dirichlet_in, size_t at, bool rd, bool ok,
                                                  const PuctArgs& pa, int gid, int turn, int a) {
  if (dirichlet_in) return rd ? dirichlet_in[at] : 0.f;
  if (pa.dir_frac == 0.f) return 0.f;
  return row_softmax24(ok ? root_noise_log_gamma(pa.dir_alpha, pa.seed, gid, turn, a) : 0.f, ok);
}

// policies.py _add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions and the tree's softmax: the masked
// root prior probability from the prior probability pr and the noise share dn (inv: the action is not legal)
__device__ __forceinline__ float root_prior(float pr, float dn, float dir_frac, bool inv, bool ok) {
#pragma clang fp contract(off)
  const float noisy = (1.f - dir_frac) * pr + dir_frac * dn;
  float lg = ok ? log_cr(fmaxf(noisy, kTinyF)) : -INFINITY;
  lg = lg - row_max(lg);
  return row_softmax24(inv ? kFMin : lg, ok);
}

// muzero_action_selection's score of child k of a decision node with value nv and nvis visits: value_score +
// policy_score + 1e-7 U (tb: the tie-break uniform), -inf where the lane may not be chosen (inv)
template <int QT>
__device__ __forceinline__ float puct_score(const Kid& k, float nv, int nvis, const float* tab, float tb, bool inv,
                                            const PuctArgs& pa) {
#pragma clang fp contract(off)
  const float vs = value_score<QT>(k, nv, pa);
  const float ps = tab[nvis] * k.prior / (float)(k.visits + 1);
  return inv ? -INFINITY : vs + ps + 1e-7f * tb;
}

// The final draw's Gumbel value of action ai: the caller's array or the counter RNG's policy stream
__device__ __forceinline__ float final_gumbel(const float* gumbel_in, size_t at, bool ok, unsigned long long seed,
                                              int gid, int turn, int ai) {
  return ok ? (gumbel_in ? gumbel_in[at] : gumbel_noise(seed ^ 0xC2B2AE3D27D4EB4Full, gid, turn, ai)) : 0.f;
}

// muzero_policy's tail (summary().visit_probs, _apply_temperature, categorical as argmax(logits + Gumbel)): this
// lane's action weight from its root visits and the row's drawn action
struct PolicyDraw {
  float weight;
  int action;
};
__device__ __forceinline__ PolicyDraw visit_policy(int visits, bool ok, float temperature, float gmb) {
#pragma clang fp contract(off)
  const int vc = ok ? visits : 0;
  const int tot = row_isum(vc);
  const float w = (float)vc / (float)max(tot, 1);
  float lw = ok ? log_cr(w) : -INFINITY;
  lw = (lw - row_max(lw)) / fmaxf(kTinyF, temperature);
  float sc = ok ? lw + gmb : -INFINITY;
  int bi = tsub();
  row_argmax(sc, bi);
  return PolicyDraw{w, bi};
}

// qtransform_completed_by_mix_value's prior_probs of this lane's child, softmax(prior logits) clamped at the smallest
// normal float; pm: the row's largest prior logit.  (k_gumbel_search, k_env_gumbel)
__device__ __forceinline__ float prior_probs(float prior, bool ok, float& pm) {
#pragma clang fp contract(off)
  pm = row_max(ok ? prior : -INFINITY);
  const float e = ok ? exp_cr(prior - pm) : 0.f;
  const float es = row_sum24(e);
  return fmaxf(kTinyF, e / es);
}

// qtransform_completed_by_mix_value (value_scale, maxvisit_init, rescale, mixed value, eps 1e-8); pp: prior_probs of
// the node's children.
__device__ __forceinline__ float completed_q(const Kid& k, float pp, float raw, const SearchArgs& sa, int& sumv) {
#pragma clang fp contract(off)
  const float q = k.reward + k.disc * k.value;
  const bool vis = k.ok && k.visits > 0;
  const int sv = row_isum(k.ok ? k.visits : 0);
  const int mv = row_imax(k.ok ? k.visits : 0);
  const float sp = row_sum24(vis ? pp : 0.f);
  const float wq = row_sum24(vis ? pp * q / sp : 0.f);
  const float mixed = (raw + (float)sv * wq) / (float)(sv + 1);
  float cq = vis ? q : mixed;
  const float lo = row_min(k.ok ? cq : INFINITY);
  const float hi = row_max(k.ok ? cq : -INFINITY);
  const float den = fmaxf(hi - lo, 1e-8f);
  const float scale = (sa.maxvisit_init + (float)mv) * sa.value_scale;
  sumv = sv;
  return scale * ((cq - lo) / den);
}

// seq_halving.get_sequence_of_considered_visits(m, S)[idx] without the table.
__host__ __device__ __forceinline__ int considered_visit(int m, int S, int idx) {
  if (m <= 1) return idx;
  int log2max = 0;
  while ((1 << log2max) < m) ++log2max;
  int k = m, v = 0, len = 0;
  while (len < S) {
    const int extra = max(1, S / (log2max * k));
    for (int e = 0; e < extra; ++e) {
      if (idx < len + k) return v;
      len += k;
      ++v;
    }
    k = max(2, k / 2);
  }
  return v;
}
// The same sequence as a table: entries first, first + step, ... of cv[0..S) (k_gumbel_search: the 32 lanes of a game
// fill its LDS row once per search, lane i the entries i, i + 32, ...; the host entry fills all of it).  S <= kMaxSims,
// so every value fits a byte.
__host__ __device__ __forceinline__ void fill_considered_visits(uint8_t* cv, int m, int S, int first, int step) {
  static_assert(kMaxSims <= 255, "considered-visit table entries are bytes");
  for (int i = first; i < S; i += step) cv[i] = (uint8_t)considered_visit(m, S, i);
}

// A narrow tree's workspace: six children arrays [n][N][APAD] (a node's A <= APAD children padded to APAD), then the
// node embeddings [n][N][256].  Arrays: TreeArrays, or a struct derived from it for a kernel that keeps further
// per-node arrays after these (the kernel argument's layout is the arrays, then N).  The pad slots A..APAD-1 of a node
// are read and written by nothing here; k_gumbel_search keeps a seventh per-child word in those of three of the float
// arrays (search.hip GumbelTree), so the workspace and its cache lines stay what they are.
struct TreeArrays {
  int32_t* c_index;
  float* c_prior;
  float* c_value;
  int32_t* c_visits;
  float* c_reward;
  float* c_disc;
  float* emb;
};
template <int APAD, class Arrays = TreeArrays>
struct NarrowTree : Arrays {
  int N;
  __device__ __forceinline__ size_t ca(int g, int node, int a) const { return ((size_t)g * N + node) * APAD + a; }
  __device__ __forceinline__ AS1 float* e(int g, int node) const {
    return gpw(this->emb) + ((size_t)g * N + node) * LAT;
  }
  // global-address-space views (see common.hpp: keeps LDS waits independent of global loads)
  __device__ __forceinline__ AS1 int32_t* index() const { return gpw(this->c_index); }
  __device__ __forceinline__ AS1 float* prior() const { return gpw(this->c_prior); }
  __device__ __forceinline__ AS1 float* value() const { return gpw(this->c_value); }
  __device__ __forceinline__ AS1 int32_t* visits() const { return gpw(this->c_visits); }
  __device__ __forceinline__ AS1 float* reward() const { return gpw(this->c_reward); }
  __device__ __forceinline__ AS1 float* disc() const { return gpw(this->c_disc); }
  // child a of `node` (lanes past the real slots, !ok: slot 0's words with no visits)
  __device__ __forceinline__ Kid kid(int g, int node, int a, bool ok) const {
    Kid k;
    const size_t e = ca(g, node, ok ? a : 0);
    k.ok = ok;
    k.prior = tree_ld(prior() + e);
    k.value = tree_ld(value() + e);
    k.reward = tree_ld(reward() + e);
    k.disc = tree_ld(disc() + e);
    k.visits = ok ? tree_ld(visits() + e) : 0;
    k.index = tree_ld(index() + e);
    return k;
  }

  static size_t child_bytes(int64_t n, int N) { return (size_t)n * N * APAD * 4; }
  static size_t bytes(int64_t n, int N) { return 6 * child_bytes(n, N) + (size_t)n * N * LAT * 4; }
  static NarrowTree carve(void* ws, int n, int N) {
    char* p = (char*)ws;
    const size_t cb = child_bytes(n, N);
    NarrowTree t;
    t.c_index = (int32_t*)p;
    t.c_prior = (float*)(p + cb);
    t.c_value = (float*)(p + 2 * cb);
    t.c_visits = (int32_t*)(p + 3 * cb);
    t.c_reward = (float*)(p + 4 * cb);
    t.c_disc = (float*)(p + 5 * cb);
    t.emb = (float*)(p + 6 * cb);
    t.N = N;
    return t;
  }
};
// the det-MADN searches' tree (k_gumbel_search, k_puct_search): children arrays padded to 32 actions
using TreeWs = NarrowTree<32>;

// One row's recorded path (an entry per level: node, chosen child, the child's visit-count word, its reward and
// discount) and its node statistics, all in LDS.
struct PathRow {
  const int* node;
  const int* act;
  const int* cvis;
  const float* rew;
  const float* disc;
  int* visits;
  float* val;
};

// search.py backward along the recorded path of depth d, one level per lane: lane a of the row's lanes holds level
// base + a (chunks of CHUNK levels from the top when d > CHUNK).  Path nodes are distinct, so every level's parent
// statistics are read at once; only the discounted leaf value is a chain, evaluated level by level in the original
// order (leaf = r + discount * leaf, bit-identical to a sequential walk) with the level above's value moved down one
// lane per step.  v: the new leaf's value; rw, dc: the reward and discount of the path's last edge (the expansion's).
// The parents' values and visit counts are updated here; edge(l, parent, pact, the level's cvis word, r, dsc,
// child_v) is called once per level for what the kernel keeps per edge (child_v: the new value of the edge's child).
template <int CHUNK, class Edge>
__device__ __forceinline__ void backup_lanes(const PathRow& p, int a, int d, float v, float rw, float dc, Edge edge) {
#pragma clang fp contract(off)
  static_assert(CHUNK >= 1 && CHUNK <= kRowLanes && CHUNK <= 32, "one level per lane (the ballot's 32-lane halves)");
  float carry = v;      // leaf value entering the chunk from the level above it
  float carry_v = v;    // new value of the node below the chunk's top level (its tree edge's value)
  for (int base = ((d - 1) / CHUNK) * CHUNK; base >= 0; base -= CHUNK) {
    const int l = base + a;
    const int top = min(d, base + CHUNK) - 1 - base;   // highest lane of this row's chunk
    const bool on = a <= top;
    int parent = 0, pact = 0, cvis = 0, cnt = 0;
    float r = 0.f, dsc = 0.f, pval = 0.f;
    if (on) {
      parent = p.node[l];
      pact = p.act[l];
      cvis = p.cvis[l];
      r = (l == d - 1) ? rw : p.rew[l];
      dsc = (l == d - 1) ? dc : p.disc[l];
      cnt = p.visits[parent];
      pval = p.val[parent];
    }
    // highest chunk lane over the wave's two rows (wave-uniform loop bound)
    const unsigned long long tb = __ballot(a == top);
    const int k0 = max(tb & 0xFFFFFFFFull ? 31 - __builtin_clz((unsigned)tb) : -1,
                       tb >> 32 ? 31 - __builtin_clz((unsigned)(tb >> 32)) : -1);
    float leaf = 0.f;
    for (int k = k0; k >= 0; --k) {
      const float up = dpp<DPP_WAVE_SHL1>(leaf);   // lane a + 1's value
      if (a == k && on) leaf = r + dsc * (a == top ? carry : up);
    }
    const float pv = (pval * (float)cnt + leaf) / ((float)cnt + 1.0f);
    const float pv_up = dpp<DPP_WAVE_SHL1>(pv);
    const float child_v = (a == top) ? carry_v : pv_up;
    if (on) {
      edge(l, parent, pact, cvis, r, dsc, child_v);
      p.val[parent] = pv;
      p.visits[parent] = cnt + 1;
    }
    carry = __shfl(leaf, 0, kRowLanes);
    carry_v = __shfl(pv, 0, kRowLanes);
  }
}

// Where a walk ended: the node to expand from, the action taken there, the child already at that edge (-1: none yet)
// and the path's depth.
struct WalkEnd {
  int node, act, next, depth;
};

// The per-row LDS state of a search over a narrow tree (one __shared__ object per kernel): node statistics, the
// recorded path and the walk's hand-off to the expand phase.
struct SearchLds {
  int visits[kRows][kMaxNodes];
  float val[kRows][kMaxNodes];
  int p_node[kRows][kMaxDepth];
  int p_act[kRows][kMaxDepth];
  int p_cvis[kRows][kMaxDepth];
  float p_rew[kRows][kMaxDepth];
  float p_disc[kRows][kMaxDepth];
  int act[kRows], parent[kRows], next[kRows], depth[kRows];
  float rootv[kRows];

  __device__ __forceinline__ PathRow path(int row) {
    return PathRow{p_node[row], p_act[row], p_cvis[row], p_rew[row], p_disc[row], visits[row], val[row]};
  }
  // (one lane of the row) the walk's end for the expand phase; a path that ends at a missing child creates node
  // sim + 1
  __device__ __forceinline__ void hand_off(int row, const WalkEnd& w, int sim) {
    parent[row] = w.node;
    act[row] = w.act;
    next[row] = (w.next == -1) ? sim + 1 : w.next;
    depth[row] = w.depth;
  }
};

// search.py simulate for this lane's game: from the root (its children: rk, in registers) take the child with the
// largest score(kid, node, depth) -- this lane's score, -INFINITY for a lane that may not be chosen -- at every level,
// recording the path, until the chosen edge has no child yet or max_depth levels are taken.
template <class Tree, class Score>
__device__ __forceinline__ WalkEnd walk(const Tree& T, SearchLds& L, const Kid& rk, int max_depth, Score score) {
  const int row = trow(), a = tsub();
  const int g = blockIdx.x * kRows + row;
  int node = 0, depth = 0;
  while (true) {
    const Kid k = depth == 0 ? rk : T.kid(g, node, a, rk.ok);
    float sc = score(k, node, depth);
    int bi = a;
    row_argmax(sc, bi);
    const int child = __shfl(k.index, bi, kRowLanes);
    if (a == bi) {
      L.p_node[row][depth] = node;
      L.p_act[row][depth] = bi;
      L.p_rew[row][depth] = k.reward;
      L.p_disc[row][depth] = k.disc;
      L.p_cvis[row][depth] = k.visits;
    }
    ++depth;
    if (child == -1 || depth >= max_depth) return WalkEnd{node, bi, child, depth};
    node = child;
  }
}

// search.py expand's bookkeeping for node L.next[row] (fresh when it is node sim + 1): this lane's child slot gets
// `prior` (a fresh node's other five words are initialised), the edge L.parent[row] -- L.act[row] is linked to the
// node with its reward and discount (a root edge: rk, registers; else the tree) and the node takes value v and one
// more visit.
template <class Tree>
__device__ __forceinline__ void commit_expansion(const Tree& T, SearchLds& L, Kid& rk, int sim, float prior, float v,
                                                 float rw, float dc) {
  const int row = trow(), a = tsub();
  const int g = blockIdx.x * kRows + row;
  const int nx = L.next[row];
  const bool fresh = nx == sim + 1;
  if (rk.ok) {
    const size_t nb = T.ca(g, nx, a);
    tree_st(T.prior() + nb, prior);
    if (fresh) {
      tree_st(T.index() + nb, -1);
      tree_st(T.visits() + nb, 0);
      tree_st(T.value() + nb, 0.f);
      tree_st(T.reward() + nb, 0.f);
      tree_st(T.disc() + nb, 0.f);
    }
  }
  const int par = L.parent[row], pa = L.act[row];
  if (par == 0 && a == pa) {   // a root edge: registers
    rk.index = nx;
    rk.reward = rw;
    rk.disc = dc;
  }
  if (a == 0) {
    if (par != 0) {
      const size_t eb = T.ca(g, par, pa);
      tree_st(T.index() + eb, nx);
      tree_st(T.reward() + eb, rw);
      tree_st(T.disc() + eb, dc);
    }
    L.val[row][nx] = v;
    L.visits[row][nx] = fresh ? 1 : L.visits[row][nx] + 1;
  }
}

// search.py backward along the recorded path (backup_lanes): an interior edge's new value and visit count go to the
// tree, the root edge's (level 0: registers) through L.rootv to the lane that holds it.
template <class Tree>
__device__ __forceinline__ void commit_backup(const Tree& T, SearchLds& L, Kid& rk, float v, float rw, float dc) {
  const int row = trow(), a = tsub();
  const int g = blockIdx.x * kRows + row;
  backup_lanes<kBackupChunk>(L.path(row), a, L.depth[row], v, rw, dc,
                             [&](int l, int parent, int pact, int cvis, float, float, float child_v) {
                               if (l > 0) {
                                 const size_t ei = T.ca(g, parent, pact);
                                 tree_st(T.value() + ei, child_v);
                                 tree_st(T.visits() + ei, cvis + 1);
                               } else {
                                 L.rootv[row] = child_v;
                               }
                             });
  // the root edge of this path (level 0): its lane takes the value lane 0 just backed up
  // (same wave: LDS operations of one wave complete in order)
  __builtin_amdgcn_wave_barrier();
  if (a == L.p_act[row][0]) {
    rk.value = L.rootv[row];
    rk.visits += 1;
  }
}

}  // namespace MUZ_NN_NS
}  // namespace muz
