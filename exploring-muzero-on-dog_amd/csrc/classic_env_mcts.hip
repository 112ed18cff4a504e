// Network-free MCTS agent for classic (dice) MADN: mctx stochastic_muzero_policy whose model is the environment
// itself, with random-rollout leaf values (MADN/classic_madn.py:543-714 winning_action / policy_function / rollout /
// value_function / recurrent_chance_fn / recurrent_fn / root_fn) as ONE persistent kernel per batched search.
//
// The tree is k_stochastic_search's (stochastic.hip): decision nodes (a state with its die thrown, children = the 4
// pins) alternate with chance nodes (afterstates, children = the 6 die outcomes), A' = 4 + 6 child slots per node
// padded to 16, a chance node's (reward, discount) applied on its chance -> decision edges.  The simulation body is
// tree.hpp's (walk, commit_expansion, commit_backup on a NarrowTree<16>) and so is the muzero_policy frame around it
// (fill_pb_table, root_noise_share, root_prior, puct_score for the decision nodes, final_gumbel, visit_policy), the
// geometry k_env_mcts's (env_mcts.hip): a workgroup owns 16 games for the whole search, 32 lanes per game, lane a holds
// child slot a; root children in registers, node statistics and the path in SearchLds, the children arrays in the
// workspace (CEnvTree, env_model.hpp's carve at 16 slots per node).  A game never leaves its half wave, so the
// simulation loop has no workgroup barrier; wave_sync() is enough for the reason env_model.hpp gives (LDS and vector
// memory operations of one wave complete in order, only the compiler has to be held).
//
// The environment runs in lane 0 of a game's 32 lanes (classic.hpp is written one board per lane and a node has only
// 4 actions to check): the working state is a ClsLane in registers, its board and the rollout's copy of the board are
// LDS rows, a node's state (16 pins, player, die, done, reward; then the chance node's reward and discount) is a
// 64-byte row of the workspace.  The other lanes hold the children and take part in the selection and the backup.
//
// The reference path cannot run (winning_action builds its state without `key`), never changes the discount's sign
// between sides and gives every chance node uniform logits, so parity with it is UNPINNED; the definition is
// tests/_classic_env_mcts.py, which this kernel equals bit for bit (see include/muz.h for the semantics).
//
// Resource targets, checked from the compiler's report (hipcc -Rpass-analysis=kernel-resource-usage): 0 B scratch,
// LDS no larger than k_env_mcts's 43,928 B, and k_env_mcts's occupancy of 4 waves per SIMD (126 VGPRs there).  As
// built: 0 B scratch, 37,808 B LDS, 128 VGPRs, 4 waves per SIMD -- the last under __launch_bounds__(kThreads, 4);
// without the bound the allocator takes 130 VGPRs and the occupancy drops to 3.
#include "classic.hpp"
#include "env_model.hpp"

namespace muz {

namespace {

// (CEnvTree = EnvTreeT<16>: the carve, 10 of a node's 16 child slots used as in stochastic.hip; wave_sync, side_of,
// kMaxRollout, last_pin_wins, rollout_uniform, pick_kth_bit, outcome_for, env_prior_logit: the toolkit at the top of
// env_model.hpp, shared with k_env_mcts and k_env_gumbel)
constexpr int kPins = MUZ_CLASSIC_ACTIONS, kDie = MUZ_CHANCE_OUTCOMES, kCAp = kPins + kDie;
constexpr unsigned long long kClassicRolloutStream = 0xC1A551CD1CEull;   // != env_model.hpp kRolloutStream
// a node's byte in LDS: bits 0-3 the decision node's mask, then its kind and what the expansion hands to the lanes
enum : uint32_t { K_DEC = 16u, K_PASS = 32u, K_SOFT = 64u };

// A node's state row: words 0-3 the 16 pins, word 4 player | die | done | reward
__device__ __forceinline__ void row_store(AS1 uint32_t* r, const ClsLane& s) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t x = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) x |= ((uint32_t)s.pins[w * 4 + k] & 0xFFu) << (8 * k);
    tree_st(r + w, x);
  }
  tree_st(r + 4, ((uint32_t)s.cp & 0xFFu) | (((uint32_t)s.die & 0xFFu) << 8) | (((uint32_t)s.done & 0xFFu) << 16) |
                     (((uint32_t)s.reward & 0xFFu) << 24));
}
__device__ __forceinline__ void row_load(const AS1 uint32_t* r, ClsLane& s) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t x = tree_ld(r + w);
#pragma unroll
    for (int k = 0; k < 4; ++k) s.pins[w * 4 + k] = (int)(int8_t)(x >> (8 * k));
  }
  const uint32_t x = tree_ld(r + 4);
  s.cp = (int)(int8_t)x;
  s.die = (int)(int8_t)(x >> 8);
  s.done = (int)(int8_t)(x >> 16);
  s.reward = (int)(int8_t)(x >> 24);
}

// wins(s): bit k set iff pin k is legal and env_step(s, k) returns reward 1.  Only the move that brings the mover's
// (substituted player's) last pin from the track onto one of its goal cells can complete its goal -- pins in the goal
// are never hit -- so: three pins on goal cells, env_step's landing cell of the fourth (cls_step_masked's new_pos) and
// get_winner on the board with the mover's goal full.  tests/test_classic_env_mcts_host.py compares this formulation
// with the trial steps.
__device__ __forceinline__ uint32_t cls_wins(const DetConsts& c, const ClsLane& s, const BoardView& b,
                                             uint32_t legal) {
  const int cp = sub_player(c, b, s.cp);
  const int g0 = goal_of(c, cp, 0), g3 = goal_of(c, cp, 3);
  int ng = 0, out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pos = cpin(s, cp, k);
    const bool in = pos >= g0 && pos <= g3;
    ng += in ? 1 : 0;
    out = in ? out : k;
  }
  if (ng != 3 || ((legal >> out) & 1u) == 0u) return 0u;
  return last_pin_wins(c, b, cp, cpin(s, cp, out), s.die) ? (1u << out) : 0u;
}

// A random rollout from state s (a copy; its board in `from`), played by one lane on the board copy `bd`: every turn
// throws the die (the first turn of a decision node's rollout keeps the node's die), then no_step without a legal pin,
// else a uniform pick among the winning pins if any, else among the legal ones.  Returns the outcome seen from side
// `view`; `turns` counts the turns played.
__device__ __forceinline__ float cls_rollout(const DetConsts& c, ClsLane s, const int8_t* from, int8_t* bd, int view,
                                             bool keep_die, unsigned long long key, int node_key, int steps,
                                             int& turns) {
#pragma unroll
  for (int w = 0; w < kCells / 4; ++w) reinterpret_cast<uint32_t*>(bd)[w] = reinterpret_cast<const uint32_t*>(from)[w];
  const BoardView b{bd, 1};
#pragma unroll 1
  for (int i = 0; i < steps; ++i) {
    if (s.done) break;
    if (i > 0 || !keep_die) {
      float p[6];
      cls_dice_probs(c, cls_soft_locked(c, s, b), p);
      s.die = cls_choice(p, rollout_uniform(key, node_key, 2 * i));
    }
    const uint32_t lm = cls_legal(c, s, b);
    if (lm == 0u) {
      s.cp = mod_small(s.cp + 1, c.P);
    } else {
      const uint32_t wm = cls_wins(c, s, b, lm);
      cls_step_masked(c, s, b, pick_kth_bit(wm ? wm : lm, rollout_uniform(key, node_key, 2 * i + 1)), lm);
    }
    ++turns;
  }
  return outcome_for(c, b, view);
}

__global__ __launch_bounds__(kThreads, 4) void k_classic_env_mcts(DetConsts c, PuctArgs pa, int rollout_steps,
                                                               muz_classic_soa st,
                                                               const float* __restrict__ dirichlet_in,
                                                               const float* __restrict__ gumbel_in,
                                                               const int32_t* __restrict__ game_id, int n, CEnvTree T,
                                                               int32_t* out_action, float* out_weights,
                                                               float* out_value, int32_t* out_visits, float* out_q) {
  // tree arithmetic exactly as written
#pragma clang fp contract(off)
  __shared__ SearchLds L;
  __shared__ float s_pbtab[kMaxNodes + 1];   // sqrt(N) * pb_c(N) for a node's visit count N = 0..S+1
  __shared__ uint8_t s_kind[kRows][kMaxNodes];   // every node's kind byte
  // the board of the node being expanded and the rollout's copy
  __shared__ __attribute__((aligned(16))) int8_t s_board[kRows][kCells], r_board[kRows][kCells];
  // lane 0's hand-off of an expansion to the game's lanes: the wins mask; value, edge reward and discount
  __shared__ uint32_t s_wins[kRows];
  __shared__ float s_v[kRows], s_er[kRows], s_ed[kRows];

  constexpr int A = kPins;
  const int row = trow(), a = tsub();      // this lane holds child slot `a` of game `row`
  const int g0 = blockIdx.x * kRows;
  const int g = g0 + row;
  const bool valid = g < n;
  const bool ok = a < kCAp;               // a real child slot
  const bool pin_lane = a < A, die_lane = ok && !pin_lane;
  const int ai = pin_lane ? a : 0;        // in-bounds alias for the other lanes
  const BoardView cur{s_board[row], 1};

  fill_pb_table(s_pbtab, pa);
  if (a == 0) {
    s_kind[row][0] = 0;
    s_wins[row] = 0u;
  }
  __syncthreads();

  // ---------------- root (root_fn: prior 100 legal + 200 wins, value a rollout that keeps the root's die; then
  // policies.py stochastic_muzero_policy: _add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions)
  int gid = 0, turns = 0;
  unsigned long long rkey = 0;
  Kid rk = empty_kid(ok, 0.f);   // the root's children, in registers for the whole search (prior: the probability)
  if (valid) {
    gid = game_id ? game_id[g] : g;
    rkey = game_key(pa.seed ^ kClassicRolloutStream, gid, pa.turn);
    if (a == 0) {
      ClsLane s;
      const int S = st.stride;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int v = st.pins[(size_t)min(j, c.P * 4 - 1) * S + g];
        s.pins[j] = (j < c.P * 4) ? v : -1;
      }
      s.cp = st.current_player[g];
      s.done = st.done[g] ? 1 : 0;
      s.reward = st.reward[g];
      s.die = st.die[g];
      cls_rebuild_board(c, s, cur);
      const uint32_t lm = s.done ? 0u : cls_legal(c, s, cur);
      if (lm != 0u) {   // a root that is finished or has no legal pin for its die is not searched
        s_wins[row] = cls_wins(c, s, cur, lm);
        row_store(T.row(g, 0), s);
        const float v = cls_rollout(c, s, s_board[row], r_board[row], side_of(c, s.cp), true, rkey, 0, rollout_steps,
                                    turns);
        s_kind[row][0] = (uint8_t)(lm | K_DEC);
        L.visits[row][0] = 1;
        L.val[row][0] = v;
      }
    }
  }
  wave_sync();
  const uint32_t lm0 = s_kind[row][0] & 15u;
  const bool live = valid && lm0 != 0u;
  {
    const uint32_t wm = s_wins[row];
    const bool inv = !pin_lane || ((lm0 >> a) & 1u) == 0u;
    const float pr = row_softmax24(pin_lane ? env_prior_logit(lm0, wm, ai) : 0.f, pin_lane);
    const float dn =
        root_noise_share(dirichlet_in, (size_t)g * A + ai, valid && pin_lane, pin_lane, pa, gid, pa.turn, a);
    const float p0 = root_prior(pr, dn, pa.dir_frac, inv, pin_lane);
    rk.prior = (live && pin_lane) ? p0 : 0.f;
  }
  wave_sync();

#pragma unroll 1
  for (int sim = 0; sim < pa.S; ++sim) {
    if (live) {
      // ---------------- simulate (search.py simulate): walk from the root
      const WalkEnd w = walk(T, L, rk, pa.D, [&](const Kid& k, int node, int depth) -> float {
        const uint32_t kind = s_kind[row][node];
        // a decision node: muzero_action_selection inside the node's mask
        const bool inv = !pin_lane || ((kind >> a) & 1u) == 0u;
        const float tb = tiebreak_uniform(pa.seed, gid, pa.turn, sim, depth, ai);
        const float ds =
            puct_score<MUZ_QT_PARENT_SIBLINGS>(k, L.val[row][node], L.visits[row][node], s_pbtab, tb, inv, pa);
        // a chance node: argmax p / (n + 1) on the environment's own die probabilities
        const float cs = die_lane ? k.prior / (float)(k.visits + 1) : -INFINITY;
        return (kind & K_DEC) ? ds : cs;
      });
      if (a == 0) L.hand_off(row, w, sim);
    }
    wave_sync();
    if (live && a == 0) {
      // ---------------- expand (search.py expand): both recurrent functions are the environment
      const int par = L.parent[row], act = L.act[row], nx = L.next[row];
      const uint32_t pk = s_kind[row][par];
      ClsLane s;
      row_load(T.row(g, par), s);
      cls_rebuild_board(c, s, cur);
      float v, er, ed;
      uint32_t nk;
      if (pk & K_DEC) {
        // recurrent_fn: decision -> afterstate.  The chance node keeps (reward, discount) for its outgoing edges
        const int mover = side_of(c, s.cp);
        int rw = 0;
        if (pk & K_PASS)
          s.cp = mod_small(s.cp + 1, c.P);
        else
          rw = cls_step_masked(c, s, cur, act, pk & 15u);
        const float dc = s.done ? 0.f : (side_of(c, s.cp) == mover ? 1.f : -1.f);
        AS1 uint32_t* r = T.row(g, nx);
        row_store(r, s);
        tree_st(reinterpret_cast<AS1 float*>(r) + 5, (float)rw);
        tree_st(reinterpret_cast<AS1 float*>(r) + 6, dc);
        nk = cls_soft_locked(c, s, cur) ? K_SOFT : 0u;
        v = s.done ? (float)rw
                   : cls_rollout(c, s, s_board[row], r_board[row], mover, false, rkey, sim + 1, rollout_steps, turns);
        er = 0.f;
        ed = 1.f;
      } else {
        // recurrent_chance_fn: afterstate + die -> state
        const AS1 uint32_t* r = T.row(g, par);
        er = tree_ld(reinterpret_cast<const AS1 float*>(r) + 5);
        ed = tree_ld(reinterpret_cast<const AS1 float*>(r) + 6);
        s.die = act - A + 1;
        const uint32_t lm = s.done ? 0u : cls_legal(c, s, cur);
        s_wins[row] = lm ? cls_wins(c, s, cur, lm) : 0u;
        row_store(T.row(g, nx), s);
        nk = K_DEC | (lm ? lm : (K_PASS | 1u));   // without a legal pin: one action, pin 0, which passes
        v = s.done ? 0.f
                   : cls_rollout(c, s, s_board[row], r_board[row], side_of(c, s.cp), true, rkey, sim + 1, rollout_steps,
                                 turns);
      }
      s_kind[row][nx] = (uint8_t)nk;
      s_v[row] = v;
      s_er[row] = er;
      s_ed[row] = ed;
    }
    wave_sync();
    {
      // the new node's priors: a decision node's softmax of 100 legal + 200 wins inside its mask, a chance node's
      // dice_probabilities
      const uint32_t nk = live ? s_kind[row][L.next[row]] : 0u;
      const uint32_t wm = s_wins[row];
      const bool inv = !pin_lane || ((nk >> a) & 1u) == 0u;
      const float dp = row_softmax24(inv ? kFMin : env_prior_logit(nk, wm, ai), pin_lane);
      float p[6];
      cls_dice_probs(c, (nk & K_SOFT) != 0u, p);
      const float pc = (a == A) ? p[0] : ((a == A + 5) ? p[5] : p[1]);   // die 1, die 6, the equal middle four
      const float prior = (nk & K_DEC) ? (pin_lane ? dp : 0.f) : (die_lane ? pc : 0.f);
      if (live) {
        const float v = s_v[row], er = s_er[row], ed = s_ed[row];
        commit_expansion(T, L, rk, sim, prior, v, er, ed);
        // ---------------- backward (search.py backward) along the recorded path
        commit_backup(T, L, rk, v, er, ed);
      }
    }
    wave_sync();
  }

  // ---------------- tail (_mask_tree(decision), summary().visit_probs, _apply_temperature, categorical as
  // argmax(logits + Gumbel); summary().visit_counts / qvalues)
  if (!valid) return;
  const float gmb = final_gumbel(gumbel_in, (size_t)g * A + ai, pin_lane, pa.seed, gid, pa.turn, ai);
  const PolicyDraw pd = visit_policy(rk.visits, pin_lane, pa.temperature, gmb);
  if (pin_lane) {
    out_weights[(size_t)g * A + a] = live ? pd.weight : 0.f;
    if (out_visits) out_visits[(size_t)g * A + a] = rk.visits;
    if (out_q) out_q[(size_t)g * A + a] = rk.reward + rk.disc * rk.value;
  }
  if (a == 0) {
    out_action[g] = live ? pd.action : -1;
    out_value[g] = live ? fminf(1.f, fmaxf(-1.f, L.val[row][0])) : 0.f;
    T.turns[g] = turns;
  }
}

}  // namespace

}  // namespace muz

using namespace muz;

extern "C" {

int64_t muz_classic_mcts_tree_bytes(int32_t n, const muz_stoch_cfg* cfg) {
  if (!cfg || n < 0 || check_search_limits(cfg->num_simulations, cfg->max_depth)) return -1;
  return (int64_t)CEnvTree::bytes(n, cfg->num_simulations + 1);
}

int muz_classic_mcts(const muz_rules* rules, const muz_stoch_cfg* cfg, const muz_env_mcts_cfg* mcfg,
                     muz_classic_soa state, const float* dirichlet, const float* gumbel, const int32_t* game_id,
                     int32_t n, void* workspace, int64_t workspace_bytes, int32_t* action, float* action_weights,
                     float* root_value, int32_t* visit_counts, float* qvalues, void* stream) {
  if (!rules || !cfg || !mcfg) return MUZ_E_INVALID;
  DetConsts c;
  const int rc = make_det_consts(rules, &c);
  if (rc) return rc;
  if (check_stoch_cfg(*cfg) || check_search_limits(cfg->num_simulations, cfg->max_depth)) return MUZ_E_UNSUPPORTED;
  if (mcfg->rollout_steps < 0 || mcfg->rollout_steps > kMaxRollout) return MUZ_E_UNSUPPORTED;
  MUZ_HOST_CHECK(n >= 0 && state.stride >= n && workspace && action && action_weights && root_value);
  MUZ_HOST_CHECK(state.board && state.pins && state.current_player && state.done && state.reward && state.die);
  MUZ_HOST_CHECK(((uintptr_t)workspace & 15u) == 0 &&
                 workspace_bytes >= (int64_t)CEnvTree::bytes(n, cfg->num_simulations + 1));
  if (n == 0) return MUZ_OK;
  const PuctArgs pa = make_puct_args(*cfg);
  const CEnvTree T = CEnvTree::carve(workspace, n, pa.S + 1);
  const dim3 grid((n + kRows - 1) / kRows);
  k_classic_env_mcts<<<grid, kThreads, 0, (hipStream_t)stream>>>(c, pa, mcfg->rollout_steps, state, dirichlet, gumbel,
                                                                 game_id, n, T, action, action_weights, root_value,
                                                                 visit_counts, qvalues);
  return muz_last_launch_error();
}

}  // extern "C"
