// The det-MADN environment as a search's model, shared by the network-free agents k_env_mcts (env_mcts.hip: PUCT
// muzero_policy) and k_env_gumbel (env_gumbel.hip: gumbel_muzero_policy): the tree's carve with a 64-byte state row
// per node, a game's LDS rows, wins(s), the node mask, the expansion's transition (env_step plus the no-move passes)
// and the random rollout.  One game per kRowLanes lanes, lane a holds action a; everything here is called by all the
// lanes of a game together.  The semantics are fixed in tests/_env_mcts.py (see env_mcts.hip's head).
// At the top, what k_classic_env_mcts (classic_env_mcts.hip) takes too: the carve (EnvTreeT), wave_sync, side_of, the
// rollout cap, the tail of wins(s), the rollout's uniform, pick and outcome, and the prior logit.
#pragma once
#include "detmadn.hpp"
#include "host_consts.hpp"
#include "rng.hpp"
#include "tree.hpp"

namespace muz {
inline namespace MUZ_NN_NS {   // (built on tid(): see the note at the top of nn.hpp)

// ---- the toolkit of every environment-as-model search, det (below) and classic (classic_env_mcts.hip) ---------------

constexpr int kNodeRow = 64;        // bytes of a node's state row in the workspace (det: kStateRow used, classic: 28)
constexpr int kMaxRollout = 1000;   // the entry points' bound on rollout_steps

// The tree's own carve: each game's count of rollout turns [n] (int32, read by the caller after the search), the six
// children arrays of NarrowTree<APAD>, then 64 B per node for its state row.  No latent slots.
struct EnvArrays : TreeArrays {
  int8_t* rows;
  int32_t* turns;
};
template <int APAD>
struct EnvTreeT : NarrowTree<APAD, EnvArrays> {
  using Base = NarrowTree<APAD, EnvArrays>;
  __device__ __forceinline__ AS1 uint32_t* row(int g, int node) const {
    return reinterpret_cast<AS1 uint32_t*>(gpw(this->rows) + ((size_t)g * this->N + node) * kNodeRow);
  }
  static size_t head_bytes(int64_t n) { return ((size_t)n * 4 + 255) & ~(size_t)255; }
  static size_t bytes(int64_t n, int N) {
    return head_bytes(n) + 6 * Base::child_bytes(n, N) + (size_t)n * N * kNodeRow;
  }
  static EnvTreeT carve(void* ws, int n, int N) {
    char* p = (char*)ws;
    EnvTreeT t;
    t.turns = (int32_t*)p;
    p += head_bytes(n);
    const size_t cb = Base::child_bytes(n, N);
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
using EnvTree = EnvTreeT<32>;    // det-MADN: 24 actions per node
using CEnvTree = EnvTreeT<16>;   // classic: 4 pins + 6 die outcomes per node

// A game's lanes hand LDS rows and tree words to each other inside their wave only: LDS and vector memory operations
// of one wave complete in order, so the compiler alone has to be held (no cache action, no wait).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int side_of(const DetConsts& c, int p) { return has(c.flags, R_TEAMS) ? (p & 1) : p; }

// The shared tail of wins(s) (det_wins_g below, cls_wins): does player cp's last pin outside its goal, at cell `cur`
// and moved m cells, land on a goal cell (env_step's new_pos of the det / classic step) and does get_winner, with cp
// done as well, then name cp?
__device__ __forceinline__ bool last_pin_wins(const DetConsts& c, const BoardView& b, int cp, int cur, int m) {
  const uint32_t F = c.flags;
  const int tgt = cst(c.target, cp);
  const int x = cur + m - tgt - (has(F, R_MUST_TRAVERSE) ? 1 : 0);
  const int gx = goal_of(c, cp, jidx(x - 1, 4));
  const bool A = (b.at(gx) != cp) && (has(F, R_JUMP_GOAL) || goal_path_free(c, b, cp, -1, x));
  const bool win = cur != -1 && 4 >= x && x > 0 && A && cur <= tgt;
  // get_winner with player cp done as well
  uint32_t d = 1u << cp;
#pragma unroll
  for (int p = 0; p < 4; ++p) d |= player_done(c, b, p) ? (1u << p) : 0u;
  if (has(F, R_TEAMS)) {
    const bool t0 = (d & 1u) && (d & 4u), t1 = (d & 2u) && (d & 8u);
    d = ((t0 && t1) || !(t0 || t1)) ? 0u : (t0 ? 0x5u : 0xAu);
  }
  return win && ((d >> cp) & 1u);
}

// A rollout's uniform j of node `node_key` (key: the game's), its pick among the candidate actions `cand` (!= 0) --
// the k-th set bit, k = min(floor(u count), count - 1) -- and its outcome on board b seen from `side`
__device__ __forceinline__ float rollout_uniform(unsigned long long key, int node_key, int j) {
  return u24(mix64(key ^ mix64(((unsigned long long)(unsigned)node_key << 16) | (unsigned)j)));
}
__device__ __forceinline__ int pick_kth_bit(uint32_t cand, float u) {
  const int cnt = __popc(cand);
  int k = (int)(u * (float)cnt);
  k = k >= cnt ? cnt - 1 : k;
  uint32_t x = cand;
  for (int j = 0; j < k; ++j) x &= x - 1;   // drop the k lowest set bits
  return __ffs(x) - 1;
}
__device__ __forceinline__ float outcome_for(const DetConsts& c, const BoardView& b, int side) {
  const uint32_t w = winners(c, b);
  bool mine = false;
#pragma unroll
  for (int p = 0; p < 4; ++p) mine |= ((w >> p) & 1u) && side_of(c, p) == side;
  return mine ? 1.f : (w ? -1.f : 0.f);
}

// root_fn / recurrent_fn's prior logit of action ai under a node's legal and winning masks
__device__ __forceinline__ float env_prior_logit(uint32_t legal, uint32_t wins, int ai) {
#pragma clang fp contract(off)
  return 100.f * (float)((legal >> ai) & 1u) + 200.f * (float)((wins >> ai) & 1u);
}

// ---- det-MADN -------------------------------------------------------------------------------------------------------

constexpr int kMaxPasses = 4;       // the turn head's fast-forward cap (selfplay.hip)
constexpr unsigned long long kRolloutStream = 0x7011007D1CEull;
constexpr uint32_t kAllActions = 0xFFFFFFu;

// The LDS rows of one game: its state row and its board
struct GameRows {
  int8_t* st;
  int8_t* bd;
  __device__ __forceinline__ BoardView board() const { return BoardView{bd, 1}; }
  __device__ __forceinline__ LdsLane lane() const { return LdsLane{st, st[40], st[41], st[42]}; }
};

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
  if (win) win = last_pin_wins(c, b, cp, pin_of(s, cp, i), m);
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
        const int act = pick_kth_bit(wm ? wm : lm, rollout_uniform(key, node_key, i));
        det_step_masked(c, s, b, act / 6, act % 6 + 1, lm);
      }
      r.st[40] = (int8_t)s.cp;
      r.st[41] = (int8_t)s.done;
      r.st[42] = (int8_t)s.reward;
    }
    ++turns;
    wave_sync();
  }
  return outcome_for(c, b, side0);
}

// What the expansion of an edge gives (search.py expand's recurrent_fn, the environment): the edge's reward and
// discount, the new node's mask and winning actions, and whether the game is finished there.
struct EnvEdge {
  float reward, disc;
  uint32_t legal, wins;
  bool done;
};

// The transition of edge (par, act) of game g into node nx: the parent's state row from the tree into the game's
// LDS rows `cur`, env_step of `act` under the parent's mask (masks: the game's node masks, read by the stepping lane),
// then no_step while the state is not finished and has no legal action (at most kMaxPasses); the new state stays in
// `cur` and its row goes to the tree.
__device__ __forceinline__ EnvEdge env_expand(const DetConsts& c, const EnvTree& T, const GameRows& cur, int g, int par,
                                              int act, int nx, const uint32_t* masks, int a, int t) {
  if (a < kStateRow / 4) reinterpret_cast<uint32_t*>(cur.st)[a] = tree_ld(T.row(g, par) + a);
  wave_sync();
  rebuild_board_g(c, cur, a);
  const int side_p = side_of(c, cur.st[40]);
  wave_sync();   // every lane has read the mover before the step changes it
  if (a == 0) {
    LdsLane s = cur.lane();
    det_step_masked(c, s, cur.board(), act / 6, act % 6 + 1, masks[par]);
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
  return EnvEdge{rw, dc, lm, wm, fin};
}

}  // namespace MUZ_NN_NS
}  // namespace muz
