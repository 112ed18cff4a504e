// The native self-play driver: one turn loop (sp_turns) and one entry-point body (sp_play) over a small *game* object
// -- det MADN with the Gumbel or the PUCT search (selfplay.hip), classic MADN with the stochastic search
// (selfplay_classic.hip) -- with the workspace carve, the argument checks, the trajectory clear and the lane reset /
// init kernels they need.  The loop owns the TurnLedger, the turn counters, the error discipline after every launch
// group and the order of a turn.  A game supplies its types (Net, Cfg, Soa, Records), the static check / args_ok /
// carve / clear / reset_lane, and per call:
//   head(turn, led)    every launch up to the compacted observations of the games that search; returns TurnCounts
//   root(tc)           its launch_root_inference overload
//   search(counts, t)  its search launcher (GumbelTurn, PuctTurn, StochasticTurn)
//   after_search(t)    what follows the search within the turn (classic: the apply; det: marks it pending)
//   finish()           what is left after the last turn (det: the pending apply)
#pragma once
#include <algorithm>

#include "detmadn.hpp"
#include "launch.hpp"
#include "turn_ledger.hpp"

namespace muz {

// One call's workspace: the search tree, then the per-game / per-slot arrays of a turn, each 256-byte aligned.
struct SpWs {
  void* tree;
  float* conv;
  float* obs;
  uint32_t* legal;
  uint32_t* legal_c;
  int32_t* flag;
  int32_t* slot;
  int32_t* list;
  float* root_logits;
  float* root_value;
  float* root_emb;
  int32_t* action;
  float* weights;
  float* value;
  int32_t* counts;
  int32_t* lane_game;   // streaming driver: game number per lane
  int32_t* next_game;
};

// Carves n games' workspace (C observation channels, A actions, tree_bytes of search tree) out of base and returns
// its size; base null: the size only.
static inline size_t sp_carve(char* base, int n, int C, int A, size_t tree_bytes, SpWs* w) {
  const size_t n16 = (size_t)((n + 15) / 16 * 16);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  SpWs t;
  t.tree = take(tree_bytes);
  t.conv = (float*)take(n16 * kConvRowFloats * 4);
  t.obs = (float*)take(n16 * C * kCells * 4);
  t.legal = (uint32_t*)take((size_t)n * 4);
  t.legal_c = (uint32_t*)take((size_t)n * 4);
  t.flag = (int32_t*)take((size_t)n * 4);
  t.slot = (int32_t*)take((size_t)n * 4);
  t.list = (int32_t*)take((size_t)n * 4);
  t.root_logits = (float*)take(n16 * A * 4);
  t.root_value = (float*)take(n16 * 4);
  t.root_emb = (float*)take(n16 * 256 * 4);
  t.action = (int32_t*)take(n16 * 4);
  t.weights = (float*)take(n16 * A * 4);
  t.value = (float*)take(n16 * 4);
  t.counts = (int32_t*)take(64);
  t.lane_game = (int32_t*)take((size_t)n * 4);
  t.next_game = (int32_t*)take(64);
  if (w) *w = t;
  return off;
}

// The drivers' argument check: `lanes` games at a time (state rows of stride >= lanes) out of num_games (a batch:
// num_games = lanes), a workspace, every trajectory array; align16: a driver that writes the observation records and
// its workspace in 16-byte chunks
static inline bool sp_args_ok(int lanes, int num_games, int stride, const void* workspace, const muz_traj& tr,
                              bool align16) {
  return lanes >= 0 && num_games >= 0 && stride >= lanes && workspace && tr.max_steps > 0 && tr.obs && tr.act &&
         tr.rew && tr.val && tr.pol && tr.mask && tr.player && tr.team && tr.discount && tr.idx &&
         (!align16 || ((((uintptr_t)tr.obs | (uintptr_t)workspace) & 15u) == 0));
}

// Zeroed records of `games` games (init_buffers, game_agent.py:158-169): C observation channels, A actions
static inline int traj_clear(const muz_traj& tr, int games, int C, int A, hipStream_t s) {
  const size_t nt = (size_t)games * tr.max_steps;
  MUZ_HIP_RET(hipMemsetAsync(tr.obs, 0, nt * C * kCells, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.act, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.rew, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.val, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.pol, 0, nt * A * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.mask, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.player, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.team, 0xFF, nt * 4, s));   // jnp.full(..., -1)
  MUZ_HIP_RET(hipMemsetAsync(tr.discount, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(tr.idx, 0, (size_t)games * 4, s));
  return MUZ_OK;
}
// ... and the classic driver's die records beside them
static inline int traj_clear(const muz_traj_chance& ch, int games, int T, hipStream_t s) {
  const size_t nt = (size_t)games * T;
  MUZ_HIP_RET(hipMemsetAsync(ch.dice, 0, nt * 4, s));
  MUZ_HIP_RET(hipMemsetAsync(ch.dice_dist, 0, nt * 6 * 4, s));
  return MUZ_OK;
}

// The streaming driver: at most ceil(num_games / lanes) generations of T turns each
static inline int stream_max_turns(int num_games, int lanes, int T) {
  const long long gens = ((long long)num_games + lanes - 1) / lanes;
  return (int)std::min<long long>(gens * T + 1, 1 << 30);
}

// A fresh game in lane g, as far as det and classic MADN agree (a game's reset_lane adds its own rows)
template <class Soa>
__device__ __forceinline__ void madn_reset_lane(const DetConsts& c, const Soa& st, int g) {
  const int S = st.stride;
  const bool fp = has(c.flags, R_FREE_PIN);
  for (int cell = 0; cell < kCells; ++cell) st.board[cell * S + g] = -1;
  for (int p = 0; p < c.P; ++p) {
    for (int k = 0; k < 4; ++k) st.pins[(p * 4 + k) * S + g] = (int8_t)((fp && k == 0) ? c.start[p] : -1);
    if (fp) st.board[c.start[p] * S + g] = (int8_t)p;
  }
  st.current_player[g] = (int8_t)c.starting_player;
  st.reward[g] = 0;
  st.done[g] = 0;
}

template <class Game>
__global__ void k_sp_reset(DetConsts c, typename Game::Soa st, int n) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Game::reset_lane(c, st, g);
}

template <class Game>
__global__ void k_sp_init(DetConsts c, typename Game::Soa st, int32_t* lane_game, int32_t* next, int num_games, int W) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l == 0) next[0] = min(num_games, W);
  if (l >= W) return;
  lane_game[l] = l < num_games ? l : -1;
  Game::reset_lane(c, st, l);
}

// Where a turn's counts (searching, active) are on the device; host_slot: the ledger's pinned slot when root inference
// is to write them there itself (else the head has queued led.counts)
struct TurnCounts {
  const int32_t* dev;
  int32_t* host_slot;
};

// The turn loop of the batch and the streaming driver.  Batch: lane g plays game g for at most T turns.  Streaming:
// lanes are refilled with the next game number when theirs ends, until num_games games have been played.
template <class Game>
static int sp_turns(Game& game, int max_turns, muz_sp_stats* stats, hipStream_t s) {
  TurnLedger led(s, stats != nullptr);
  int rc = led.begin();
  if (rc) return rc;
  int turns = 0;
  for (int turn = 0; turn < max_turns; ++turn) {
    if (!led.proceed(turn)) break;
    const TurnCounts tc = game.head(turn, led);
    if ((rc = muz_last_launch_error())) break;
    if ((rc = game.root(tc))) break;
    if (tc.host_slot) led.counts_written(turn);
    led.search_begin(turn);
    if ((rc = game.search(tc.dev, turn))) break;
    led.search_end(turn);
    game.after_search(turn);
    if ((rc = muz_last_launch_error())) break;
    ++turns;
  }
  if (rc == MUZ_OK) rc = game.finish();
  led.finish(turns, stats);
  return rc;
}

// The checks of every entry point (`lanes` games at a time out of num_games), in this order: the rules, the game's
// network and search settings (Game::check), the arguments, the search limits, the workspace size; then the carve
template <class Game>
static int sp_setup(const muz_rules* rules, const typename Game::Net* w, const typename Game::Cfg* cfg,
                    const typename Game::Soa& st, const typename Game::Records& rec, int lanes, int num_games,
                    void* workspace, int64_t workspace_bytes, muz_sp_stats* stats, DetConsts* c, SpWs* ws) {
  int rc = make_det_consts(rules, c);
  if (rc) return rc;
  if ((rc = Game::check(w, cfg, c->P))) return rc;
  MUZ_HOST_CHECK(Game::args_ok(lanes, num_games, st.stride, workspace, rec));
  if ((rc = check_search_limits(cfg->num_simulations, cfg->max_depth))) return rc;
  if (stats) *stats = muz_sp_stats{};
  const int C = w->obs_channels, S = cfg->num_simulations;
  MUZ_HOST_CHECK(workspace_bytes >= (int64_t)Game::carve(nullptr, lanes, C, S, nullptr));
  Game::carve((char*)workspace, lanes, C, S, ws);
  return MUZ_OK;
}

// Every entry point: the checks, zeroed records, fresh games, then the turn loop.  A batch (play_n_games_v3,
// num_games == lanes): lane g plays game g.  Streaming: num_games games through `lanes` lanes, lane l starts game l and
// later games are handed out by the turn head's refill.
template <class Game>
static int sp_play(const muz_rules* rules, const typename Game::Net* w, const typename Game::Cfg* cfg,
                   typename Game::Soa st, typename Game::Records rec, int num_games, int lanes, bool stream,
                   void* workspace, int64_t workspace_bytes, muz_sp_stats* stats, hipStream_t s) {
  DetConsts c;
  SpWs ws;
  int rc = sp_setup<Game>(rules, w, cfg, st, rec, lanes, num_games, workspace, workspace_bytes, stats, &c, &ws);
  if (rc || lanes == 0 || num_games == 0) return rc;
  if ((rc = Game::clear(rec, num_games, w->obs_channels, ws, s))) return rc;
  if (stream)
    k_sp_init<Game><<<(lanes + 255) / 256, 256, 0, s>>>(c, st, ws.lane_game, ws.next_game, num_games, lanes);
  else
    k_sp_reset<Game><<<(lanes + 255) / 256, 256, 0, s>>>(c, st, lanes);
  MUZ_HIP_RET(hipGetLastError());
  Game game(c, *w, *cfg, st, rec, lanes, ws, stream, num_games, s);
  return sp_turns(game, stream ? stream_max_turns(num_games, lanes, rec.max_steps) : rec.max_steps, stats, s);
}

}  // namespace muz
