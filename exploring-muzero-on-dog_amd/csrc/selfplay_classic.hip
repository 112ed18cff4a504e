// Native self-play driver for classic MADN with Stochastic MuZero: play_n_games_v3 /
// play_batch_of_games_jitted of MuZero_Classic_MADN/game_agent_stochastic.py:52-257, as a host loop of
// stream-ordered HIP launches (same structure as the det driver, selfplay.hip).
//
// Per turn: throw the die of every active game (counter RNG -> throw_die) + legal masks + flags ->
// device compaction of the games that search -> encode -> root inference -> stochastic search ->
// env_step / no_step + trajectory records (incl. the die and the next state's dice distribution).
#include "classic.hpp"
#include "compact.hpp"
#include "host_consts.hpp"
#include "launch.hpp"
#include "rng.hpp"
#include "selfplay_host.hpp"

namespace muz {

constexpr int kCsBlock = 256;
constexpr unsigned long long kDieStream = 0xD1CE5EEDF00DULL;

// Die of the turn: u = U[0,1) from (seed ^ kDieStream, game, turn), die = throw_die(env, u).
__device__ __forceinline__ float die_uniform(unsigned long long seed, int g, int turn) {
  return u24(mix64(game_key(seed ^ kDieStream, g, turn)));
}

// The die of lane g's game: its game number (lane_game, streaming driver) and own step count (== the
// turn in a batch) key the draw, so a game throws the same dice in whichever lane it is played.
__global__ __launch_bounds__(kCsBlock) void k_cs_flags(DetConsts c, muz_classic_soa st, unsigned long long seed,
                                                       const int32_t* idx, int T, const int32_t* lane_game,
                                                       uint32_t* legal, int32_t* flag, int n) {
  __shared__ int8_t sboard[kCells * kCsBlock];
  const int g = blockIdx.x * kCsBlock + threadIdx.x;
  if (g >= n) return;
  const int gn = lane_game ? lane_game[g] : g;
  if (st.done[g] || gn < 0 || idx[gn] >= T) {   // do_skip_step: nothing happens to a finished game
    flag[g] = 0;
    legal[g] = 0;
    return;
  }
  BoardView b{sboard + threadIdx.x, kCsBlock};
  ClsLane s;
  cls_load(c, st, g, s, b);
  float p[6];
  cls_dice_probs(c, cls_soft_locked(c, s, b), p);
  s.die = cls_choice(p, die_uniform(seed, gn, idx[gn]));
  st.die[g] = (int8_t)s.die;
  const uint32_t l = cls_legal(c, s, b);
  legal[g] = l;
  flag[g] = l ? 1 : 2;
}

// Observation (after the die) of every searching game, compacted order, + its int8 record.
__global__ __launch_bounds__(64) void k_cs_encode(DetConsts c, muz_classic_soa st, const int32_t* list,
                                                  const int32_t* counts, const uint32_t* legal, uint32_t* legal_c,
                                                  float* obs, int8_t* traj_obs, const int32_t* idx, int T,
                                                  const int32_t* lane_game) {
  const int sl = blockIdx.x;
  if (sl >= counts[0]) return;
  const int w = threadIdx.x;
  if (w >= kCells) return;
  const int g = list[sl];
  if (w == 0) legal_c[sl] = legal[g];
  const int S = st.stride;
  ClsLane s;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int v = st.pins[min(j, c.P * 4 - 1) * S + g];
    s.pins[j] = (j < c.P * 4) ? v : -1;
  }
  s.cp = st.current_player[g];
  s.die = st.die[g];
  const int C = 2 * c.P + 3;
  float* o = obs + (size_t)sl * C * kCells;
  const int gn = lane_game ? lane_game[g] : g;
  int8_t* to = traj_obs + ((size_t)gn * T + idx[gn]) * C * kCells;
  auto owner = [&](int cell) { return (int)st.board[cell * S + g]; };
  for (int ch = 0; ch < C; ++ch) {
    const int v = cls_encode_value(c, s, ch, w, owner);
    o[ch * kCells + w] = (float)v;
    to[ch * kCells + w] = (int8_t)v;
  }
}

// do_mcts / do_skip + the buffer update (game_agent_stochastic.py:104-174).
__global__ __launch_bounds__(kCsBlock) void k_cs_apply(DetConsts c, muz_classic_soa st, const int32_t* flag,
                                                       const int32_t* slot, const int32_t* s_action,
                                                       const float* s_weights, const float* s_value, muz_traj tr,
                                                       muz_traj_chance ch, int n, const int32_t* lane_game,
                                                       const uint32_t* legal) {
  __shared__ int8_t sboard[kCells * kCsBlock];
  const int g = blockIdx.x * kCsBlock + threadIdx.x;
  if (g >= n) return;
  const int f = flag[g];
  if (f == 0) return;
  BoardView b{sboard + threadIdx.x, kCsBlock};
  ClsLane s;
  cls_load(c, st, g, s, b);
  const bool teams = has(c.flags, R_TEAMS);
  const int T = tr.max_steps;
  const int gn = lane_game ? lane_game[g] : g;
  const int t = tr.idx[gn];
  const size_t rec = (size_t)gn * T + t;
  const int cp_before = s.cp;
  const int team_before = teams ? cp_before % 2 : -1;
  const int die = s.die;
  int act, rew_cls, disc_cls;
  float val, mask;
  if (f == 1) {
    const int sl = slot[g];
    act = s_action[sl];
    const int r = cls_step_masked(c, s, b, act, legal[g]);   // legal[g]: this state's mask (k_cs_flags)
    const bool nd = s.done != 0;
    const int next_team = teams ? s.cp % 2 : -1;
    rew_cls = (nd && r > 0) ? 2 : ((nd && r < 0) ? 0 : 1);
    disc_cls = nd ? 1 : (teams ? (team_before == next_team ? 2 : 0) : (cp_before == s.cp ? 2 : 0));
    val = s_value[sl];
    mask = 1.f;
    for (int a = 0; a < MUZ_CLASSIC_ACTIONS; ++a)
      tr.pol[rec * MUZ_CLASSIC_ACTIONS + a] = s_weights[(size_t)sl * MUZ_CLASSIC_ACTIONS + a];
  } else {
    s.cp = (s.cp + 1) % c.P;   // no_step (353-365); obs / policy records stay zero
    act = -1;
    rew_cls = 1;
    disc_cls = 1;
    val = 0.f;
    mask = 0.f;
  }
  cls_store(c, st, g, s, b);
  float p[6];
  cls_dice_probs(c, cls_soft_locked(c, s, b), p);   // dice_probabilities(next_env) (line 162)
  for (int i = 0; i < 6; ++i) ch.dice_dist[rec * 6 + i] = p[i];
  ch.dice[rec] = die;
  tr.act[rec] = act;
  tr.rew[rec] = rew_cls;
  tr.val[rec] = val;
  tr.mask[rec] = mask;
  tr.player[rec] = cp_before;
  tr.team[rec] = team_before;
  tr.discount[rec] = disc_cls;
  tr.idx[gn] = t + 1;
}

__device__ void cls_reset_lane(const DetConsts& c, const muz_classic_soa& st, int g) {
  madn_reset_lane(c, st, g);
  st.die[g] = 0;
}

// Streaming refill (one workgroup, deterministic): every lane whose game ended (done, or its record is full) takes
// the next unplayed game number in lane order and is reset; lanes left without a game go idle (-1).  next[0] = next
// unplayed game number.
__global__ __launch_bounds__(kScanThreads) void k_cs_refill(DetConsts c, muz_classic_soa st, int32_t* lane_game,
                                                            const int32_t* idx, int T, int32_t* next, int num_games,
                                                            int W) {
  __shared__ int part[kScanThreads];
  const int t = threadIdx.x;
  const int chunk = (W + kScanThreads - 1) / kScanThreads;
  const int lo = min(W, t * chunk), hi = min(W, lo + chunk);
  auto ended = [&](int l) {
    const int gn = lane_game[l];
    return gn >= 0 && (st.done[l] || idx[gn] >= T);
  };
  int cnt = 0;
  for (int l = lo; l < hi; ++l) cnt += ended(l);
  part[t] = cnt;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const int base = next[0];
  int r = part[t] - cnt;
  for (int l = lo; l < hi; ++l) {
    if (!ended(l)) continue;
    const int gn = base + r++;
    if (gn < num_games) {
      lane_game[l] = gn;
      cls_reset_lane(c, st, l);
    } else {
      lane_game[l] = -1;
    }
  }
  __syncthreads();
  if (t == kScanThreads - 1) next[0] = min(num_games, base + part[t]);
}

// The turn's search as sp_turns launches it (see GumbelTurn, selfplay.hip)
struct StochasticTurn {
  SArgs sa;
  StochasticTurn(const muz_stoch_cfg& cfg, const int32_t* lane_game, const int32_t* idx)
      : sa(make_sargs(cfg, MUZ_CLASSIC_ACTIONS)) {
    sa.key_game = lane_game;
    sa.key_turn = idx;   // the game's own step count (== the turn for every game of a batch)
  }
  int operator()(const muz_classic_net_w& w, const SpWs& ws, int n, const int* counts, int turn, hipStream_t s) {
    sa.turn = turn;
    return launch_stochastic_search(w, sa, ws.root_logits, ws.root_value, ws.root_emb, ws.legal_c, nullptr, nullptr,
                                    ws.list, n, counts, ws.tree, ws.action, ws.weights, ws.value, s);
  }
};

// The records of a classic game: the det keys and, beside them, the die and the next state's dice distribution
struct ClassicRecords : muz_traj {
  muz_traj_chance ch;
};

// Classic MADN as the turn loop plays it (selfplay_host.hpp: sp_turns): the head is four launches (refill, flags,
// compaction, encode) and the apply follows the search within the turn.
struct ClassicGame {
  using Net = muz_classic_net_w;
  using Cfg = muz_stoch_cfg;
  using Soa = muz_classic_soa;
  using Records = ClassicRecords;
  static int check(const Net* w, const Cfg* cfg, int P) {
    if (!cfg) return MUZ_E_INVALID;
    if (int rc = check_classic_net(w)) return rc;
    return w->obs_channels == 2 * P + 3 ? MUZ_OK : MUZ_E_UNSUPPORTED;
  }
  static bool args_ok(int lanes, int num_games, int stride, const void* workspace, const Records& rec) {
    return sp_args_ok(lanes, num_games, stride, workspace, rec, false) && rec.ch.dice && rec.ch.dice_dist;
  }
  static size_t carve(char* base, int n, int C, int S, SpWs* ws) {
    return sp_carve(base, n, C, MUZ_CLASSIC_ACTIONS, (size_t)stochastic_workspace_bytes(n, S), ws);
  }
  static int clear(const Records& rec, int games, int C, const SpWs&, hipStream_t s) {
    if (int rc = traj_clear(rec, games, C, MUZ_CLASSIC_ACTIONS, s)) return rc;
    return traj_clear(rec.ch, games, rec.max_steps, s);
  }
  static __device__ void reset_lane(const DetConsts& c, const Soa& st, int g) { cls_reset_lane(c, st, g); }

  const DetConsts& c;
  const Net& w;
  Soa st;
  Records tr;   // (with tr.ch, the chance records)
  int n;
  const SpWs& ws;
  const int32_t* lane_game;   // streaming: the game number of every lane; batch: null, lane g plays game g
  int num_games;
  unsigned long long seed;
  hipStream_t s;
  StochasticTurn search_;

  ClassicGame(const DetConsts& c, const Net& w, const Cfg& cfg, Soa st, const Records& rec, int n, const SpWs& ws,
              bool stream, int num_games, hipStream_t s)
      : c(c), w(w), st(st), tr(rec), n(n), ws(ws), lane_game(stream ? ws.lane_game : nullptr),
        num_games(num_games), seed(cfg.seed), s(s), search_(cfg, lane_game, tr.idx) {}

  TurnCounts head(int turn, TurnLedger& led) {
    const int T = tr.max_steps;
    if (lane_game)
      k_cs_refill<<<1, kScanThreads, 0, s>>>(c, st, ws.lane_game, tr.idx, T, ws.next_game, num_games, n);
    k_cs_flags<<<(n + kCsBlock - 1) / kCsBlock, kCsBlock, 0, s>>>(c, st, seed, tr.idx, T, lane_game, ws.legal,
                                                                   ws.flag, n);
    k_sp_compact<<<1, kScanThreads, 0, s>>>(ws.flag, n, ws.list, ws.slot, ws.counts);
    led.counts(turn, ws.counts);
    k_cs_encode<<<n, 64, 0, s>>>(c, st, ws.list, ws.counts, ws.legal, ws.legal_c, ws.obs, tr.obs, tr.idx, T, lane_game);
    return {ws.counts, nullptr};
  }
  int root(const TurnCounts& tc) {
    return launch_root_inference(w, ws.obs, n, tc.dev, ws.conv, ws.root_logits, ws.root_value, ws.root_emb, s);
  }
  int search(const int32_t* counts, int turn) { return search_(w, ws, n, counts, turn, s); }
  void after_search(int) {
    k_cs_apply<<<(n + kCsBlock - 1) / kCsBlock, kCsBlock, 0, s>>>(c, st, ws.flag, ws.slot, ws.action, ws.weights,
                                                                   ws.value, tr, tr.ch, n, lane_game, ws.legal);
  }
  int finish() { return MUZ_OK; }
};

}  // namespace muz

using namespace muz;

extern "C" {

int64_t muz_classic_selfplay_workspace_bytes(int32_t n, int32_t obs_channels, const muz_stoch_cfg* cfg) {
  if (!cfg || n < 0 || cfg->num_simulations < 1) return -1;
  return (int64_t)ClassicGame::carve(nullptr, n, obs_channels, cfg->num_simulations, nullptr);
}

int muz_classic_selfplay(const muz_rules* rules, const muz_classic_net_w* w, const muz_stoch_cfg* cfg,
                         muz_classic_soa st, muz_traj tr, muz_traj_chance ch, int32_t n, void* workspace,
                         int64_t workspace_bytes, muz_sp_stats* stats, void* stream) {
  return sp_play<ClassicGame>(rules, w, cfg, st, {tr, ch}, n, n, false, workspace, workspace_bytes, stats,
                              (hipStream_t)stream);
}

int muz_classic_selfplay_stream(const muz_rules* rules, const muz_classic_net_w* w, const muz_stoch_cfg* cfg,
                                muz_classic_soa st, muz_traj tr, muz_traj_chance ch, int32_t num_games, int32_t lanes,
                                void* workspace, int64_t workspace_bytes, muz_sp_stats* stats, void* stream) {
  return sp_play<ClassicGame>(rules, w, cfg, st, {tr, ch}, num_games, lanes, true, workspace, workspace_bytes, stats,
                              (hipStream_t)stream);
}

}  // extern "C"
