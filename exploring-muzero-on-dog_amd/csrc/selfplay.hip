// Native self-play driver for deterministic MADN: play_n_games_v3 / play_batch_of_games_jitted
// (MuZero_det_MADN/game_agent.py:50-192) as a host loop of stream-ordered HIP launches.
//
// Per turn: legal masks + active flags for every game -> deterministic device compaction of the
// games that search (has a legal move) -> encode their observations -> root inference ->
// persistent search (Gumbel, or muzero_policy's PUCT: muz_detmadn_selfplay_puct) -> env_step / no_step +
// trajectory records.  Unlike the reference's vmap-of-cond, finished games and no-move turns cost no
// network work, and there is no host round trip inside a turn: batch sizes live on the device (`counts`), surplus workgroups exit early.
// The host checks the active-game count two turns late (pinned memory + events), so the GPU queue
// never drains; the at most two trailing turns it launches find no active game and record nothing.
// The streaming driver's turn head also plays no-move turns where it finds them (fast-forward, k_sp_head), so a
// game without a move does not sit out a whole launched turn; MUZ_SP_FASTFORWARD=0 turns that off.
#include <algorithm>
#include <cstdlib>

#include "detmadn.hpp"
#include "host_consts.hpp"
#include "launch.hpp"
#include "selfplay_host.hpp"

namespace muz {

// lane kernels' workgroup size; 64 / 128 measured within noise of 256 (profiles/r1g_sp_block_ab.log)
constexpr int kSpBlock = 256;
// One game per kFlagLanes lanes in every lane kernel (a lane per game would leave a 4096-game batch on 16 of 256 CUs,
// a game's 24 legality checks serial in one lane): the workgroup copies its games' SoA rows into LDS (coalesced) and
// each game's lanes work on them in parallel.
constexpr int kFlagLanes = 32;

// Apply the searched action (env_step) or no_step, and write the trajectory record (game_agent.py:79-141): the
// workgroup's SoA rows go through LDS both ways (coalesced), lane 0 of a game steps it on its LDS rows (LdsLane),
// its lanes copy the 24 action weights into the record.
// The apply of one game's searched action (or no_step) on its LDS rows and its trajectory record; lane a of the
// game's G lanes, f / sl / leg: the game's flag, slot and legal mask of the turn being applied.
template <int G>
__device__ __forceinline__ void sp_apply_game(const DetConsts& c, int8_t* sp, int8_t* board, int f, int sl, uint32_t leg,
                                              int gn, int tt, const int32_t* s_action, const float* s_weights,
                                              const float* s_value, const muz_traj& tr, int a) {
  const int T = tr.max_steps;
  const size_t rec = (size_t)gn * T + tt;
  if (f == 1 && a < MUZ_DET_ACTIONS)
    tr.pol[rec * MUZ_DET_ACTIONS + a] = s_weights[(size_t)sl * MUZ_DET_ACTIONS + a];
  if (f != 0 && a == 0) {
    LdsLane s{sp, sp[40], sp[41], sp[42]};
    const BoardView b{board, 1};
    const bool teams = has(c.flags, R_TEAMS);
    const int cp_before = s.cp;
    const int team_before = teams ? cp_before % 2 : -1;
    int act, rew_cls, disc_cls;
    float val, mask;
    if (f == 1) {
      act = s_action[sl];
      // leg: this state's mask from the flags pass (the state is unchanged since), so no second legality pass
      const int r = det_step_masked(c, s, b, fdiv(act, 6), fmodp(act, 6) + 1, leg);
      const bool nd = s.done != 0;
      const int next_player = s.cp;
      const int next_team = teams ? next_player % 2 : -1;
      rew_cls = (nd && r > 0) ? 2 : ((nd && r < 0) ? 0 : 1);
      disc_cls = nd ? 1 : (teams ? (team_before == next_team ? 2 : 0) : (cp_before == next_player ? 2 : 0));
      val = s_value[sl];
      mask = 1.f;
    } else {
      det_nostep(c, s);   // obs / policy records stay zero (buffers are zeroed per call)
      act = -1;
      rew_cls = 1;
      disc_cls = 1;
      val = 0.f;
      mask = 0.f;
    }
    sp[40] = (int8_t)s.cp;
    sp[41] = (int8_t)s.done;
    sp[42] = (int8_t)s.reward;
    tr.act[rec] = act;
    tr.rew[rec] = rew_cls;
    tr.val[rec] = val;
    tr.mask[rec] = mask;
    tr.player[rec] = cp_before;
    tr.team[rec] = team_before;
    tr.discount[rec] = disc_cls;
    tr.idx[gn] = tt + 1;
  }
}

__global__ __launch_bounds__(kSpBlock) void k_sp_apply_g(DetConsts c, muz_detmadn_soa st, const int32_t* flag,
                                                         const int32_t* slot, const int32_t* s_action,
                                                         const float* s_weights, const float* s_value, muz_traj tr,
                                                         int n, const int32_t* lane_game, const uint32_t* legal) {
  constexpr int G = kFlagLanes, NG = kSpBlock / G;
  __shared__ int8_t sboard[NG][kCells];
  __shared__ int8_t sstate[NG][kStateRow];
  const int t = threadIdx.x, lg = t / G, a = t % G;
  const int g0 = blockIdx.x * NG, games = min(NG, n - g0), g = g0 + lg;
  det_rows_load<NG>(c, st, g0, games, sboard, sstate, t, kSpBlock);
  const int f = lg < games ? flag[g] : 0;
  const int gn = f ? (lane_game ? lane_game[g] : g) : 0;
  const int tt = f ? tr.idx[gn] : 0;   // read by every lane of the game before lane 0 advances it
  __syncthreads();
  if (f) sp_apply_game<G>(c, sstate[lg], sboard[lg], f, slot[g], legal[g], gn, tt, s_action, s_weights, s_value, tr, a);
  __syncthreads();
  det_rows_store<NG>(c, st, g0, games, sboard, sstate, t, kSpBlock);
}

// ---- the turn head as one launch: refill + flags + compaction + encode ------------------------------------------
//  * refill (streaming driver): every lane whose game ended (done, or its record is full: idx == T, the
//    reference's max_steps) takes the next unplayed game number and is reset; lanes left without a game go idle
//    (-1).  next[0] counts the numbers handed out;
//  * flags: the legal mask of every lane's game (det_legal_g, one ballot per 32 actions) and 1 = searches (a legal
//    move), 2 = no move (no_step), 0 = idle;
//  * fast-forward (streaming driver, kSpFfCap below): a game flagged 2 plays its no_step turn at once on its LDS
//    rows (sp_apply_game with f == 2) and is flagged again for the next player, until it has a move, its record is
//    full (idle this turn, refilled by the next head) or the cap; flag, mask, slot and counts below are those of
//    the state after it, and idx is final in global memory before the search reads it as key_turn;
//  * compaction: slot sl of the searching games plays lane list[sl]; counts = (searching, active);
//  * encode: the observation of every searching game at its slot as fp32 for root inference + its int8 trajectory
//    record.  The game's lanes stage the encode in LDS (det_enc_stage: rel[56] + constant channels) and write both
//    outputs from the staging -- fp32 as float4 per 4 cells of a channel (56 = 14 x 4; 4 bytes = one v_perm_b32
//    through the channel table), int8 as 16-byte chunks -- consecutive lanes on consecutive chunks of the game's
//    contiguous block.
// As four launches these cost ~37 us per turn at 4096 lanes, most of it two single-workgroup scans and kernel
// boundaries (profiles/r5s_kernel_stats.csv).  Here every workgroup loads its rows once and takes its
// share of the two lane-order counts the head needs -- refilled lanes' game numbers, searching games' slots -- with
// one device atomic each.  The workgroups' order among themselves then decides which lane takes which new game
// number and which slot a searching game gets, but no result: a game's search, records and noise depend on its
// game number and its own step count only (key_game / key_turn), never on its lane or its slot, and the set of game
// numbers handed out per turn is the same (tests/test_gpu_selfplay.py: stream == batch, oracle parity).  (Ordered
// alternatives measured: a decoupled look-back over the 512 workgroups, 262 us serial / 69 us 64-wide -- each poll
// an agent-scope load across XCDs.)
// counts: this turn's [searching, active, -, arrivals]; the next turn's four (the other parity) are zeroed here.
// 32 games per workgroup (128 workgroups at 4096 lanes): the same-address atomics serialise, so fewer, larger
// workgroups take fewer of them.
constexpr int kHeadBlock = 1024;
// Fast-forward (streaming driver): a no-move turn needs det_nostep and seven scalar records, yet left to the next
// head it holds its lane out of a whole turn -- root inference and a search launch whose length is one tile's serial
// chain of simulations, whatever the batch.  The flags pass plays up to kSpFfCap of them per game on the spot (longer
// runs finish in the next heads: no result depends on the cap), so every launched lane-turn but those carries a
// search.  Records are keyed by game number and step count, so they stay bit for bit; only the batched turn in
// which a step happens changes, and `turns` shrinks.  The batch driver keeps one reference turn per launch.
constexpr int kSpFfCap = 4;

struct SpHead {
  uint32_t* legal;
  int32_t* flag;
  int32_t* list;
  int32_t* slot;
  int32_t* counts;        // this turn's four counters (zeroed by the previous turn's head or the driver)
  int32_t* counts_next;   // the next turn's four, zeroed here
  uint32_t* legal_c;
  float* obs;
  int8_t* traj_obs;
  int32_t* host_counts;   // the turn's pinned ledger slot (device-visible), or null
  // APPLY: the previous turn's search results, applied first (what k_sp_apply_g did at the end of that turn)
  const int32_t* s_action;
  const float* s_weights;
  const float* s_value;
  muz_traj tr;
  int ff_cap;             // STREAM: no-move turns the flags pass plays per game and launch (0: none, <= kSpFfCap)
};

// the game's lanes order their LDS accesses around lane 0's step (half a wave: no workgroup barrier)
__device__ __forceinline__ void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// STREAM: the lane refill first (lane_game / next) and the fast-forward in the flags pass (o.ff_cap); otherwise
// lane g plays game g, one reference turn per launch.
// APPLY: the previous turn's apply first (k_sp_apply_g, on the rows this launch loads anyway): one launch and one
// round trip of the rows fewer per turn.
template <bool STREAM, bool APPLY>
__global__ __launch_bounds__(kHeadBlock) void k_sp_head(DetConsts c, muz_detmadn_soa st, int n, const int32_t* idx, int T,
                                                      int32_t* lane_game, int32_t* next, int num_games, SpHead o) {
  constexpr int G = kFlagLanes, NG = kHeadBlock / G;
  __shared__ int8_t sboard[NG][kCells];
  __shared__ int8_t sstate[NG][kStateRow];
  __shared__ __attribute__((aligned(16))) uint8_t senc[NG][kEncStride];
  __shared__ int s_gn[NG], s_f[NG], s_pre, s_reset, s_ffwd;
  const int t = threadIdx.x, lg = t / G, a = t % G;
  const int b = blockIdx.x, nb = gridDim.x;
  const int g0 = b * NG, games = min(NG, n - g0), g = g0 + lg;
  det_rows_load<NG>(c, st, g0, games, sboard, sstate, t, kHeadBlock);
  int fprev = 0, slprev = 0, gnprev = 0, ttprev = 0;
  uint32_t legprev = 0;
  if (APPLY && lg < games) {   // the previous turn's flag / slot / mask, read before this turn's passes rewrite them
    fprev = o.flag[g];
    if (fprev) {
      slprev = o.slot[g];
      legprev = o.legal[g];
      gnprev = STREAM ? lane_game[g] : g;
      ttprev = idx[gnprev];
    }
  }
  if (t < NG) {
    s_gn[t] = -1;
    s_f[t] = 0;
  }
  if (t == 0) s_reset = s_ffwd = 0;
  if (b == 0 && t < 4) o.counts_next[t] = 0;
  __syncthreads();
  if (APPLY) {
    if (fprev)
      sp_apply_game<G>(c, sstate[lg], sboard[lg], fprev, slprev, legprev, gnprev, ttprev, o.s_action, o.s_weights,
                       o.s_value, o.tr, a);
    __syncthreads();   // (the refill below reads the advanced idx and the new done flags)
  }
  if constexpr (STREAM) {
    // refill: every lane whose game ended takes the next unplayed game number (next[0] counts the
    // numbers handed out, possibly past num_games: those lanes go idle)
    if (t < games) {
      const int gn = lane_game[g0 + t];
      s_gn[t] = gn;
      s_f[t] = gn >= 0 && (sstate[t][41] || idx[gn] >= T);
    }
    __syncthreads();
    if (t == 0) {
      int cnt = 0;
      for (int i = 0; i < games; ++i) cnt += s_f[i];
      int r = cnt ? atomicAdd(next, cnt) : 0;
      for (int i = 0; i < games; ++i)
        if (s_f[i]) {
          s_gn[i] = r < num_games ? r : -1;
          s_reset |= r < num_games;
          ++r;
        }
    }
    __syncthreads();
    if (t < games && s_f[t]) lane_game[g0 + t] = s_gn[t];
    if (s_reset) {   // DetGame::reset_lane on the LDS rows of the refilled lanes (stored back below)
      const bool fp = has(c.flags, R_FREE_PIN);
      for (int i = t; i < NG * kCells; i += kHeadBlock) {
        const int gi = i / kCells, cell = i % kCells;
        if (gi < games && s_f[gi] && s_gn[gi] >= 0) {
          int v = -1;
          for (int p = 0; p < c.P; ++p)
            if (fp && cell == c.start[p]) v = p;
          sboard[gi][cell] = (int8_t)v;
        }
      }
      for (int i = t; i < NG * kStateRow; i += kHeadBlock) {
        const int gi = i / kStateRow, r = i % kStateRow;
        if (gi < games && s_f[gi] && s_gn[gi] >= 0) {
          int8_t v = sstate[gi][r];
          if (r < 16) v = r < 4 * c.P ? (int8_t)((fp && (r & 3) == 0) ? c.start[r >> 2] : -1) : (int8_t)-1;
          else if (r < 40) v = r - 16 < 6 * c.P ? (int8_t)4 : (int8_t)0;
          else if (r == 40) v = (int8_t)c.starting_player;
          else if (r == 41 || r == 42) v = 0;
          sstate[gi][r] = v;
        }
      }
    }
    __syncthreads();
    if (t < NG) s_f[t] = 0;
    __syncthreads();
  }
  // flags: 1 = searches (a legal move), 2 = no move (no_step), 0 = idle
  int tt = 0;   // the game's step count, carried through the fast-forward to the encode
  if (lg < games) {
    const int gn = STREAM ? s_gn[lg] : g;
    if (!STREAM || gn >= 0) tt = idx[gn];   // (every lane of the game, before its lane 0 advances it below)
    const bool idle = sstate[lg][41] || (STREAM && (gn < 0 || tt >= T));
    uint32_t l = 0;
    int f = 0;
    if (!idle) {   // (uniform over the game's lanes)
      l = det_legal_g<G>(c, LdsLane{sstate[lg], sstate[lg][40], 0, 0}, BoardView{sboard[lg], 1}, a, t);
      f = l ? 1 : 2;
    }
    int fc = f;   // what the compaction counts (== f but for a record filled below)
    if constexpr (STREAM) {
      // fast-forward: a game without a move plays its no_step turn here, on the rows in LDS, and is flagged again
      // for the next player -- until it has a move, its record is full or the cap (then it keeps flag 2 and the
      // next head applies it).  Local to the game's G lanes; every value below is uniform over them.
      for (int it = 0; it < o.ff_cap && f == 2; ++it) {
        sp_apply_game<G>(c, sstate[lg], sboard[lg], 2, 0, 0u, gn, tt, nullptr, nullptr, nullptr, o.tr, a);
        ++tt;
        if (a == 0) s_ffwd = 1;
        sp_wave_sync();   // lane 0's action-set row and player, before the game's lanes read them
        if (tt >= T) {
          // Record full: idle for this turn, the next head's refill replaces the game.  While game numbers are
          // left to hand out the lane still counts as active, or a turn in which every active lane ended like
          // this would stop the driver (next[0] only grows: a stale value errs to one empty turn).
          l = 0;
          f = 0;
          fc = __hip_atomic_load(next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < num_games ? 3 : 0;
          break;
        }
        l = det_legal_g<G>(c, LdsLane{sstate[lg], sstate[lg][40], 0, 0}, BoardView{sboard[lg], 1}, a, t);
        fc = f = l ? 1 : 2;
        sp_wave_sync();   // the lanes' reads, before lane 0 steps again
      }
    }
    if (a == 0) {
      o.legal[g] = l;
      o.flag[g] = f;
      s_f[lg] = fc;
    }
  }
  __syncthreads();
  // compaction: slots of the searching games; counts = (searching, active); the last workgroup to
  // arrive hands the totals to the host ledger
  if (t == 0) {
    int c1 = 0, c2 = 0;
    for (int i = 0; i < games; ++i) {
      c1 += s_f[i] == 1;
      c2 += s_f[i] != 0;
    }
    // (searching, active) as one 64-bit add: counts[0] the low word, counts[1] the high word
    const unsigned long long add = ((unsigned long long)(unsigned)c2 << 32) | (unsigned)c1;
    s_pre = add ? (int)(unsigned)atomicAdd(reinterpret_cast<unsigned long long*>(o.counts), add) : 0;
    if (o.host_counts) {
      __threadfence();
      if (atomicAdd(&o.counts[3], 1) == nb - 1) {
        __threadfence();
        const int tot1 = __hip_atomic_load(&o.counts[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int tot2 = __hip_atomic_load(&o.counts[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&o.host_counts[0], tot1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&o.host_counts[1], tot2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
  __syncthreads();
  int sl = -1;
  if (lg < games && s_f[lg] == 1) {
    sl = s_pre;
    for (int i = 0; i < lg; ++i) sl += s_f[i] == 1;
  }
  if (a == 0 && lg < games) {
    o.slot[g] = sl;
    if (sl >= 0) {
      o.list[sl] = g;
      o.legal_c[sl] = o.legal[g];
    }
  }
  // encode of this workgroup's searching games at their slots
  if (sl >= 0) det_enc_stage<G>(c, LdsLane{sstate[lg], sstate[lg][40], 0, 0}, BoardView{sboard[lg], 1}, senc[lg], a);
  __syncthreads();
  if (sl >= 0) {
    const int P = c.P, C = 8 * P + 2;
    const bool teams = has(c.flags, R_TEAMS);
    const uint8_t* e = senc[lg];
    float4* ob = reinterpret_cast<float4*>(o.obs + (size_t)sl * C * kCells);
    // channels >= 6 are constant planes (the global features): root inference reads them at cell 0 only
    // (k_root_dense: x[:, 6:, 0]; k_repr_conv reads channels 0..5), so only their first float4 is written
    const int nq = 6 * 14 + (C - 6);
    for (int u = a; u < nq; u += G) {
      const int q = u < 6 * 14 ? u : (u - 6 * 14 + 6) * 14;
      const int ch = q / 14, w0 = (q - ch * 14) * 4;
      const uint32_t rel4 = *reinterpret_cast<const uint32_t*>(e + w0);
      const uint32_t v4 = ch < P + 2 ? __builtin_amdgcn_perm(0u, det_obs_table(ch, P, teams), rel4)
                                     : (uint32_t)e[kCells + ch] * 0x01010101u;
      ob[q] = make_float4((float)(v4 & 0xFFu), (float)((v4 >> 8) & 0xFFu), (float)((v4 >> 16) & 0xFFu),
                          (float)(v4 >> 24));
    }
    const int gn = STREAM ? s_gn[lg] : g;
    uint4* to = reinterpret_cast<uint4*>(o.traj_obs + ((size_t)gn * T + tt) * C * kCells);
    for (int q = a; q < C * 7 / 2; q += G) {
      const uint2 lo = det_obs_half(e, 2 * q, P, teams), hi = det_obs_half(e, 2 * q + 1, P, teams);
      to[q] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
  }
  if (APPLY || (STREAM && (s_reset | s_ffwd))) det_rows_store<NG>(c, st, g0, games, sboard, sstate, t, kHeadBlock);
}

// The streaming driver's fast-forward cap: kSpFfCap unless MUZ_SP_FASTFORWARD says otherwise (read per call) --
// 0 selects the head without fast-forward (A/B runs), 1 .. kSpFfCap that many no-move turns per game and launch
// (tests of the cap path).
static int sp_fastforward_cap() {
  if (const char* e = getenv("MUZ_SP_FASTFORWARD")) return std::min(kSpFfCap, std::max(0, atoi(e)));
  return kSpFfCap;
}

// The turn's search, as sp_turns launches it: the compacted batch (ws.legal_c, ws.list as game_id, `counts` as the
// device-resident row count) into the per-slot ws.action / ws.weights / ws.value, noise keyed by the game's number
// (key_game = lane_game) and its own step count (key_turn = tr.idx, == the turn for every game of a batch).
struct GumbelTurn {
  using Cfg = muz_search_cfg;
  static int check(const Cfg&) { return MUZ_OK; }
  SearchArgs sa;
  GumbelTurn(const Cfg& cfg, const int32_t* lane_game, const int32_t* idx) : sa(make_search_args(cfg)) {
    sa.key_turn = idx;
    sa.key_game = lane_game;
  }
  int operator()(const muz_net_w& w, const SpWs& ws, int n, const int* counts, int turn, hipStream_t s) {
    sa.turn = turn;
    return launch_gumbel_search(w, sa, ws.root_logits, ws.root_value, ws.root_emb, ws.legal_c, nullptr, ws.list, n,
                                counts, ws.tree, ws.action, ws.weights, ws.value, s);
  }
};
// muzero_policy (puct_search.hip) on the same tree workspace; Dirichlet, tie-break and final-draw noise from the
// counter RNG (cfg.turn is not used: key_turn is set for both drivers); the policy's own settings are refused as its
// search entry point refuses them
struct PuctTurn {
  using Cfg = muz_puct_cfg;
  static int check(const Cfg& cfg) { return check_puct_cfg(cfg); }
  PuctArgs pa;
  PuctTurn(const Cfg& cfg, const int32_t* lane_game, const int32_t* idx) : pa(make_puct_args(cfg)) {
    pa.key_turn = idx;
    pa.key_game = lane_game;
  }
  int operator()(const muz_net_w& w, const SpWs& ws, int n, const int* counts, int turn, hipStream_t s) {
    pa.turn = turn;
    return launch_puct_search(w, pa, ws.root_logits, ws.root_value, ws.root_emb, ws.legal_c, nullptr, nullptr, ws.list,
                              n, counts, ws.tree, ws.action, ws.weights, ws.value, s);
  }
};

// Det MADN as the turn loop plays it (selfplay_host.hpp: sp_turns), with Search = GumbelTurn or PuctTurn.  The head is
// one launch, k_sp_head, which first applies the previous turn's searched actions: after_search only marks them
// pending, and finish() applies the last turn's.
template <class Search>
struct DetGame {
  using Net = muz_net_w;
  using Cfg = typename Search::Cfg;
  using Soa = muz_detmadn_soa;
  using Records = muz_traj;
  static int check(const Net* w, const Cfg* cfg, int P) {
    if (!w || !cfg) return MUZ_E_INVALID;
    if (w->obs_channels != 8 * P + 2 || w->num_actions != MUZ_DET_ACTIONS) return MUZ_E_UNSUPPORTED;
    return Search::check(*cfg);
  }
  // (the head writes the observation records and its workspace in 16-byte chunks)
  static bool args_ok(int lanes, int num_games, int stride, const void* workspace, const Records& tr) {
    return sp_args_ok(lanes, num_games, stride, workspace, tr, true);
  }
  static size_t carve(char* base, int n, int C, int S, SpWs* ws) {
    return sp_carve(base, n, C, MUZ_DET_ACTIONS, (size_t)search_workspace_bytes(n, S), ws);
  }
  // zeroed records, and both parities of k_sp_head's counters
  static int clear(const Records& tr, int games, int C, const SpWs& ws, hipStream_t s) {
    MUZ_HIP_RET(hipMemsetAsync(ws.counts, 0, 8 * sizeof(int32_t), s));
    return traj_clear(tr, games, C, MUZ_DET_ACTIONS, s);
  }
  static __device__ void reset_lane(const DetConsts& c, const Soa& st, int g) {
    madn_reset_lane(c, st, g);
    for (int r = 0; r < 6 * c.P; ++r) st.action_set[r * st.stride + g] = 4;
  }

  const DetConsts& c;
  const Net& w;
  Soa st;
  muz_traj tr;
  int n;
  const SpWs& ws;
  const int32_t* lane_game;   // streaming: the game number of every lane; batch: null, lane g plays game g
  int num_games, ff_cap;
  hipStream_t s;
  Search search_;
  bool pending = false;       // a turn's searched actions not applied yet

  DetGame(const DetConsts& c, const Net& w, const Cfg& cfg, Soa st, const Records& tr, int n, const SpWs& ws,
          bool stream, int num_games, hipStream_t s)
      : c(c), w(w), st(st), tr(tr), n(n), ws(ws), lane_game(stream ? ws.lane_game : nullptr), num_games(num_games),
        ff_cap(stream ? sp_fastforward_cap() : 0), s(s), search_(cfg, lane_game, tr.idx) {}

  TurnCounts head(int turn, TurnLedger& led) {
    const int T = tr.max_steps;
    const int nbh = (n + kHeadBlock / kFlagLanes - 1) / (kHeadBlock / kFlagLanes);
    int32_t* const counts = ws.counts + 4 * (turn & 1);   // (the other parity: the next turn's, zeroed by the head)
    // (the ledger's counts reach the host through root inference's first kernel: no last-arrival ticket here)
    int32_t* const host_counts = led.device_slot(turn);
    const SpHead h{ws.legal, ws.flag, ws.list, ws.slot, counts, ws.counts + 4 * ((turn + 1) & 1), ws.legal_c, ws.obs,
                   tr.obs, nullptr, ws.action, ws.weights, ws.value, tr, ff_cap};
    if (lane_game) {
      if (pending)
        k_sp_head<true, true><<<nbh, kHeadBlock, 0, s>>>(c, st, n, tr.idx, T, ws.lane_game, ws.next_game, num_games, h);
      else
        k_sp_head<true, false><<<nbh, kHeadBlock, 0, s>>>(c, st, n, tr.idx, T, ws.lane_game, ws.next_game, num_games, h);
    } else {
      if (pending)
        k_sp_head<false, true><<<nbh, kHeadBlock, 0, s>>>(c, st, n, tr.idx, T, nullptr, nullptr, num_games, h);
      else
        k_sp_head<false, false><<<nbh, kHeadBlock, 0, s>>>(c, st, n, tr.idx, T, nullptr, nullptr, num_games, h);
    }
    pending = false;
    if (!host_counts) led.counts(turn, counts);
    return {counts, host_counts};
  }
  int root(const TurnCounts& tc) {
    return launch_root_inference(w, ws.obs, n, tc.dev, ws.conv, ws.root_logits, ws.root_value, ws.root_emb, s,
                                 tc.host_slot);
  }
  int search(const int32_t* counts, int turn) { return search_(w, ws, n, counts, turn, s); }
  void after_search(int) { pending = true; }   // applied by the next turn's head, or by finish()
  int finish() {
    if (!pending) return MUZ_OK;
    k_sp_apply_g<<<(n + kSpBlock / kFlagLanes - 1) / (kSpBlock / kFlagLanes), kSpBlock, 0, s>>>(
        c, st, ws.flag, ws.slot, ws.action, ws.weights, ws.value, tr, n, lane_game, ws.legal);
    return muz_last_launch_error();
  }
};

}  // namespace muz

using namespace muz;

extern "C" {

int64_t muz_selfplay_workspace_bytes(int32_t n, int32_t obs_channels, const muz_search_cfg* cfg) {
  if (!cfg || n < 0) return -1;
  return (int64_t)DetGame<GumbelTurn>::carve(nullptr, n, obs_channels, cfg->num_simulations, nullptr);
}

int muz_detmadn_selfplay(const muz_rules* rules, const muz_net_w* w, const muz_search_cfg* cfg, muz_detmadn_soa st,
                         muz_traj tr, int32_t n, void* workspace, int64_t workspace_bytes, muz_sp_stats* stats,
                         void* stream) {
  return sp_play<DetGame<GumbelTurn>>(rules, w, cfg, st, tr, n, n, false, workspace, workspace_bytes, stats,
                                      (hipStream_t)stream);
}

int muz_detmadn_selfplay_stream(const muz_rules* rules, const muz_net_w* w, const muz_search_cfg* cfg,
                                muz_detmadn_soa st, muz_traj tr, int32_t num_games, int32_t lanes, void* workspace,
                                int64_t workspace_bytes, muz_sp_stats* stats, void* stream) {
  return sp_play<DetGame<GumbelTurn>>(rules, w, cfg, st, tr, num_games, lanes, true, workspace, workspace_bytes, stats,
                                      (hipStream_t)stream);
}

int muz_detmadn_selfplay_puct(const muz_rules* rules, const muz_net_w* w, const muz_puct_cfg* cfg, muz_detmadn_soa st,
                              muz_traj tr, int32_t n, void* workspace, int64_t workspace_bytes, muz_sp_stats* stats,
                              void* stream) {
  return sp_play<DetGame<PuctTurn>>(rules, w, cfg, st, tr, n, n, false, workspace, workspace_bytes, stats,
                                    (hipStream_t)stream);
}

int muz_detmadn_selfplay_puct_stream(const muz_rules* rules, const muz_net_w* w, const muz_puct_cfg* cfg,
                                     muz_detmadn_soa st, muz_traj tr, int32_t num_games, int32_t lanes,
                                     void* workspace, int64_t workspace_bytes, muz_sp_stats* stats, void* stream) {
  return sp_play<DetGame<PuctTurn>>(rules, w, cfg, st, tr, num_games, lanes, true, workspace, workspace_bytes, stats,
                                    (hipStream_t)stream);
}

}  // extern "C"
