// Host-side scaffolding the native self-play drivers share (selfplay.hip, selfplay_classic.hip): the workspace
// carve, the argument checks, the trajectory clear and the streaming drivers' turn bound.
#pragma once
#include <algorithm>

#include "detmadn.hpp"

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

// Streaming drivers: at most ceil(num_games / lanes) generations of T turns each
static inline int stream_max_turns(int num_games, int lanes, int T) {
  const long long gens = ((long long)num_games + lanes - 1) / lanes;
  return (int)std::min<long long>(gens * T + 1, 1 << 30);
}

}  // namespace muz
