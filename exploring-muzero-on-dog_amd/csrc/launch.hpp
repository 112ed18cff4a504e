// Internal (C++) launchers shared between translation units.  `n_dev`, when non-null, is a
// device-resident row count that overrides `n` (grids are sized for `n`; surplus workgroups exit),
// so a device-compacted batch can be processed without a host round trip.
#pragma once
#include "common.hpp"

namespace muz {

// The limits every search kernel is built for (its per-node and per-path-level arrays in LDS)
constexpr int kMaxSims = 100;              // S <= 100 (config (e) uses 100)
constexpr int kMaxNodes = kMaxSims + 1;
constexpr int kMaxDepth = 64;
static inline int check_search_limits(int num_simulations, int max_depth) {
  const bool ok = num_simulations >= 1 && num_simulations <= kMaxSims && max_depth >= 1 && max_depth <= kMaxDepth;
  return ok ? MUZ_OK : MUZ_E_UNSUPPORTED;
}
// What muz_gumbel_search, muz_puct_search and muz_stochastic_search check once the network and the policy's own
// settings are accepted: the limits (unsupported), then the buffers every search takes and the workspace size (invalid;
// need: the search's workspace bytes for (n, num_simulations)).
static inline int check_search_call(int num_simulations, int max_depth, int n, const void* root_logits,
                                    const void* root_value, const void* root_embedding, const void* legal_bits,
                                    const void* workspace, int64_t workspace_bytes, int64_t (*need)(int, int),
                                    const void* action, const void* action_weights, const void* root_value_out) {
  if (check_search_limits(num_simulations, max_depth)) return MUZ_E_UNSUPPORTED;
  MUZ_HOST_CHECK(n >= 0 && root_logits && root_value && root_embedding && legal_bits && workspace && action &&
                 action_weights && root_value_out);
  MUZ_HOST_CHECK(workspace_bytes >= need(n, num_simulations));
  return MUZ_OK;
}

// MUZ_RING_ADDR (read per launch): the dense layers' weight addressing in k_gumbel_search (default form),
// k_root_dense and k_recurrent -- unset or 1: a scalar base and one 32-bit lane offset (nn.hpp, SB); 0: the form
// before, 64-bit addresses per lane, kept for A/B runs and tests/test_gpu_ring_addressing.py
static inline bool ring_scalar_base() {
  const char* e = getenv("MUZ_RING_ADDR");
  return !e || atoi(e) != 0;
}

struct SearchArgs {
  int S, D, max_considered;
  float value_scale, maxvisit_init, gumbel_scale;
  unsigned long long seed;
  int turn;
  // Optional noise keys of a self-play driver: the game id of lane l is key_game[l] (else l) and its
  // turn key_turn[game id] (else `turn`) -- the game's own step count, so a game draws the same noise
  // whichever lane and global turn it is played in.
  const int32_t* key_game = nullptr;
  const int32_t* key_turn = nullptr;
  int exact_select = 0;   // k_dog_search: every interior selection on the exact path (MUZ_DOG_EXACT_SELECT)
  int games_per_wg = 8;   // k_dog_search one-game-per-wave form: games per workgroup (<= 8; MUZ_DOG_GPW)
};
static inline SearchArgs make_search_args(const muz_search_cfg& cfg) {
  SearchArgs sa;
  sa.S = cfg.num_simulations;
  sa.D = cfg.max_depth;
  sa.max_considered = cfg.max_num_considered;
  sa.value_scale = cfg.value_scale;
  sa.maxvisit_init = cfg.maxvisit_init;
  sa.gumbel_scale = cfg.gumbel_scale;
  sa.seed = cfg.seed;
  sa.turn = cfg.turn;
  return sa;
}

// host_counts (optional): the self-play ledger's mapped pinned slot; k_repr_conv's first workgroup copies n_dev[0..1]
// (the turn's searching / active counts, final once the turn head has run) into it
int launch_root_inference(const muz_net_w& w, const float* obs, int n, const int* n_dev, float* conv_scratch,
                          float* logits, float* value, float* emb, hipStream_t s, int32_t* host_counts = nullptr);

int launch_root_inference(const muz_classic_net_w& w, const float* obs, int n, const int* n_dev, float* conv_scratch,
                          float* logits, float* value, float* emb, hipStream_t s);

// k_repr_conv (RepresentationNetwork2's convolutions, nets.hip) and k_film (the per-action FiLM table)
int launch_repr_conv(const muz_repr_w& r, const float* obs, int C, int n, const int* n_dev, float* conv,
                     hipStream_t s, int32_t* host_counts = nullptr);
// k_dense0 (nets.hip): Dense_0 (3584 -> 256) of every row of the root scratch, 64 x 64 output tiles
int launch_dense0(const muz_dense& d0, int n, const int* n_dev, float* conv, hipStream_t s);
int launch_film(const muz_dyn_w& d, int A, hipStream_t s);

int launch_gumbel_search(const muz_net_w& w, const SearchArgs& sa, const float* root_logits, const float* root_value,
                         const float* root_emb, const uint32_t* legal, const float* gumbel, const int32_t* game_id,
                         int n, const int* n_dev, void* workspace, int32_t* action, float* weights, float* value,
                         hipStream_t s);

int64_t search_workspace_bytes(int n, int S);

// PUCT MuZero search for det-MADN (puct_search.hip); its workspace is the Gumbel search's (search_workspace_bytes)
struct PuctArgs {
  int S, D, qtransform;
  float min_value, max_value, dir_frac, dir_alpha, pb_c_init, pb_c_base, temperature;
  unsigned long long seed;
  int turn;
  // optional noise keys of a self-play driver (see SearchArgs): game id key_game[lane], turn key_turn[game id]
  const int32_t* key_game = nullptr;
  const int32_t* key_turn = nullptr;
};
// (the settings muz_puct_cfg and muz_stoch_cfg both have, under the same names)
template <class Cfg>
static inline PuctArgs puct_args_of(const Cfg& cfg, int qtransform, float min_value, float max_value) {
  PuctArgs pa;
  pa.S = cfg.num_simulations;
  pa.D = cfg.max_depth;
  pa.qtransform = qtransform;
  pa.min_value = min_value;
  pa.max_value = max_value;
  pa.dir_frac = cfg.dirichlet_fraction;
  pa.dir_alpha = cfg.dirichlet_alpha;
  pa.pb_c_init = cfg.pb_c_init;
  pa.pb_c_base = cfg.pb_c_base;
  pa.temperature = cfg.temperature;
  pa.seed = cfg.seed;
  pa.turn = cfg.turn;
  return pa;
}
static inline PuctArgs make_puct_args(const muz_puct_cfg& cfg) {
  return puct_args_of(cfg, cfg.qtransform, cfg.min_value, cfg.max_value);
}
// muz_classic_mcts (classic_env_mcts.hip) runs the same frame from a muz_stoch_cfg: mctx's default qtransform,
// parent-and-siblings, between the value bounds -1 and 1
static inline PuctArgs make_puct_args(const muz_stoch_cfg& cfg) {
  return puct_args_of(cfg, MUZ_QT_PARENT_SIBLINGS, -1.f, 1.f);
}
// muz_puct_cfg's own settings, as every entry point that takes one refuses them (written so that a NaN is refused too)
static inline int check_puct_cfg(const muz_puct_cfg& cfg) {
  if (cfg.qtransform != MUZ_QT_MIN_MAX && cfg.qtransform != MUZ_QT_PARENT_SIBLINGS) return MUZ_E_UNSUPPORTED;
  if (!(cfg.max_value > cfg.min_value)) return MUZ_E_UNSUPPORTED;
  if (!(cfg.dirichlet_fraction >= 0.f && cfg.dirichlet_fraction <= 1.f)) return MUZ_E_UNSUPPORTED;
  if (!(cfg.dirichlet_alpha > 0.f) || !(cfg.pb_c_base > 0.f) || !(cfg.temperature >= 0.f)) return MUZ_E_UNSUPPORTED;
  return MUZ_OK;
}
// muz_stoch_cfg's own settings, as muz_classic_mcts refuses them (written so that a NaN is refused too;
// muz_stochastic_search keeps its own checks)
static inline int check_stoch_cfg(const muz_stoch_cfg& cfg) {
  if (!(cfg.dirichlet_fraction >= 0.f && cfg.dirichlet_fraction <= 1.f)) return MUZ_E_UNSUPPORTED;
  if (!(cfg.dirichlet_alpha > 0.f) || !(cfg.pb_c_base > 0.f) || !(cfg.temperature >= 0.f)) return MUZ_E_UNSUPPORTED;
  if (!(cfg.pb_c_init == cfg.pb_c_init)) return MUZ_E_UNSUPPORTED;
  return MUZ_OK;
}
int launch_puct_search(const muz_net_w& w, const PuctArgs& pa, const float* root_logits, const float* root_value,
                       const float* root_emb, const uint32_t* legal, const float* dirichlet, const float* gumbel,
                       const int32_t* game_id, int n, const int* n_dev, void* workspace, int32_t* action,
                       float* weights, float* value, hipStream_t s);

// Stochastic MuZero (stochastic.hip)
struct SArgs {
  int S, D, A;
  float dir_frac, dir_alpha, pb_c_init, pb_c_base, temperature;
  unsigned long long seed;
  int turn;
  // optional noise keys of a self-play driver (see SearchArgs): game id key_game[lane], turn key_turn[game id]
  const int32_t* key_game = nullptr;
  const int32_t* key_turn = nullptr;
};
SArgs make_sargs(const muz_stoch_cfg& cfg, int A);
int launch_stochastic_search(const muz_classic_net_w& w, const SArgs& sa, const float* root_logits,
                             const float* root_value, const float* root_emb, const uint32_t* legal,
                             const float* dirichlet, const float* gumbel, const int32_t* game_id, int n, const int* n_dev,
                             void* workspace, int32_t* action, float* weights, float* value, hipStream_t s);
int64_t stochastic_workspace_bytes(int n, int S);
int check_classic_net(const muz_classic_net_w* w);

}  // namespace muz
