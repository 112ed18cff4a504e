// muz_root_noise_diag: the searches' on-device Dirichlet root noise, read out (diagnostic; tests/test_gpu_root_noise.py
// compares it with oracle/root_noise.py).  The draw is rng.hpp's root_noise_log_gamma, the helper k_stochastic_search
// and k_puct_search call, in their geometry (16 games per workgroup, 32 lanes per game, lane a holds action a), and
// each width is normalised as its search's root block does: 4 actions as k_stochastic_search (expf, row_sum), 24 as
// k_puct_search (exp_cr, row_sum24).
#include "rng.hpp"
#include "tree.hpp"

namespace muz {
namespace {

constexpr int kClassicActions = 4;   // classic MADN: one action per pin (stochastic.hip kCls)

template <int A>
__global__ __launch_bounds__(kThreads) void k_root_noise_diag(float alpha, unsigned long long seed, int turn,
                                                              const int32_t* __restrict__ game_id, int n,
                                                              float* __restrict__ out_gamma,
                                                              float* __restrict__ out_noise) {
#pragma clang fp contract(off)
  static_assert(A == kClassicActions || A == MUZ_DET_ACTIONS, "the two searches' action counts");
  const int row = trow(), a = tsub();
  const int g = blockIdx.x * kRows + row;
  if (g < n) {   // uniform over the game's 32 lanes
    const bool ok = a < A;
    const int gid = game_id ? game_id[g] : g;
    const float lgm = ok ? root_noise_log_gamma(alpha, seed, gid, turn, a) : -INFINITY;
    const float lgx = row_max(lgm);
    float dn;
    if constexpr (A == MUZ_DET_ACTIONS) {
      const float e = ok ? exp_cr(lgm - lgx) : 0.f;
      dn = e / row_sum24(e);
    } else {
      const float e = ok ? expf(lgm - lgx) : 0.f;
      dn = e / row_sum(e);
    }
    if (ok) {
      out_gamma[(size_t)g * A + a] = expf(lgm);
      out_noise[(size_t)g * A + a] = dn;
    }
  }
}

}  // namespace
}  // namespace muz

using namespace muz;

extern "C" {

int muz_root_noise_diag(uint64_t seed, int32_t turn, const int32_t* game_id, float alpha, int32_t num_actions,
                        int32_t n, float* gamma, float* noise, void* stream) {
  if (num_actions != kClassicActions && num_actions != MUZ_DET_ACTIONS) return MUZ_E_UNSUPPORTED;
  if (!(alpha > 0.f)) return MUZ_E_UNSUPPORTED;
  MUZ_HOST_CHECK(n >= 0 && gamma && noise);
  if (n == 0) return MUZ_OK;
  const dim3 grid((n + kRows - 1) / kRows);
  hipStream_t s = (hipStream_t)stream;
  if (num_actions == MUZ_DET_ACTIONS)
    k_root_noise_diag<MUZ_DET_ACTIONS><<<grid, kThreads, 0, s>>>(alpha, seed, turn, game_id, n, gamma, noise);
  else
    k_root_noise_diag<kClassicActions><<<grid, kThreads, 0, s>>>(alpha, seed, turn, game_id, n, gamma, noise);
  return muz_last_launch_error();
}

}  // extern "C"
