"""CPU oracle: the engine's on-device Dirichlet root noise, restated (TEST INFRASTRUCTURE ONLY).

The reference draws the root noise of its muzero_policy searches with jax.random.dirichlet (threefry: not
restated).  The engine draws it inside k_stochastic_search / k_puct_search from its counter RNG (csrc/rng.hpp:
mix64, game_key, u24, root_noise_log_gamma = Marsaglia-Tsang on Box-Muller normals, then a softmax over the row of
log-gammas).  This file restates that stream in NumPy, vectorised over (game, action):

  key(game, action) = mix64(game_key(seed ^ 0x5DEECE66D, gid, turn) ^ (action + 1))
  a' = alpha + 1 if alpha < 1 else alpha;  d = a' - 1/3;  c = 1 / sqrt(9 d)
  round it = 0..31:  u1 = max(u24(mix64(key ^ (4 it + 1))), tiny),  u2 = u24(mix64(key ^ (4 it + 2)))
                     x = sqrt(-2 log u1) cos(2 pi u2);  v = 1 + c x;  skip the round if v <= 0;  v = v^3
                     u = max(u24(mix64(key ^ (4 it + 3))), tiny)
                     accept if log u < x^2 / 2 + d - d v + d log v:  log g = log(d v)
  no round accepted (probability < 1e-40): log g = log d
  alpha < 1:  log g += log(max(u24(mix64(key ^ 0xA5A5A5A5)), tiny)) / alpha     (the U^(1/alpha) boost)
  noise = softmax over the row's A log-gammas (the device's summation order for A = 4 and A = 24)

The sample stays in log space until the row is normalised, as jax.random.dirichlet does: at small alpha the boost
U^(1/alpha) is far below the smallest float32, and a row of underflowed gammas has no sum to divide by.

Precision: every operation runs in one dtype, float32 operation by operation (the device's arithmetic up to its libm's
last ulp and its contraction of a*b+c) or float64 (the exact-arithmetic twin: same uniforms, same comparisons, the
constants 1/3, 2 pi and alpha' in float64; alpha itself is the float32 number the engine is given).  The dtype is the
argument, else the one in force under oracle.nets.precision.

Near-accepts.  The two comparisons of a round (v <= 0, log u < rhs) can flip under a last-ulp difference of log / cos /
sqrt, and a flipped comparison changes the draw wholesale.  ``margin`` is, per draw, the smallest |log u - rhs| and
|1 + c x| over the rounds up to and including the accepting one; ``t`` holds every evaluated log u - rhs, so a test
can size a threshold from the float32 run's own distance to the float64 run."""
from __future__ import annotations

import numpy as np

ROOT_NOISE_STREAM = 0x5DEECE66D
BOOST_STREAM = 0xA5A5A5A5
ROUNDS = 32
TINY = np.finfo(np.float32).tiny
U64 = np.uint64


def _dtype(dtype):
    if dtype is None:
        from oracle import nets as ON
        dtype = ON._P.dtype
    dtype = np.dtype(dtype).type
    if dtype not in (np.float32, np.float64):
        raise ValueError(f"root_noise: float32 or float64, not {dtype}")
    return dtype


def mix64(x):
    """csrc/rng.hpp mix64 (the splitmix64 finaliser) on a uint64 array."""
    x = np.atleast_1d(np.asarray(x, U64))
    x = x + U64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def game_key(seed, gid, turn):
    """csrc/rng.hpp game_key: seed ^ mix64((unsigned)gid << 32 | (unsigned)turn); gid / turn int32 arrays or scalars."""
    g = (np.asarray(gid).astype(np.int64) & 0xFFFFFFFF).astype(U64)
    t = (np.asarray(turn).astype(np.int64) & 0xFFFFFFFF).astype(U64)
    return U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ mix64((g << U64(32)) | t)


def u24(h, dtype=None):
    """csrc/rng.hpp u24: U[0, 1) on a 24-bit grid (exact in either precision)."""
    T = _dtype(dtype)
    return (np.asarray(h, U64) >> U64(40)).astype(T) * T(1.0 / 16777216.0)


def root_noise_keys(seed, gids, turn, A):
    """The Gamma stream's key of every (game, action): uint64 [n, A].  turn: one int or one per game."""
    gids = np.atleast_1d(np.asarray(gids))
    turn = np.broadcast_to(np.asarray(turn), gids.shape)
    gk = game_key((int(seed) ^ ROOT_NOISE_STREAM) & 0xFFFFFFFFFFFFFFFF, gids, turn)
    return mix64(gk[:, None] ^ (np.arange(A, dtype=U64) + U64(1))[None, :])


def log_gamma_sample(alpha, key, dtype=None):
    """csrc/rng.hpp root_noise_log_gamma on a uint64 key array -> (log g, margin, t): log of the Gamma(alpha) draw
    per key, the draw's acceptance margin (float64), and t [rounds run, *key.shape] = log u - rhs of every evaluated
    comparison (nan: the draw had accepted before that round, or v <= 0 in it)."""
    T = _dtype(dtype)
    key = np.asarray(key, U64)
    al = T(np.float32(alpha))
    a = al + T(1) if al < T(1) else al
    d = a - T(1) / T(3)
    c = T(1) / np.sqrt(T(9) * d)
    two_pi = T(np.float32(2.0 * np.pi)) if T is np.float32 else T(2.0 * np.pi)
    tiny = T(TINY)
    logg = np.full(key.shape, np.log(d), T)           # no round accepts: g = d
    active = np.ones(key.shape, bool)
    margin = np.full(key.shape, np.inf)
    ts = []
    for it in range(ROUNDS):
        if not active.any():
            break
        u1 = np.maximum(u24(mix64(key ^ U64(4 * it + 1)).reshape(key.shape), T), tiny)
        u2 = u24(mix64(key ^ U64(4 * it + 2)).reshape(key.shape), T)
        x = np.sqrt(T(-2) * np.log(u1)) * np.cos(two_pi * u2)
        v1 = T(1) + c * x
        pos = v1 > T(0)
        v = v1 * v1 * v1
        u = np.maximum(u24(mix64(key ^ U64(4 * it + 3)).reshape(key.shape), T), tiny)
        vs = np.where(pos, v, T(1))
        rhs = T(0.5) * x * x + d - d * vs + d * np.log(vs)
        t = np.log(u) - rhs
        assert t.dtype == T
        acc = active & pos & (t < T(0))
        m = np.where(pos, np.minimum(np.abs(t), np.abs(v1)), np.abs(v1)).astype(np.float64)
        margin = np.where(active, np.minimum(margin, m), margin)
        ts.append(np.where(active & pos, t, T(np.nan)))
        logg = np.where(acc, np.log(d * vs), logg)
        active &= ~acc
    if al < T(1):
        ub = np.maximum(u24(mix64(key ^ U64(BOOST_STREAM)).reshape(key.shape), T), tiny)
        logg = logg + np.log(ub) / al
    assert logg.dtype == T
    return logg, margin, np.stack(ts)


def _row_sum(e):
    """The device's order of a row sum: row_sum24 (csrc/tree.hpp) for 24 actions, the xor butterfly of row_sum
    (csrc/nn.hpp) for a power of two, the plain sum otherwise."""
    A = e.shape[-1]
    if A == 24:
        r = (e[..., 0:8] + e[..., 8:16]) + e[..., 16:24]
    elif A & (A - 1) == 0:
        r = e
    else:
        return e.sum(-1, keepdims=True, dtype=e.dtype)
    while r.shape[-1] > 1:
        r = r[..., 0::2] + r[..., 1::2]
    return r


def normalise(logg):
    """The root blocks' row normalisation: softmax of the row's log-gammas [n, A]."""
    z = logg - logg.max(-1, keepdims=True)
    e = np.exp(z)
    out = e / _row_sum(e)
    assert out.dtype == logg.dtype
    return out


def root_noise(seed, gids, turn, alpha, A, dtype=None):
    """The device's Dirichlet(alpha) root noise of games `gids` at `turn` (one int or one per game) ->
    dict(noise [n, A], gamma [n, A] = exp(log g), logg, margin [n, A] float64, t [rounds, n, A])."""
    T = _dtype(dtype)
    logg, margin, t = log_gamma_sample(alpha, root_noise_keys(seed, gids, turn, A), T)
    with np.errstate(under="ignore"):
        return {"noise": normalise(logg), "gamma": np.exp(logg), "logg": logg, "margin": margin, "t": t}


def dirichlet(seed, gids, turn, alpha=0.3, A=4):
    """The float32 restatement's noise [n, A]: what the oracle searches are fed for the device's draw."""
    return root_noise(seed, gids, turn, alpha, A, np.float32)["noise"]
