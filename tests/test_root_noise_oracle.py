"""oracle/root_noise.py (the restatement of the on-device Dirichlet root noise) against the textbook distributions
(CPU), so that the GPU tests compare the kernels with something that is right and not with a copy of themselves.

Fixed seeds.  Every bound is a number of standard errors derived from the sample size: Z = 5 (a two-sided normal tail
of 6e-7 per comparison; the file makes a few hundred).  The Kolmogorov-Smirnov bound is the 1 % point 1.63 of the
Kolmogorov distribution for sqrt(N) D."""
import numpy as np
import pytest
import torch

from oracle import nets as ON
from oracle import root_noise as RN
from oracle import selfplay as OS
from tests import _root_noise as H

Z = 5.0
KS_1PCT = 1.63
N_GAMES = 4096
SEED, TURN = 1234, 7


def _draw(alpha, A, dtype=np.float64, seed=SEED, turn=TURN, gids=None):
    return RN.root_noise(seed, np.arange(N_GAMES) if gids is None else gids, turn, alpha, A, dtype)


def test_hash_matches_the_scalar_restatement():
    """mix64 / game_key / u24 vectorised == the Python-int restatement the other oracles use (oracle/selfplay.py)."""
    rng = np.random.default_rng(0)
    xs = [0, 1, 2 ** 63, 2 ** 64 - 1] + [int(v) for v in rng.integers(0, 2 ** 63, 50)]
    assert [int(v) for v in RN.mix64(np.array(xs, np.uint64))] == [OS._mix64(v) for v in xs]
    for seed, gid, turn in ((0, 0, 0), (1234, 5, 7), (H.SEED_HI, 2 ** 31 - 1, 65535), (99, -1, 3)):
        want = (seed & OS.M64) ^ OS._mix64(((gid & 0xFFFFFFFF) << 32) | (turn & 0xFFFFFFFF))
        assert int(RN.game_key(seed, gid, turn)[0]) == want
        k = int(RN.root_noise_keys(seed, [gid], turn, 4)[0, 2])
        assert k == OS._mix64(((seed ^ RN.ROOT_NOISE_STREAM) & OS.M64)
                              ^ OS._mix64(((gid & 0xFFFFFFFF) << 32) | (turn & 0xFFFFFFFF)) ^ 3)
    h = np.array([0, 1 << 40, (1 << 64) - 1], np.uint64)
    for T in (np.float32, np.float64):
        assert np.array_equal(RN.u24(h, T), np.array([0.0, 2.0 ** -24, 1.0 - 2.0 ** -24], T))


def test_precision_switch():
    a = RN.root_noise(SEED, np.arange(8), TURN, 0.3, 4)
    with ON.precision(np.float64):
        b = RN.root_noise(SEED, np.arange(8), TURN, 0.3, 4)
    assert a["noise"].dtype == np.float32 and a["gamma"].dtype == np.float32
    assert b["noise"].dtype == np.float64 and b["logg"].dtype == np.float64
    assert np.array_equal(a["noise"], RN.dirichlet(SEED, np.arange(8), TURN, 0.3, 4))


def _ks(x, alpha):
    """sqrt(N) D of the sample x against the Gamma(alpha) distribution function (torch.special.gammainc, float64)."""
    x = np.sort(np.asarray(x, np.float64).ravel())
    N = x.size
    cdf = torch.special.gammainc(torch.tensor(float(np.float32(alpha)), dtype=torch.float64),
                                 torch.from_numpy(x)).numpy()
    i = np.arange(1, N + 1)
    return float(np.sqrt(N) * max((i / N - cdf).max(), (cdf - (i - 1) / N).max()))


@pytest.mark.parametrize("alpha", H.ALPHAS)
@pytest.mark.parametrize("A", H.WIDTHS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gamma_marginals_kolmogorov_smirnov(alpha, A, dtype):
    ks = _ks(_draw(alpha, A, dtype)["gamma"], alpha)
    print(f"Gamma({alpha}) A={A} {np.dtype(dtype).name}: sqrt(N) D = {ks:.3f}")
    assert ks < KS_1PCT


def _beta_moments(a, b):
    """mean, variance and the variance of (X - mean)^2 of Beta(a, b), from its raw moments."""
    m = [1.0]
    for r in range(4):
        m.append(m[-1] * (a + r) / (a + b + r))
    mu = m[1]
    var = m[2] - mu ** 2
    m4 = m[4] - 4 * mu * m[3] + 6 * mu ** 2 * m[2] - 3 * mu ** 4
    return mu, var, m4 - var ** 2


@pytest.mark.parametrize("alpha", H.ALPHAS + (H.SMALL_ALPHA,))
@pytest.mark.parametrize("A", H.WIDTHS)
def test_dirichlet_rows_mean_and_variance(alpha, A):
    """A coordinate of Dirichlet(alpha, ..., alpha) is Beta(alpha, (A - 1) alpha): mean 1 / A, variance
    (A - 1) / (A^2 (A alpha + 1)).  The sample mean of N rows is within Z sqrt(var / N), the sample mean of
    (x - 1 / A)^2 within Z sqrt(Var[(X - 1 / A)^2] / N)."""
    x = _draw(alpha, A)["noise"]
    assert np.abs(x.sum(1) - 1.0).max() < 1e-12 and (x >= 0).all()
    al = float(np.float32(alpha))
    mu, var, var_sq = _beta_moments(al, (A - 1) * al)
    assert abs(mu - 1.0 / A) < 1e-12 and abs(var - (A - 1) / (A * A * (A * al + 1))) < 1e-12
    N = len(x)
    assert (np.abs(x.mean(0) - mu) < Z * np.sqrt(var / N)).all()
    assert (np.abs(((x - mu) ** 2).mean(0) - var) < Z * np.sqrt(var_sq / N)).all()


def _corr(x, y):
    return float(np.corrcoef(np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel())[0, 1])


@pytest.mark.parametrize("alpha", H.ALPHAS)
def test_draws_are_independent(alpha):
    """The gammas of two actions, two turns, two games and two seeds are uncorrelated: the sample correlation of N
    independent pairs has standard error 1 / sqrt(N).  (One key for every action gives a correlation of 1.)"""
    A = 4
    g = _draw(alpha, A)["gamma"]
    N = len(g)
    pairs = {f"actions {a} {b}": (g[:, a], g[:, b]) for a in range(A) for b in range(a + 1, A)}
    pairs["turns"] = (g, _draw(alpha, A, turn=TURN + 1)["gamma"])
    pairs["games"] = (g, _draw(alpha, A, gids=np.arange(N_GAMES) + 1)["gamma"])
    pairs["games far"] = (g, _draw(alpha, A, gids=np.arange(N_GAMES) + N_GAMES)["gamma"])
    pairs["seeds"] = (g, _draw(alpha, A, seed=SEED + 1)["gamma"])
    pairs["game / turn swapped"] = (_draw(alpha, A, turn=3, gids=np.full(N_GAMES, 5) + np.arange(N_GAMES))["gamma"],
                                    _draw(alpha, A, turn=5, gids=np.full(N_GAMES, 3) + np.arange(N_GAMES))["gamma"])
    for name, (x, y) in pairs.items():
        n = np.asarray(x).size
        r = _corr(x, y)
        assert abs(r) < Z / np.sqrt(n), (name, r, n)
        assert not np.array_equal(x, y), name
    assert N == N_GAMES


def test_margin_bounds_every_evaluated_comparison():
    """The margin of a draw is no larger than |log u - rhs| of any round the draw evaluated, and every draw accepted
    (its last evaluated t is negative) well inside the 32 rounds."""
    r = _draw(0.3, 24)
    t = r["t"]
    assert len(t) < RN.ROUNDS
    assert (r["margin"] <= np.nanmin(np.abs(t), axis=0)).all() and (r["margin"] > 0).all()
    last = np.array([t[np.flatnonzero(np.isfinite(t[:, i, j]))[-1], i, j] for i in range(64) for j in range(24)])
    assert (last < 0).all()


@pytest.mark.parametrize("alpha", H.ALPHAS)
@pytest.mark.parametrize("A", H.WIDTHS)
def test_excused_rows_stay_under_the_cap(alpha, A):
    """tests/test_gpu_root_noise.py's seeds, on the reference alone: at most 1 % of a key case's rows are excused, and
    the float32 run itself never differs wholesale from the float64 run on a row that is not excused."""
    for name, r in H.reference(A, alpha).items():
        print(f"A={A} alpha={alpha} {name}: THR {r.thr:.2e}, excused {int(r.excused.sum())} of {r.n} rows; "
              f"smallest float64 margin {r.r64['margin'].min():.2e}")
        assert 0 < r.thr < 1e-3
        assert r.excused_fraction() <= H.MAX_EXCUSED
        keep = ~r.excused
        assert H._abs_err(r.r32["noise"][keep], r.r64["noise"][keep]) < 1e-5
        assert H._rel_err(r.r32["gamma"][keep], r.r64["gamma"][keep]) < 1e-4
        if name == "plain":
            assert not r.excused[:H.COUNTS[-1]].any()      # the small counts compare every row


@pytest.mark.parametrize("A", H.WIDTHS)
def test_small_alpha_reference(A):
    """alpha = 0.03: the chosen games include rows whose four float32 gammas all underflow (a linear-space
    normalisation would divide 0 by 0 there); in log space the float32 restatement stays finite, sums to 1 and follows
    the float64 run."""
    dead, gids = H.small_alpha_games()
    assert len(dead) >= 1 and len(gids) <= 400
    r = H.small_alpha_reference(A)
    if A == 4:
        with np.errstate(under="ignore"):
            lin = np.exp(r.r32["logg"][:len(dead)])
        assert (lin < np.float32(RN.TINY)).all()
    assert r.excused_fraction() <= H.MAX_EXCUSED
    keep = ~r.excused
    n32 = r.r32["noise"][keep]
    assert np.isfinite(n32).all() and np.abs(n32.sum(1, dtype=np.float64) - 1.0).max() < 1e-6
    assert H._abs_err(n32, r.r64["noise"][keep]) < 1e-4


def test_selfplay_keys_are_game_and_step():
    """oracle/selfplay.py feeds play_batch_of_games_stochastic the noise of (seed, game, step)."""
    gids = np.array([3, 0, 7])
    want = RN.dirichlet(4242, gids, 11, 0.3, 4)
    assert np.array_equal(OS.root_dirichlet(4242, gids, 11), want)
    assert not np.array_equal(OS.root_dirichlet(4242, gids, 12), want)
