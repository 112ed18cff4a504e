"""The on-device Dirichlet root noise (csrc/rng.hpp root_noise_log_gamma, read out by muz_root_noise_diag) against the
float64 run of its NumPy restatement (oracle/root_noise.py) (GPU).

Ruler, excused draws and cases: tests/_root_noise.py.  The restatement itself is checked against the Gamma and
Dirichlet distributions in tests/test_root_noise_oracle.py, on the same seeds."""
import numpy as np
import pytest

from tests import _root_noise as H
from tests._parity import log

pytestmark = pytest.mark.gpu

MUZ_E_INVALID, MUZ_E_UNSUPPORTED = 10001, 10002


def _call(ref, n, gids="ref", guard=2):
    g = (None if ref.gids is None else ref.gids[:n]) if isinstance(gids, str) else gids
    rc, gamma, noise = H.device_noise(ref.seed, ref.turn, g, ref.alpha, ref.A, n, guard)
    assert rc == 0, rc
    assert np.isnan(gamma[n:]).all() and np.isnan(noise[n:]).all(), "a guard row was written"
    assert np.isfinite(gamma[:n]).all() and np.isfinite(noise[:n]).all(), "a row was left unwritten"
    return gamma, noise


@pytest.mark.parametrize("alpha", H.ALPHAS)
@pytest.mark.parametrize("A", H.WIDTHS)
def test_root_noise_matches_float64(cuda, A, alpha):
    """Every key case at every count on the ruler; a row's bits depend on (seed, game, turn) only."""
    refs = H.reference(A, alpha)
    bad = []
    full = {}
    for name, ref in refs.items():
        assert ref.excused_fraction() <= H.MAX_EXCUSED
        full[name] = _call(ref, ref.n)
        bad += H.ruler(f"A={A} alpha={alpha} {name} (THR {ref.thr:.2e})", ref, *full[name], ref.n)
        assert np.abs(full[name][1][:ref.n].sum(1, dtype=np.float64) - 1.0).max() <= A * 2.0 ** -23
    # the smaller counts: leading rows of every key case, bit for bit the full call's rows, and on the ruler themselves
    for name, ref in refs.items():
        for n in H.COUNTS:
            gamma, noise = _call(ref, n)
            assert np.array_equal(gamma[:n], full[name][0][:n]) and np.array_equal(noise[:n], full[name][1][:n]), (name, n)
            if name == "plain":
                bad += H.ruler(f"A={A} alpha={alpha} {name}", ref, gamma, noise, n)
    # a row alone and the rows reversed, through game_id
    ref = refs["plain"]
    for k in (0, 5, 16, 4095):
        gamma, noise = _call(ref, 1, gids=np.array([k], np.int32))
        assert np.array_equal(gamma[0], full["plain"][0][k]) and np.array_equal(noise[0], full["plain"][1][k]), k
    for name in ("perm", "edge"):
        ref = refs[name]
        gamma, noise = _call(ref, ref.n, gids=ref.gids[::-1].copy())
        assert np.array_equal(gamma[:ref.n][::-1], full[name][0][:ref.n]), name
        assert np.array_equal(noise[:ref.n][::-1], full[name][1][:ref.n]), name
    # game_id null is the identity
    ident, _ = _call(refs["plain"], 33, gids=np.arange(33, dtype=np.int32))
    assert np.array_equal(ident[:33], full["plain"][0][:33])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("A", H.WIDTHS)
def test_root_noise_small_alpha(cuda, A):
    """alpha = 0.03 on games whose four gammas all underflow in float32 (and 300 ordinary ones): every noise row is
    finite, sums to 1 and follows the float64 restatement, which does not underflow.  (The raw gammas underflow by
    construction; the searches never form them.)"""
    dead, gids = H.small_alpha_games()
    ref = H.small_alpha_reference(A)
    assert ref.excused_fraction() <= H.MAX_EXCUSED
    gamma, noise = _call(ref, ref.n)
    if A == 4:
        assert (gamma[:len(dead)] < np.finfo(np.float32).tiny).all()
    bad = H.ruler(f"A={A} alpha={H.SMALL_ALPHA} underflowing rows {len(dead)}", ref, gamma, noise, ref.n,
                  check_gamma=False)
    keep = ~ref.excused
    e32 = H._abs_err(ref.r32["noise"][keep], ref.r64["noise"][keep])
    dsum = float(np.abs(noise[:ref.n][keep].sum(1, dtype=np.float64) - 1.0).max())
    log(f"root noise A={A} alpha={H.SMALL_ALPHA}: THR {ref.thr:.2e}, max |row sum - 1| {dsum:.2e}")
    assert dsum <= max(H.FACTOR * e32, A * 2.0 ** -23)
    assert not bad, "\n".join(bad)


def test_root_noise_refusals(cuda):
    """n = 0 launches nothing; a null output or a width other than 4 or 24 is refused before any launch."""
    rc, gamma, noise = H.device_noise(1, 0, None, 0.3, 4, 0, guard=3)
    assert rc == 0 and np.isnan(gamma).all() and np.isnan(noise).all()
    for kw in (dict(gamma_null=True), dict(noise_null=True)):
        rc, gamma, noise = H.device_noise(1, 0, None, 0.3, 4, 17, **kw)
        assert rc == MUZ_E_INVALID and np.isnan(gamma).all() and np.isnan(noise).all()
    for A in (3, 5, 6, 23, 25, 32):
        rc, gamma, noise = H.device_noise(1, 0, None, 0.3, A, 17)
        assert rc == MUZ_E_UNSUPPORTED and np.isnan(gamma).all() and np.isnan(noise).all(), A
    for alpha in (0.0, -0.3, float("nan")):
        rc, gamma, noise = H.device_noise(1, 0, None, alpha, 4, 17)
        assert rc == MUZ_E_UNSUPPORTED and np.isnan(gamma).all(), alpha
    rc, _, _ = H.device_noise(1, 0, None, 0.3, 4, -1, guard=4)
    assert rc == MUZ_E_INVALID
