"""Shared helpers of tests/test_root_noise_oracle.py (CPU) and tests/test_gpu_root_noise.py (GPU): the cases, the
float64 / float32 references of oracle/root_noise.py, the excused draws and the ruler (test helper, not a test module).

The ruler is tests/_nets64.py's, with its two constants: the device may sit no further from the float64 restatement
than max(3 x the float32 restatement's own worst distance over the same rows, 4 fp32 ulps) -- absolute on the
normalised noise (values in [0, 1]), relative on the raw gammas (they span 1e-19 to 10).

Excused draws.  A draw whose float64 acceptance margin (oracle/root_noise.py) is below THR may differ wholesale -- a
comparison of the sampler went the other way -- so its row is left out of the ruler and counted; at most 1 % of a
reference's rows may be left out (tests/test_root_noise_oracle.py asserts it on the reference alone, the GPU tests
again).  THR = 8 x the largest |t32 - t64| over the reference's own draws, t = log u - rhs of a round in the float32 and in
the float64 run, taken over the comparisons with |t64| <= 1.  Without that band the largest difference is set by
rounds whose v = (1 + c x)^3 is nearly 0: there d log v amplifies the last ulp of 1 + c x a thousandfold (1.2e-3 over
4096 x 24 draws, against 3e-6 inside the band) while t itself is tens of units away from a flip; a threshold of 8 x
that excuses 29 % of the 24-action rows on the reference alone.  The band only removes comparisons that no rounding can
flip, and the threshold it gives is never larger than the unrestricted one, so no draw is excused that the
unrestricted rule would not excuse."""
import ctypes
import functools

import numpy as np

from oracle import root_noise as RN
from tests._parity import log

ULP_FLOOR = 4 * 2.0 ** -23
FACTOR = 3.0
THR_FACTOR = 8.0
T_BAND = 1.0
MAX_EXCUSED = 0.01
ALPHAS = (0.3, 1.0, 2.5)
WIDTHS = (4, 24)
COUNTS = (1, 15, 16, 17, 33)      # around the searches' 16-row workgroups
BIG = 4096
SEED_HI = 2 ** 63 + 0x1234567     # a seed with the top bit set
SMALL_ALPHA = 0.03
SMALL_SEED, SMALL_TURN, SMALL_SCAN, SMALL_ORDINARY = 99, 3, 65536, 300


def key_cases():
    """name -> (seed, turn, game_id or None, rows).  Every key case has BIG rows, and the smaller counts are leading
    rows of these calls.  The ruler's yardstick is a maximum over the call's draws, so it needs enough of them: a
    gamma is exp(log g) with |log g| up to 44 at alpha 0.3, one rounding of log g moves it by up to 1.9e-6 relative,
    and which draw takes the worst rounding differs between the device's libm and NumPy's.  Over 4096 rows the float32
    run's worst relative gamma error is 3.8e-6 and the device's 4.1e-6; over the 33 x 4 draws these key cases first
    had, the float32 run's worst was 0.96e-6 and 1.03e-6, and the device's 2.90e-6 on the first set was 3.02x its
    yardstick while 1.54e-6 on the second was 1.49x."""
    rng = np.random.default_rng(5)
    perm = rng.permutation(BIG).astype(np.int32)
    edge = np.concatenate([[0, 2 ** 31 - 1], rng.integers(1, 2 ** 31 - 1, BIG - 2)]).astype(np.int32)
    return {"plain": (1234, 7, None, BIG), "perm": (0, 0, perm, BIG), "edge": (SEED_HI, 65535, edge, BIG)}


def threshold(pairs):
    """THR over (float32 run, float64 run) pairs of oracle.root_noise.root_noise."""
    worst = 0.0
    for r32, r64 in pairs:
        k = min(len(r32["t"]), len(r64["t"]))
        t32, t64 = r32["t"][:k].astype(np.float64), r64["t"][:k]
        both = np.isfinite(t32) & np.isfinite(t64)
        both[both] &= np.abs(t64[both]) <= T_BAND
        if both.any():
            worst = max(worst, float(np.abs(t32 - t64)[both].max()))
    return THR_FACTOR * worst


class Ref:
    """One key case's rows in both precisions, THR over its draws and the rows THR excuses."""

    def __init__(self, seed, turn, gids, n, alpha, A):
        self.seed, self.turn, self.gids, self.n, self.alpha, self.A = seed, turn, gids, n, alpha, A
        g = np.arange(n) if gids is None else gids
        self.r64 = RN.root_noise(seed, g, turn, alpha, A, np.float64)
        self.r32 = RN.root_noise(seed, g, turn, alpha, A, np.float32)
        self.thr = threshold([(self.r32, self.r64)])
        self.excused = (self.r64["margin"] < self.thr).any(1)

    def excused_fraction(self):
        return float(self.excused.mean())


@functools.lru_cache(maxsize=None)
def reference(A, alpha):
    """The key cases' references of one (A, alpha) -> {name: Ref}."""
    return {k: Ref(seed, turn, gids, n, alpha, A) for k, (seed, turn, gids, n) in key_cases().items()}


@functools.lru_cache(maxsize=None)
def small_alpha_games():
    """Game ids for the alpha = 0.03 case: the games of 0..65535 (seed 99, turn 3) whose four float32 gammas are all
    below the smallest normal float32 -- the rows a linear-space g * u^(1/alpha) normalises as 0 / 0 -- then 300
    ordinary ones."""
    logg = RN.root_noise(SMALL_SEED, np.arange(SMALL_SCAN), SMALL_TURN, SMALL_ALPHA, 4, np.float32)["logg"]
    dead = np.flatnonzero((logg < np.log(np.float32(RN.TINY))).all(1))
    return dead.astype(np.int32), np.concatenate([dead, np.arange(SMALL_ORDINARY)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def small_alpha_reference(A):
    _, gids = small_alpha_games()
    return Ref(SMALL_SEED, SMALL_TURN, gids, len(gids), SMALL_ALPHA, A)


# ------------------------------------------------------------------------------------------ the device
def device_noise(seed, turn, gids, alpha, A, n, guard=2, gamma_null=False, noise_null=False):
    """muz_root_noise_diag on n rows -> (return code, gamma [n + guard, A], noise [n + guard, A]) as NumPy arrays;
    the buffers are NaN-filled before the call, so the guard rows and every unwritten value stay NaN."""
    import torch
    from exploring_muzero_on_dog_amd import lib as L
    lib = L.load()
    g = torch.full((n + guard, A), float("nan"), dtype=torch.float32, device="cuda")
    z = torch.full((n + guard, A), float("nan"), dtype=torch.float32, device="cuda")
    gi = None if gids is None else torch.from_numpy(np.ascontiguousarray(gids, np.int32)).cuda()
    rc = lib.muz_root_noise_diag(ctypes.c_uint64(seed), int(turn), L.ptr(gi), float(alpha), int(A), int(n),
                                 L.ptr(None if gamma_null else g), L.ptr(None if noise_null else z), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, g.cpu().numpy(), z.cpu().numpy()


# ------------------------------------------------------------------------------------------ the ruler
def _abs_err(x, ref64):
    return float(np.abs(np.asarray(x, np.float64) - ref64).max()) if len(ref64) else 0.0


def _rel_err(x, ref64):
    return float((np.abs(np.asarray(x, np.float64) - ref64) / np.abs(ref64)).max()) if len(ref64) else 0.0


def ruler(label, ref, dev_gamma, dev_noise, n, check_gamma=True):
    """The ruler on the first n rows of one reference.  Logs one line and returns the violations (empty: met)."""
    keep = ~ref.excused[:n]
    bad, parts = [], []
    outs = [("noise", _abs_err, dev_noise)] + ([("gamma", _rel_err, dev_gamma)] if check_gamma else [])
    for name, fn, dev in outs:
        d = np.asarray(dev)[:n][keep]
        if not np.isfinite(d).all():
            bad.append(f"{label} n={n} {name}: not finite")
            continue
        r64 = ref.r64[name][:n][keep]
        e_dev, e_32 = fn(d, r64), fn(ref.r32[name][:n][keep], r64)
        bound = max(FACTOR * e_32, ULP_FLOOR)
        parts.append(f"{name} dev {e_dev:.2e} f32 {e_32:.2e} ratio {e_dev / max(e_32, 1e-30):.2f}")
        if e_dev > bound:
            bad.append(f"{label} n={n} {name}: device {e_dev:.3e} > bound {bound:.3e} (fp32 {e_32:.3e})")
    log(f"root noise {label} n={n}: " + "; ".join(parts) + f"; rows excused {int((~keep).sum())} of {n}")
    return bad
