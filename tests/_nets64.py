"""Shared helpers of tests/test_gpu_nets_edges.py: the inference network kernels against the float64 run of the
NumPy restatements (oracle.nets.precision), per game and per C entry point (test helper, not a test module).

The ruler (tests/test_gpu_learner_oracle.py's, with its two constants): per output tensor
    err(x) = max|x - ref64| / max(1, max|ref64|)
and the device may sit no further from float64 than
    max(3 x max(err(fp32 restatement of that output), the call's worst output's err(fp32)), ULP_FLOOR = 4 x 2^-23).

Every device call goes through the C ABI with raw pointers (lib.load()), so the tests own every buffer: the outputs
can carry guard rows and the scratch can be pre-filled and sized to the byte.

Positions are real encoded boards: seeded random play of the oracle environments (the loops of
tests.test_gpu_nets.random_obs / tests.test_gpu_stochastic.random_classic_states, which return one position per game
played and would need 577 games; here a handful of games give every ply's position) and tests.test_gpu_dog_muzero.
dog_states for DOG."""
import ctypes

import numpy as np
import torch

from oracle import classic_madn as cm
from oracle import classic_nets as CN
from oracle import detmadn as dm
from oracle import dog_muzero as DM
from oracle import nets as ON
from tests._detmadn_util import random_play_transitions
from tests._parity import log

ULP_FLOOR = 4 * 2.0 ** -23
FACTOR = 3.0
LAT = 256
N_ROOT = 577      # one oracle call per (game, weight set); smaller counts are its leading rows (rows are independent)
N_REC = 33
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ------------------------------------------------------------------------------------------ positions
def det_obs(rule_set, n, seed, games):
    """n distinct-ply positions of `games` seeded random det-MADN games (every ply of every game is a candidate)."""
    envs = []
    for _, batch in random_play_transitions(rule_set, games, seed, max_plies=400, p_illegal=0.0):
        envs.extend(e for _, e, _, _ in batch)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(envs), size=n, replace=False)
    return np.stack([dm.encode_board(envs[i]) for i in pick]).astype(np.float32)


def classic_obs(n, seed, games=12, plies=120, P=4):
    """n positions (after the die throw) of seeded random classic-MADN play."""
    rng = np.random.default_rng(seed)
    envs = [cm.env_reset(num_players=P, **cm.SELFPLAY_RULES) for _ in range(games)]
    out = []
    for _ in range(plies):
        nxt = []
        for e in envs:
            if e.done:
                e = cm.env_reset(num_players=P, **cm.SELFPLAY_RULES)
            e = cm.throw_die(e, float(rng.random()))
            out.append(e)
            va = cm.valid_action(e)
            nxt.append(cm.env_step(e, int(rng.choice(np.flatnonzero(va))))[0] if va.any() else cm.no_step(e)[0])
        envs = nxt
    pick = rng.choice(len(out), size=n, replace=False)
    return np.stack([cm.encode_board(out[i]) for i in pick]).astype(np.float32)


def dog_obs(n, seed):
    from tests.test_gpu_dog_muzero import dog_states
    _, envs = dog_states("selfplay_4p_teams", n, 0, seed)
    return np.stack([DM.encode_board(e) for e in envs]).astype(np.float32)


# ------------------------------------------------------------------------------------------ games / entry points
class Entry:
    """One C entry point.  outs: (name, floats per row) in the C argument order; ora(params, idx, x) -> the same
    outputs in that order; A: the width of its one-hot index (None: root, no index)."""

    def __init__(self, cfn, outs, ora, A=None, src=None):
        self.cfn, self.outs, self.ora, self.A, self.src = cfn, outs, ora, A, src


def _det_like(root_c, rec_c, A, mod):
    root = Entry(root_c, (("logits", A), ("value", 1), ("latent", LAT)),
                 lambda p, idx, x: mod.root_inference(p, x))
    rec = Entry(rec_c, (("reward", 1), ("discount", 1), ("logits", A), ("value", 1), ("latent", LAT)),
                lambda p, idx, x: mod.recurrent_inference(p, idx, x), A=A, src=("root", "latent"))
    return {"root": root, "recurrent": rec}


def _classic_entries():
    def dec(p, idx, x):
        cl, v, after, r, d = CN.decision_recurrent(p, idx, x)
        return after, r, d, cl, v

    def cha(p, idx, x):
        lg, v, nxt = CN.chance_recurrent(p, idx, x)
        return nxt, lg, v
    return {"root": Entry("muz_classic_nets_root", (("logits", 4), ("value", 1), ("latent", LAT)),
                          lambda p, idx, x: CN.root_inference(p, x)),
            "decision": Entry("muz_classic_nets_decision", (("afterstate", LAT), ("reward", 1), ("discount", 1),
                                                            ("chance_logits", 6), ("value", 1)), dec, A=4,
                              src=("root", "latent")),
            "chance": Entry("muz_classic_nets_chance", (("latent", LAT), ("logits", 4), ("value", 1)), cha, A=6,
                            src=("decision", "afterstate"))}


class Game:
    def __init__(self, name, C, entries, init, make_net, obs, degenerate_latent):
        self.name, self.C, self.entries, self.init, self.make_net, self.obs = name, C, entries, init, make_net, obs
        self.degenerate_latent = degenerate_latent   # what weight set 3's embedding must be, exactly


def _det_net(C):
    def make(params):
        from exploring_muzero_on_dog_amd import nets as N
        return N.DeviceNet(params, C)
    return make


def _classic_net(params):
    from exploring_muzero_on_dog_amd import stochastic as S
    return S.DeviceClassicNet(params, cm.num_channels(4))


def _dog_net(params):
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    return MD.DeviceDogNet(params)


DEG_BIAS = 0.25    # weight set 3's constant Dense_4 bias: a power of two, so every partial row sum is exact

GAMES = {
    "det2": Game("det2", dm.num_channels(2), _det_like("muz_nets_root", "muz_nets_recurrent", 24, ON),
                 lambda seed: ON.init_params(dm.num_channels(2), seed=seed, randomize_affine=True),
                 _det_net(dm.num_channels(2)), lambda n: det_obs("selfplay_2p", n, 41, 8), "zero"),
    "det4": Game("det4", dm.num_channels(4), _det_like("muz_nets_root", "muz_nets_recurrent", 24, ON),
                 lambda seed: ON.init_params(dm.num_channels(4), seed=seed, randomize_affine=True),
                 _det_net(dm.num_channels(4)), lambda n: det_obs("selfplay_4p_teams", n, 42, 3), "zero"),
    "classic": Game("classic", cm.num_channels(4), _classic_entries(),
                    lambda seed: CN.init_params(cm.num_channels(4), seed=seed, randomize_affine=True),
                    _classic_net, lambda n: classic_obs(n, 43), "zero"),
    "dog": Game("dog", DM.NUM_CHANNELS, _det_like("muz_dog_nets_root", "muz_dog_nets_recurrent", DM.NUM_ACTIONS, DM),
                lambda seed: DM.init_params(seed=seed, randomize_affine=True), _dog_net,
                lambda n: dog_obs(n, 44), "ln7_bias"),
}
SEEDS = {"det2": 101, "det4": 102, "classic": 103, "dog": 104}   # none of the older tests' (5, 11, 20, 21, 31)
ROOT_COUNTS = {"det2": (1, 2, 15, 16, 17, 63, 64, 65, 129, 513, 577), "det4": (1, 2, 15, 16, 17, 63, 64, 65, 129, 513, 577),
               "classic": (1, 17, 65, 513), "dog": (1, 17, 65, 513)}
REC_COUNTS = (1, 15, 16, 17, 33)


def weight_set(game, ws):
    """1: seeded init with non-trivial affine parameters; 2: the same with every kernel tripled (trained-like
    magnitudes: logits of several units, a saturating value head); 3: the representation's last Dense zeroed with a
    constant bias, so its min-max range / LayerNorm_7 variance is exactly 0."""
    p = GAMES[game].init(SEEDS[game])
    if ws == 2:
        p = {k: (v * np.float32(3.0) if k.endswith("/kernel") else v) for k, v in p.items()}
    elif ws == 3:
        p = dict(p)
        p["representation/Dense_4/kernel"] = np.zeros_like(p["representation/Dense_4/kernel"])
        p["representation/Dense_4/bias"] = np.full_like(p["representation/Dense_4/bias"], DEG_BIAS)
    return p


def indices(A, n, seed):
    """n in-range one-hot indices"""
    return np.random.default_rng(seed).integers(0, A, n).astype(np.int32)


def special_indices(A):
    return np.array([-2, -1, 0, A - 1, A, A + 1, INT_MAX, INT_MIN], np.int64).astype(np.int32)


# ------------------------------------------------------------------------------------------ the oracle, both precisions
def oracle_chain(game, params, obs, idx, latent_override=None):
    """Every entry point of the game on obs (root) and on the float64 run's own outputs cast to fp32 (the recurrent
    entry points' inputs, first len(idx[e]) rows; latent_override replaces them), in float64 and in fp32.
    -> inputs {entry: (idx, x)}, ref64 / ref32 {entry: {output: array}}."""
    g = GAMES[game]
    inputs, ref64, ref32 = {}, {}, {}
    for name, e in g.entries.items():
        if e.src is None:
            i, x = None, obs
        else:
            i = idx[name]
            x = ref64[e.src[0]][e.src[1]][:len(i)].astype(np.float32) if latent_override is None else latent_override
        inputs[name] = (i, x)
        with ON.precision(np.float64):
            r64 = e.ora(params, i, x)
        r32 = e.ora(params, i, x)
        assert all(a.dtype == np.float64 for a in r64) and all(a.dtype == np.float32 for a in r32)
        ref64[name] = {o[0]: a for o, a in zip(e.outs, r64)}
        ref32[name] = {o[0]: a for o, a in zip(e.outs, r32)}
    return inputs, ref64, ref32


# ------------------------------------------------------------------------------------------ the device, raw pointers
def _L():
    from exploring_muzero_on_dog_amd import lib as L
    return L


def scratch_bytes(n):
    return int(_L().load().muz_nets_root_scratch_bytes(n))


def call(game, entry, net, idx, x, n=None, guard=0, scratch_extra_rows=0, scratch_short=0, fill=float("nan")):
    """One call of the C entry point on the first n rows of (idx, x) (device tensors).  Output buffers have n + guard
    rows, the scratch (root) muz_nets_root_scratch_bytes(n) bytes + scratch_extra_rows rows - scratch_short bytes; all
    pre-filled with `fill`.  -> (return code, {output: tensor [n + guard, width]}, scratch)."""
    L = _L()
    lib = L.load()
    e = GAMES[game].entries[entry]
    n = len(x) if n is None else n
    outs = {k: torch.full((n + guard, w), fill, dtype=torch.float32, device="cuda") for k, w in e.outs}
    optrs = [L.ptr(outs[k]) for k, _ in e.outs]
    fn = getattr(lib, e.cfn)
    scratch = None
    if e.src is None:
        row_bytes = scratch_bytes(16) // 16
        nb = scratch_bytes(n) + scratch_extra_rows * row_bytes
        scratch = torch.full((max(nb, 4) // 4,), fill, dtype=torch.float32, device="cuda")
        rc = fn(net.w, L.ptr(x), n, L.ptr(scratch), ctypes.c_int64(nb - scratch_short), *optrs, L.stream_ptr())
    else:
        rc = fn(net.w, L.ptr(idx), L.ptr(x), n, *optrs, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, outs, scratch


def run(game, entry, net, idx, x, n=None):
    """The plain call: exact-size buffers, NaN pre-filled (a row the kernel leaves unwritten fails every comparison)."""
    rc, outs, _ = call(game, entry, net, idx, x, n)
    assert rc == 0, (game, entry, rc)
    return outs


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ the ruler
def err(x, ref64):
    ref64 = np.asarray(ref64, np.float64).reshape(len(ref64), -1)
    x = np.asarray(x, np.float64).reshape(ref64.shape)
    return float(np.abs(x - ref64).max()) / max(1.0, float(np.abs(ref64).max()))


def ruler(label, e, dev, ref64, ref32, n, named=()):
    """The ruler on one call's first n rows.  Logs one line (device error, fp32 error, ratio per output) and returns
    the list of violations (empty: the call meets the ruler).  named: outputs of this case listed in the test's NAMED
    table -- their yardstick is the fp32 restatement's deviation of that output over ALL rows the oracle ran for the
    weight set instead of the call's n rows (same factor, same floor)."""
    e_dev, e_32 = {}, {}
    for k, _ in e.outs:
        d = dev[k][:n].detach().cpu().numpy()
        assert np.isfinite(d).all(), (label, k, "not finite")
        e_dev[k] = err(d, ref64[k][:n])
        e_32[k] = err(ref32[k][:n], ref64[k][:n])
    worst32 = max(e_32.values())
    bad, parts = [], []
    for k, _ in e.outs:
        bound = max(FACTOR * max(e_32[k], worst32), ULP_FLOOR)
        parts.append(f"{k} dev {e_dev[k]:.2e} f32 {e_32[k]:.2e} ratio {e_dev[k] / max(e_32[k], 1e-30):.2f}")
        if e_dev[k] > bound and k in named:
            all32 = err(ref32[k], ref64[k])
            parts[-1] += (f" (NAMED: above 3x the call's worst fp32 {worst32:.2e}; fp32 over the oracle's "
                          f"{len(ref64[k])} rows {all32:.2e}, ratio {e_dev[k] / max(all32, 1e-30):.2f})")
            bound = max(FACTOR * all32, ULP_FLOOR)
        elif k in named:
            parts[-1] += " (NAMED, but within the plain ruler)"
        if e_dev[k] > bound:
            bad.append(f"{label} n={n} {k}: device {e_dev[k]:.3e} > bound {bound:.3e} (fp32 {e_32[k]:.3e}, call's "
                       f"worst fp32 {worst32:.3e})")
    log(f"nets64 {label} n={n}: " + "; ".join(parts) + f"; worst dev / call's worst f32 "
        f"{max(e_dev.values()) / max(worst32, 1e-30):.2f}")
    return bad
