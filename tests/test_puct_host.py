"""PUCT muzero_policy search (csrc/puct_search.hip), everything that needs no GPU: the muz_puct_cfg layout (header vs
ctypes), the workspace it shares with the Gumbel search, muz_puct_search's refusals (argument checks come before any
launch, so they run on a host without a GPU), and properties of the NumPy restatement (tests/_mctx_muzero.py) on a
toy recurrent function."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import _mctx_muzero as PZ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 24


def _lib():
    from exploring_muzero_on_dog_amd import lib as L
    return L


def test_puct_cfg_layout_matches_header():
    """sizeof and every field offset of muz_puct_cfg, header (gcc) vs ctypes; the two qtransform constants."""
    L = _lib()
    fields = [f[0] for f in L.MuzPuctCfg._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"muz.h\"\nint main(){\n"
    src += 'printf("size %zu\\n", sizeof(muz_puct_cfg));\n'
    for f in fields:
        src += f'printf("{f} %zu\\n", offsetof(muz_puct_cfg, {f}));\n'
    src += 'printf("QT_MIN_MAX %d\\nQT_PARENT_SIBLINGS %d\\n", MUZ_QT_MIN_MAX, MUZ_QT_PARENT_SIBLINGS);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as fh:
            fh.write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True).stdout.split("\n")
                   if line)
    assert int(out["size"]) == ctypes.sizeof(L.MuzPuctCfg)
    for f in fields:
        assert int(out[f]) == getattr(L.MuzPuctCfg, f).offset, f
    assert fields == ["num_simulations", "max_depth", "qtransform", "min_value", "max_value", "dirichlet_fraction",
                      "dirichlet_alpha", "pb_c_init", "pb_c_base", "temperature", "turn", "seed"]
    assert int(out["QT_MIN_MAX"]) == L.MUZ_QT_MIN_MAX == 0
    assert int(out["QT_PARENT_SIBLINGS"]) == L.MUZ_QT_PARENT_SIBLINGS == 1


class _Call:
    """muz_puct_search with never-dereferenced dummy pointers: every case here must return before any launch."""

    def __init__(self):
        from exploring_muzero_on_dog_amd import mcts as M
        self.L = _lib()
        self.so = self.L.load()
        self.M = M
        self.w = self.L.MuzNetW()
        self.w.num_actions = A
        self.buf = (ctypes.c_char * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)

    def __call__(self, cfg, n=1, ws_bytes=1 << 40, w="net", null=None):
        P = [self.p] * 11    # root_logits, root_value, root_emb, legal, dirichlet, gumbel, game_id, ws, act, wts, val
        if null is not None:
            P[null] = None
        return self.so.muz_puct_search(ctypes.byref(self.w) if w == "net" else w,
                                       ctypes.byref(cfg) if cfg is not None else None, P[0], P[1], P[2], P[3], P[4],
                                       P[5], P[6], n, P[7], ws_bytes, P[8], P[9], P[10], None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_puct_workspace_is_the_gumbel_workspace(call):
    """muz_puct_search takes the Gumbel search's workspace (one SearchWorkspace serves both policies): at every
    (n, S) it refuses one byte less than muz_search_workspace_bytes as MUZ_E_INVALID and asks for no more (n = 0
    with an empty workspace is MUZ_OK)."""
    L, M = call.L, call.M
    for n in (1, 17, 4096):
        for S in (1, 50, 100):
            need = call.so.muz_search_workspace_bytes(n, ctypes.byref(M.make_cfg(S, S)))
            assert need == n * (S + 1) * 1792
            cfg = M.make_puct_cfg(S, min(S, 64))
            assert call(cfg, n=n, ws_bytes=need - 1) == L.MUZ_E_INVALID, (n, S)
            assert call(cfg, n=0, ws_bytes=0) == L.MUZ_OK


@pytest.mark.parametrize("change", [
    dict(num_simulations=0), dict(num_simulations=101), dict(max_depth=0), dict(max_depth=65), dict(qtransform=2),
    dict(qtransform=-1), dict(max_value=-1.0), dict(min_value=2.0), dict(dirichlet_fraction=-0.01),
    dict(dirichlet_fraction=1.01), dict(dirichlet_alpha=0.0), dict(dirichlet_alpha=-0.3), dict(pb_c_base=0.0),
    dict(pb_c_base=-1.0), dict(temperature=-0.5), dict(temperature=float("nan")), dict(num_actions=4)])
def test_puct_search_refuses_unsupported_configurations(call, change):
    L = call.L
    cfg = call.M.make_puct_cfg(50, 25)
    change = dict(change)
    call.w.num_actions = change.pop("num_actions", A)
    for k, v in change.items():
        setattr(cfg, k, v)
    try:
        assert call(cfg) == L.MUZ_E_UNSUPPORTED
    finally:
        call.w.num_actions = A


def test_puct_search_refuses_null_pointers(call):
    L = call.L
    cfg = call.M.make_puct_cfg(50, 25)
    assert call(cfg, w=None) == L.MUZ_E_INVALID
    assert call(None) == L.MUZ_E_INVALID
    assert call(cfg, n=-1) == L.MUZ_E_INVALID
    for i in (0, 1, 2, 3, 7, 8, 9, 10):       # dirichlet (4), gumbel (5) and game_id (6) may be null
        assert call(cfg, null=i) == L.MUZ_E_INVALID, i
    # an unsupported configuration is reported as such even with a null pointer beside it
    cfg.qtransform = 7
    assert call(cfg, null=0) == L.MUZ_E_UNSUPPORTED


def test_python_entry_points_refuse_unknown_names():
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    with pytest.raises(ValueError):
        M.make_puct_cfg(8, 4, qtransform="completed_by_mix_value")
    with pytest.raises(ValueError):
        M.muzero_mcts(None, None, None, 8, 4, 1.0, policy="alphazero")
    with pytest.raises(TypeError):
        M.muzero_mcts(None, None, None, 8, 4, 1.0, dirichlet_fraction=0.0)   # a PUCT keyword on the Gumbel path
    with pytest.raises(ValueError):
        EV._search_kwargs("mcts")
    assert EV._search_kwargs("gumbel") == {}
    assert EV._search_kwargs("puct") == {"policy": "puct", "dirichlet_fraction": 0.0}
    c = M.make_puct_cfg(50, 25, 0.5, seed=-1, turn=3)
    assert (c.qtransform, c.min_value, c.max_value, c.turn, c.seed) == (0, -1.0, 1.0, 3, (1 << 64) - 1)
    assert (c.dirichlet_fraction, c.temperature, c.pb_c_base) == (0.25, 0.5, 19652.0)
    assert abs(c.dirichlet_alpha - 0.3) < 1e-7 and c.pb_c_init == 1.25


# ---- the restatement on a toy recurrent function -------------------------------------------------------------------
LAT = 8


def toy_recurrent(params, action, emb):
    """A deterministic smooth stand-in for the networks: rewards / values in (-1, 1), discounts of either sign."""
    h = np.sin(1.7 * emb.sum(-1) + 0.61 * action + params).astype(np.float32)
    reward = (0.3 * np.sin(5.0 * h + 1.0)).astype(np.float32)
    discount = (0.9 * np.where(np.cos(3.0 * h) > 0, 1.0, -1.0)).astype(np.float32)
    prior = (2.0 * np.sin(np.outer(h, np.arange(1, A + 1)) + emb[:, :1])).astype(np.float32)
    value = (0.8 * np.cos(2.0 * h)).astype(np.float32)
    nxt = (0.5 * np.roll(emb, 1, -1) + 0.1 * h[:, None] + 0.01 * action[:, None]).astype(np.float32)
    return reward, discount, prior, value, nxt


def toy_inputs(B, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(B, A)).astype(np.float32)
    value = rng.uniform(-0.9, 0.9, B).astype(np.float32)
    emb = rng.uniform(0, 1, (B, LAT)).astype(np.float32)
    invalid = rng.random((B, A)) < 0.6
    invalid[np.arange(B), rng.integers(0, A, B)] = False       # at least one legal action
    invalid[0] = True
    invalid[0, 5] = False                                      # a game with a single legal action
    dirichlet = rng.dirichlet(np.full(A, 0.3), B).astype(np.float32)
    gumbel = rng.gumbel(size=(B, A)).astype(np.float32)
    return logits, value, emb, invalid, dirichlet, gumbel


@pytest.fixture(scope="module", params=[(PZ.QT_MIN_MAX, 1.0, 0.25), (PZ.QT_PARENT_SIBLINGS, 0.0, 0.0)],
                ids=["min_max-T1-noise", "parent_siblings-T0-clean"])
def toy_search(request):
    qt, temp, frac = request.param
    S, D, B = 20, 6, 6
    logits, value, emb, invalid, dirichlet, gumbel = toy_inputs(B, 11)
    trace = {}
    a, w, rv, trees = PZ.muzero_policy(0.37, logits, value, emb, toy_recurrent, S, invalid, dirichlet, gumbel,
                                       max_depth=D, temperature=temp, qtransform=qt, dirichlet_fraction=frac, seed=77,
                                       turn=3, trace=trace)
    return dict(S=S, D=D, B=B, temp=temp, invalid=invalid, a=a, w=w, rv=rv, trees=trees, trace=trace)


def test_restatement_visits_sum_to_simulations(toy_search):
    r = toy_search
    for t in r["trees"]:
        assert t.c_visits[0].sum() == r["S"] and t.visits[0] == r["S"] + 1
        assert t.visits.sum() <= (r["S"] + 1) * (r["D"] + 1)
    assert np.array_equal(np.rint(r["w"] * r["S"]), np.stack([t.c_visits[0] for t in r["trees"]]))
    assert np.abs(r["w"].sum(-1) - 1.0).max() < 1e-6
    assert r["trace"]["margin"].shape == (r["B"],) and (r["trace"]["margin"] >= 0).all()
    assert np.isfinite(r["rv"]).all()


def test_restatement_never_visits_invalid_root_actions(toy_search):
    r = toy_search
    for b, t in enumerate(r["trees"]):
        assert (t.c_visits[0][r["invalid"][b]] == 0).all()
    assert (r["w"][r["invalid"]] == 0).all()
    assert not r["invalid"][np.arange(r["B"]), r["a"]].any()
    assert r["a"][0] == 5 and r["w"][0, 5] == 1.0


def test_restatement_temperature_zero_picks_a_most_visited_action(toy_search):
    r = toy_search
    for b, t in enumerate(r["trees"]):
        if r["temp"] == 0.0:
            assert t.c_visits[0][r["a"][b]] == t.c_visits[0].max()
        else:                        # any temperature: only a visited action can be drawn
            assert t.c_visits[0][r["a"][b]] > 0


def test_temperature_zero_draw_breaks_ties_by_the_gumbel_draw():
    visits = np.array([3, 7, 0, 7, 1] + [0] * (A - 5))
    g = np.zeros(A, np.float32)
    g[3] = 0.5
    a, w, x = PZ.final_draw(visits, g, 0.0)
    # (log w - max) / tiny: 0 for a most-visited action, below -1e37 for a less visited one, -inf for an unvisited one
    assert a == 3 and x[1] == 0.0 and x[3] == 0.5 and (x[[0, 4]] < -1e37).all() and np.isneginf(x[2])
    assert w[1] == np.float32(7) / np.float32(18)
    g[2] = 100.0                     # an unvisited action stays out whatever its draw
    assert PZ.final_draw(visits, g, 0.0)[0] == 3 and PZ.final_draw(visits, g, 1.0)[0] == 3


def test_no_root_noise_leaves_the_masked_log_softmax():
    logits, _, _, invalid, dirichlet, _ = toy_inputs(5, 3)
    p0 = PZ.root_prior_logits(logits, invalid, dirichlet, 0.0)
    assert np.array_equal(p0, PZ.root_prior_logits(logits, invalid, dirichlet[::-1], 0.0))
    l64 = logits.astype(np.float64)
    ls = l64 - np.log(np.exp(l64 - l64.max(-1, keepdims=True)).sum(-1, keepdims=True)) - l64.max(-1, keepdims=True)
    want = ls - ls.max(-1, keepdims=True)
    assert (p0[invalid] == PZ.FMIN).all()
    assert np.abs(p0[~invalid] - want[~invalid]).max() < 1e-6
    p1 = PZ.root_prior_logits(logits, invalid, dirichlet, 0.25)
    assert not np.array_equal(p0, p1) and (p1[invalid] == PZ.FMIN).all()


def test_min_max_on_unvisited_children_is_policy_plus_tiebreak():
    rng = np.random.default_rng(5)
    t = PZ.Tree(4, A, LAT)
    t.update_node(0, rng.normal(size=A).astype(np.float32), np.float32(0.4), np.zeros(LAT, np.float32))
    tb = rng.random(A).astype(np.float32)
    none = np.zeros(A, bool)
    score, gain = PZ.action_scores(t, 0, 1, none, tb, PZ.QT_MIN_MAX)
    assert gain == 0.5
    assert np.array_equal(score, PZ.puct_policy_score(t, 0) + np.float32(1e-7) * tb)
    # pb_c at N = 1: 1.25 + log((1 + 19652 + 1) / 19652), times sqrt(1), times the prior over 0 + 1 visits
    pb_c = 1.25 + np.log(19654.0 / 19652.0)
    assert np.abs(PZ.puct_policy_score(t, 0) - pb_c * PZ.softmax(t.c_prior[0])).max() < 1e-6
    # a visited child contributes (q - min) / (max - min); the root mask applies at depth 0 only
    t.c_visits[0, 2], t.c_value[0, 2], t.c_reward[0, 2], t.c_disc[0, 2] = 1, 0.5, 0.1, -1.0
    assert PZ.qtransform_by_min_max(t, 0, -1.0, 1.0)[2] == np.float32((np.float32(0.1) - np.float32(0.5) + 1) / 2)
    mask = np.arange(A) % 2 == 0
    assert np.isneginf(PZ.action_scores(t, 0, 0, mask, tb)[0][mask]).all()
    assert np.isfinite(PZ.action_scores(t, 0, 1, mask, tb)[0]).all()
