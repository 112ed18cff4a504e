"""The Gumbel network-free MCTS agent for det-MADN (csrc/env_gumbel.hip, mcts.env_gumbel_muzero_policy, the
'gumbel_mcts_agent' seat), everything that needs no GPU: the restated search (tests/_env_gumbel.py) on the fixture's
root states, the interior mask, muz_detmadn_gumbel_mcts's refusals (argument checks come before any launch, so they
run on a host without a GPU) and the refusals of the Python entry points."""
import ctypes

import numpy as np
import pytest

from oracle import detmadn as dm
from oracle import mctx_gumbel as G
from tests import _env_gumbel as EG
from tests import _env_mcts as EM

F32 = np.float32
QTS = [EG.QT_COMPLETED_MIX, EG.QT_MIN_MAX]


def _lib():
    from exploring_muzero_on_dog_amd import lib as L
    return L


def _tagged(rule_set, tag):
    envs, tags = EM.load_roots(rule_set)
    return [e for e, ts in zip(envs, tags) if tag in ts]


# ---- the restated search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", QTS)
def test_restated_search_on_a_winning_root(qt):
    env = _tagged("default_2p", "wins")[0]
    r = EG.search_one(env, 8, 4, 20, 3, 0, 0, np.zeros(EM.A, F32), qtransform=qt)
    wm = EM.wins_trial(env)
    assert (wm >> r["action"]) & 1 and r["visits"].sum() == 8 and r["qvalues"][r["action"]] == 1.0
    lm = EM.node_mask(env)
    assert not r["visits"][~EM.bits_to_bool(lm)].any() and not r["weights"][~EM.bits_to_bool(lm)].any()
    assert abs(float(r["weights"].sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("qt", QTS)
def test_a_finished_root_is_not_searched(qt):
    done = _tagged("default_2p", "done")[0]
    r = EG.search_one(done, 8, 4, 20, 3, 0, 0, np.zeros(EM.A, F32), qtransform=qt)
    assert r["action"] == -1 and r["tree"] is None and not r["weights"].any() and r["value"] == 0 and r["turns"] == 0
    stuck = _tagged("default_2p", "stuck")[0]
    assert EG.search_one(stuck, 8, 4, 20, 3, 0, 0, np.zeros(EM.A, F32), qtransform=qt)["action"] == -1


def test_sequential_halving_spreads_the_root_visits():
    """S = 16 over a root with more than 4 legal actions and max_num_considered 4: the first 4 simulations visit 4
    different children, and no other child is ever visited."""
    envs, _ = EM.load_roots("default_2p")
    env = next(e for e in envs if bin(EM.node_mask(e)).count("1") > 4)
    r = EG.search_one(env, 16, 8, 0, 3, 0, 0, np.zeros(EM.A, F32), max_num_considered=4)
    assert (r["visits"] > 0).sum() == 4 and r["visits"].sum() == 16
    assert r["visits"][r["action"]] == r["visits"].max()


@pytest.mark.parametrize("qt", QTS)
def test_a_masked_child_is_never_selected_inside_the_tree(qt):
    """A hand-built interior node: actions 0 and 1 legal, 0 visited five times with q = -1, 1 once with q = +1.  Child
    0's softmax - visit share is negative; mctx's unmasked rule gives every illegal (never visited) child 0, above it.
    With the node's mask those are -inf, whatever the legal scores are."""
    mask = 0b11
    t = G.Tree(1, 8, EM.A, 1)
    G.update_tree_node(t, np.array([1], np.int32), EM.prior_logits(mask, 0)[None], np.array([0], F32),
                       np.zeros((1, 1), F32))
    t.children_visits[0, 1, :2] = (5, 1)
    t.children_index[0, 1, :2] = (2, 3)
    t.children_rewards[0, 1, :2] = (-1, 1)
    cq = EG.completed_q(t, 1, qt)
    score = EG.interior_scores(t, 1, mask, cq)
    assert score[0] < 0 < score[1] and np.isneginf(score[2:]).all() and int(np.argmax(score)) == 1
    visits = t.children_visits[0, 1]
    unmasked = G.softmax((t.children_prior_logits[0, 1] + cq)[None])[0] - visits / F32(1 + visits.sum())
    assert (unmasked[2:] == 0).all() and unmasked[0] < unmasked[2]          # why the -inf is written out
    # a node with mask 0 (finished, or without a legal action after the passes) counts as all 24 actions legal
    G.update_tree_node(t, np.array([4], np.int32), EM.prior_logits(0, 0)[None], np.array([0], F32),
                       np.zeros((1, 1), F32))
    assert np.isfinite(EG.interior_scores(t, 4, 0, EG.completed_q(t, 4, qt))).all()


def test_min_max_is_the_puct_restatements_transform():
    from tests import _mctx_muzero as PZ
    t = G.Tree(1, 4, EM.A, 1)
    t.children_visits[0, 0, :3] = (2, 0, 1)
    t.children_rewards[0, 0, :3] = (1, 1, 0)
    t.children_discounts[0, 0, :3] = (0, 0, -1)
    t.children_values[0, 0, :3] = (0, 0, 0.5)
    p = PZ.Tree(5, EM.A, 1)
    p.c_visits[0], p.c_reward[0], p.c_disc[0], p.c_value[0] = (t.children_visits[0, 0], t.children_rewards[0, 0],
                                                               t.children_discounts[0, 0], t.children_values[0, 0])
    got = EG.completed_q(t, 0, EG.QT_MIN_MAX, min_value=-1.0, max_value=1.0)
    assert np.array_equal(got, PZ.qtransform_by_min_max(p, 0, -1.0, 1.0))
    assert got[:3].tolist() == [1.0, 0.0, 0.25]


# ---- the C entry point's refusals (no launch) ----------------------------------------------------------------------
class _Call:
    """muz_detmadn_gumbel_mcts with never-dereferenced dummy pointers: every case here must return before any
    launch."""

    def __init__(self):
        from exploring_muzero_on_dog_amd import detmadn as E
        from exploring_muzero_on_dog_amd import mcts as M
        self.L = _lib()
        self.so = self.L.load()
        self.M, self.E = M, E
        self.buf = (ctypes.c_char * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.rules = E.make_rules(num_players=2, **dm.DEFAULT_RULES)

    def soa(self, n=1, null=None):
        s = self.L.MuzDetSoA()
        for name in ("board", "pins", "current_player", "reward", "done", "action_set"):
            setattr(s, name, None if name == null else self.p)
        s.stride = n
        return s

    def gcfg(self, rollout_steps=300, qtransform=None, min_value=-1.0, max_value=1.0):
        qt = self.L.MUZ_QT_COMPLETED_MIX if qtransform is None else qtransform
        return self.L.MuzEnvGumbelCfg(rollout_steps, qt, min_value, max_value)

    def __call__(self, cfg, n=1, ws_bytes=1 << 40, rules="det", gcfg="cfg", null=None, soa=None, ws=None, **g):
        P = [self.p] * 8   # gumbel, game_id, workspace, action, weights, value, visits, qvalues
        if null is not None:
            P[null] = None
        if ws is not None:
            P[2] = ws
        m = self.gcfg(**g)
        return self.so.muz_detmadn_gumbel_mcts(self.rules if rules == "det" else rules,
                                               ctypes.byref(cfg) if cfg is not None else None,
                                               ctypes.byref(m) if gcfg == "cfg" else None,
                                               self.soa(n) if soa is None else soa, P[0], P[1], n, P[2], ws_bytes,
                                               P[3], P[4], P[5], P[6], P[7], None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_env_gumbel_cfg_layout():
    L = _lib()
    C = L.MuzEnvGumbelCfg
    assert ctypes.sizeof(C) == 16
    assert [getattr(C, f).offset for f in ("rollout_steps", "qtransform", "min_value", "max_value")] == [0, 4, 8, 12]
    assert (L.MUZ_QT_MIN_MAX, L.MUZ_QT_PARENT_SIBLINGS, L.MUZ_QT_COMPLETED_MIX) == (0, 1, 2)
    assert ctypes.sizeof(L.MuzEnvMctsCfg) == 4                      # the PUCT agent's stays what it was
    assert "muz_detmadn_gumbel_mcts" in L.SIGNATURES


def test_gumbel_mcts_uses_the_puct_agents_workspace(call):
    """No size function of its own: muz_detmadn_mcts_tree_bytes for the same S; one byte less is MUZ_E_INVALID, n = 0
    with nothing MUZ_OK."""
    L, M = call.L, call.M
    for n in (1, 17, 4096):
        for S in (1, 50, 100):
            need = call.so.muz_detmadn_mcts_tree_bytes(n, ctypes.byref(M.make_puct_cfg(S, 1)))
            assert need == (n * 4 + 255) // 256 * 256 + n * (S + 1) * (6 * 32 * 4 + 64)
            cfg = M.make_cfg(S, min(S, 64))
            assert call(cfg, n=n, ws_bytes=need - 1) == L.MUZ_E_INVALID, (n, S)
            assert call(cfg, n=0, ws_bytes=0) == L.MUZ_OK
    assert not hasattr(call.so, "muz_detmadn_gumbel_mcts_tree_bytes")


@pytest.mark.parametrize("change", [
    dict(num_simulations=0), dict(num_simulations=101), dict(max_depth=0), dict(max_depth=65),
    dict(max_num_considered=0), dict(gumbel_scale=-0.5), dict(gumbel_scale=float("nan")), dict(value_scale=-1.0),
    dict(value_scale=float("nan")), dict(maxvisit_init=-1.0), dict(maxvisit_init=float("nan")),
    dict(rollout_steps=-1), dict(rollout_steps=1001), dict(qtransform=1), dict(qtransform=3), dict(qtransform=-1),
    dict(max_value=-1.0), dict(max_value=float("nan")), dict(min_value=2.0)])
def test_gumbel_mcts_refuses_unsupported_configurations(call, change):
    cfg = call.M.make_cfg(50, 25, 0.0)
    g = {k: change[k] for k in ("rollout_steps", "qtransform", "min_value", "max_value") if k in change}
    for k, v in change.items():
        if k not in g:
            setattr(cfg, k, v)
    assert call(cfg, **g) == call.L.MUZ_E_UNSUPPORTED
    assert call(cfg, null=3, **g) == call.L.MUZ_E_UNSUPPORTED      # even with a null pointer beside it


def test_gumbel_mcts_accepts_the_limits_and_refuses_rules(call):
    L, E = call.L, call.E
    cfg = call.M.make_cfg(50, 25, 0.0)
    for g in (dict(rollout_steps=0), dict(rollout_steps=1000), dict(qtransform=L.MUZ_QT_MIN_MAX),
              dict(qtransform=L.MUZ_QT_COMPLETED_MIX)):      # accepted: the next check (a short workspace) answers
        assert call(cfg, ws_bytes=0, **g) == L.MUZ_E_INVALID
    for k, v in (("gumbel_scale", 0.0), ("value_scale", 0.0), ("maxvisit_init", 0.0), ("max_num_considered", 1)):
        cfg = call.M.make_cfg(100, 64, 1.0)
        setattr(cfg, k, v)
        assert call(cfg, ws_bytes=0) == L.MUZ_E_INVALID, k
    cfg = call.M.make_cfg(50, 25, 0.0)
    assert call(cfg, rules=E.make_rules(num_players=2, starting_player=-1, **dm.DEFAULT_RULES)) == L.MUZ_E_UNSUPPORTED
    assert call(cfg, rules=E.make_rules(num_players=2, distance=12, **dm.DEFAULT_RULES)) == L.MUZ_E_UNSUPPORTED


def test_gumbel_mcts_refuses_null_pointers_and_bad_workspaces(call):
    L = call.L
    cfg = call.M.make_cfg(50, 25, 0.0)
    assert call(None) == L.MUZ_E_INVALID
    assert call(cfg, gcfg=None) == L.MUZ_E_INVALID
    assert call(cfg, rules=None) == L.MUZ_E_INVALID
    assert call(cfg, n=-1) == L.MUZ_E_INVALID
    assert call(cfg, n=2, soa=call.soa(1)) == L.MUZ_E_INVALID          # fewer games in the state than searched
    for i in (2, 3, 4, 5):        # gumbel, game_id (0, 1) and visit_counts, qvalues (6, 7) may be null
        assert call(cfg, null=i) == L.MUZ_E_INVALID, i
    for name in ("board", "pins", "action_set", "current_player", "done", "reward"):
        assert call(cfg, soa=call.soa(1, null=name)) == L.MUZ_E_INVALID, name
    off = ctypes.c_void_p(ctypes.addressof(call.buf) + 4)              # not 16-byte aligned
    assert ctypes.addressof(call.buf) % 16 == 0
    assert call(cfg, ws=off) == L.MUZ_E_INVALID


def test_the_puct_entry_keeps_refusing_the_gumbel_qtransform(call):
    """MUZ_QT_COMPLETED_MIX is muz_env_gumbel_cfg's: muz_puct_cfg (check_puct_cfg) still knows two transforms."""
    cfg = call.M.make_puct_cfg(50, 25)
    cfg.qtransform = call.L.MUZ_QT_COMPLETED_MIX
    so, p = call.so, call.p
    rc = so.muz_detmadn_mcts(call.rules, ctypes.byref(cfg), ctypes.byref(call.L.MuzEnvMctsCfg(300)), call.soa(1), p, p,
                             p, 1, p, 1 << 40, p, p, p, p, p, None)
    assert rc == call.L.MUZ_E_UNSUPPORTED


# ---- the Python entry points ---------------------------------------------------------------------------------------
def test_python_entry_points_refuse_where_no_environment_model_exists():
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    assert EV._seat(EV._Det, "gumbel_mcts_agent", 0, 0, "cpu") == "gumbel_mcts_agent" == EV.GUMBEL_MCTS_AGENT
    assert EV._Det.GUMBEL_SEAT == EV.GUMBEL_MCTS_AGENT and EV._Det.ENV_SEAT == EV.MCTS_AGENT
    assert EV._Classic.GUMBEL_SEAT is None and EV._Dog.GUMBEL_SEAT is None
    for game, why in ((EV._Classic, "chance nodes"), (EV._Dog, "hidden hands")):
        with pytest.raises(ValueError, match="Gumbel environment-model search") as e:
            EV._seat(game, "gumbel_mcts_agent", 0, 0, "cpu")
        assert why in str(e.value)
    with pytest.raises(ValueError, match="unknown agent"):
        EV._seat(EV._Det, "gumbel_mcts", 0, 0, "cpu")
    with pytest.raises(ValueError, match="gumbel_mcts_agent"):
        EV.play_vs_random("rule_based_agent", 4, device="cpu")      # a seat of evaluate_agent_parallel only
    with pytest.raises(ValueError):
        EV._search_kwargs("gumbel_mcts_agent")    # a seat, not a search of a network
    with pytest.raises(TypeError, match="det-MADN"):
        M.env_gumbel_muzero_policy(object(), 8, 4, seed=0, turn=0)
    with pytest.raises(TypeError):
        M.env_gumbel_muzero_policy(None, 8, 4)    # seed and turn are required: the rollouts are keyed by them
    with pytest.raises(TypeError):
        M.env_gumbel_muzero_policy(None, 8, 4, seed=0)
    assert sorted(M.GUMBEL_QTRANSFORMS) == ["completed_by_mix_value", "min_max"]
