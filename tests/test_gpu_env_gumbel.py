"""The Gumbel network-free MCTS kernel (csrc/env_gumbel.hip, mcts.env_gumbel_muzero_policy) against its NumPy
restatement (tests/_env_gumbel.py) on the GPU, on the root states of tests/golden/env_mcts_roots.json (24 per rule
set, 1 to 20 legal actions: max_num_considered 16 both bites and does not).

The model's values are in {-1, 0, 1} and the tree arithmetic is the Gumbel search's, restated operation by operation
(no fma, numpy's pairwise sums, exp rounded once from float64), so there is no tolerance: actions, action weights,
root values, visit counts, q-values and the number of rollout turns are compared bit for bit.  The root's Gumbel noise
is passed in or scaled by 0 (the device's own draw goes through libm's log and is not restated); the tests of keying
and determinism use the device's draw at scale 1."""
import functools

import numpy as np
import pytest
import torch

from tests import _env_gumbel as EG
from tests import _env_mcts as EM

pytestmark = pytest.mark.gpu

SEED, TURN = 20262, 5
QTS = [EG.QT_COMPLETED_MIX, EG.QT_MIN_MAX]


def _mods():
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import lib as L
    from exploring_muzero_on_dog_amd import mcts as M
    return E, L, M


@functools.lru_cache(maxsize=None)
def roots(rule_set):
    envs, tags = EM.load_roots(rule_set)
    return tuple(envs), tuple(tuple(t) for t in tags)


def gumbel_noise(n, seed=5):
    return np.random.default_rng(seed).gumbel(size=(n, EM.A)).astype(np.float32)


def gpu_search(rule_set, envs, S, D, temperature, rollout_steps, gids=None, gumbel=None, **kw):
    E, L, M = _mods()
    st = EM.device_state(E, rule_set, envs)
    ws = M.EnvSearchWorkspace(len(envs), S)
    pol, rv, visits, q = M.env_gumbel_muzero_policy(
        st, S, D, temperature, rollout_steps=rollout_steps, seed=SEED, turn=TURN, summary=True, workspace=ws,
        game_id=None if gids is None else torch.from_numpy(np.asarray(gids, np.int32)),
        gumbel=None if gumbel is None else torch.from_numpy(gumbel), **kw)
    torch.cuda.synchronize()
    return dict(action=pol.action.cpu().numpy(), weights=pol.action_weights.cpu().numpy(), value=rv.cpu().numpy(),
                visits=visits.cpu().numpy(), qvalues=q.cpu().numpy(), turns=ws.rollout_turns(len(envs)).cpu().numpy())


def same(label, got, want):
    """Bit for bit, every output; the figures are printed before they are asserted."""
    diff = {k: int((np.asarray(got[k]) != np.asarray(want[k])).sum()) for k in want}
    print(f"{label}: searched {int((want['action'] >= 0).sum())} of {len(want['action'])} games, rollout turns "
          f"{int(want['turns'].sum())}, differing entries {diff}")
    for k in ("visits", "action", "weights", "value", "qvalues", "turns"):
        assert np.array_equal(got[k], want[k]), (label, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:5])


def check(label, rule_set, envs, S, D, rollout_steps, gids=None, gumbel=None, **kw):
    """The device at Gumbel scale 0 (or with the noise passed in) against the restatement."""
    got = gpu_search(rule_set, envs, S, D, 0.0 if gumbel is None else 1.0, rollout_steps, gids, gumbel, **kw)
    want = EG.env_gumbel_muzero_policy(list(envs), S, D, rollout_steps, SEED, TURN, gids, gumbel, **kw)
    same(label, got, want)
    return got, want


@pytest.mark.parametrize("qt", QTS)
@pytest.mark.parametrize("rule_set", list(EM.RULE_SETS))
def test_tree_only_matches_restatement(cuda, rule_set, qt):
    """rollout_steps = 0: every leaf value is 0, the tree is driven by rewards, discounts and masks alone.  21 games:
    one full 16-row tile and a 5-row tail; among them the finished game and the one without a legal action."""
    envs, tags = roots(rule_set)
    got, want = check(f"env gumbel tree only {rule_set} {qt}", rule_set, envs[:21], 50, 25, 0,
                      gids=7 * np.arange(21) + 3, qtransform=qt)
    skipped = np.array([("done" in t) or ("stuck" in t) for t in tags[:21]])
    assert skipped.any() and np.array_equal(got["action"] == -1, skipped)
    assert (got["visits"][~skipped].sum(1) == 50).all() and not got["visits"][skipped].any()
    assert (got["turns"] == 0).all()
    legal = np.array([EM.bits_to_bool(EM.node_mask(e)) for e in envs[:21]])
    assert not got["visits"][~legal].any() and not got["weights"][~legal].any()
    assert np.allclose(got["weights"][~skipped].sum(1), 1.0, atol=1e-5)
    # sequential halving: at most 16 children of a root are ever visited, and some roots have more legal actions
    assert ((got["visits"] > 0).sum(1) <= 16).all() and (legal.sum(1) > 16).any()


@pytest.mark.parametrize("rule_set", list(EM.RULE_SETS))
def test_rollouts_match_restatement(cuda, rule_set):
    envs, tags = roots(rule_set)
    pick = [i for i, t in enumerate(tags) if "pass" in t or "bonus" in t][:3] + [len(envs) - 2, len(envs) - 1]
    got, _ = check(f"env gumbel rollouts {rule_set}", rule_set, [envs[i] for i in pick], 8, 5, 40, gids=pick)
    assert (got["turns"] > 0).all() and (got["turns"] <= 9 * 40).all()


def test_rollouts_to_the_end_match_restatement(cuda):
    envs, _ = roots("default_2p")
    got, _ = check("env gumbel to the end", "default_2p", envs[-2:], 3, 3, 300)
    # rollouts that reach the end of the game give +-1 leaf values
    assert (got["turns"] < 4 * 300).any() and ((got["qvalues"] != 0).any() or (got["value"] != 0).any())


@pytest.mark.parametrize("S,D", [(1, 1), (1, 8), (8, 1), (2, 2)])
def test_limits_match_restatement(cuda, S, D):
    envs, _ = roots("selfplay_4p_teams")
    check(f"env gumbel limits S{S} D{D}", "selfplay_4p_teams", envs[1::4], S, D, 12)


@pytest.mark.parametrize("m", [1, 4, 16])
def test_max_num_considered_matches_restatement(cuda, m):
    envs, _ = roots("default_2p")
    got, _ = check(f"env gumbel considered {m}", "default_2p", envs, 16, 6, 0, max_num_considered=m)
    live = got["action"] >= 0
    assert ((got["visits"][live] > 0).sum(1) <= m).all() and ((got["visits"][live] > 0).sum(1) == m).any()


@pytest.mark.parametrize("qt", QTS)
def test_gumbel_noise_matches_restatement(cuda, qt):
    envs, _ = roots("default_2p")
    noise = gumbel_noise(len(envs), 11)
    got, _ = check(f"env gumbel noise {qt}", "default_2p", envs, 16, 6, 0, gumbel=noise, qtransform=qt)
    quiet = gpu_search("default_2p", envs, 16, 6, 0.0, 0, qtransform=qt)
    assert not np.array_equal(got["visits"], quiet["visits"])        # the noise decides which actions are considered


def test_a_game_is_keyed_by_its_id_not_its_lane(cuda):
    """A subset of the games under their game ids gives the outputs those games have in the full batch (the device's
    own Gumbel draw at scale 1 included): nothing is keyed by lane or batch position."""
    envs, _ = roots("selfplay_4p_teams")
    n = len(envs)
    gids = 100 + np.arange(n)
    full = gpu_search("selfplay_4p_teams", envs, 8, 5, 1.0, 300, gids=gids)
    sub = [19, 2, 11, 5, 23, 8, 16]
    part = gpu_search("selfplay_4p_teams", [envs[i] for i in sub], 8, 5, 1.0, 300, gids=gids[sub])
    for k in full:
        assert np.array_equal(part[k], full[k][sub]), k
    other = gpu_search("selfplay_4p_teams", [envs[i] for i in sub], 8, 5, 1.0, 300, gids=gids[sub] + 1)
    assert not all(np.array_equal(other[k], part[k]) for k in ("turns", "value", "weights"))   # other ids, other draws


def test_two_calls_with_one_seed_are_identical(cuda):
    envs, _ = roots("default_2p")
    a = gpu_search("default_2p", envs, 8, 5, 1.0, 60)
    b = gpu_search("default_2p", envs, 8, 5, 1.0, 60)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert (a["action"] >= 0).sum() >= len(envs) - 4


@pytest.mark.parametrize("qt", QTS)
def test_takes_the_win(cuda, qt):
    """Gumbel scale 0, S = 8: every fixture state with a winning action gets an action inside wins."""
    for rule_set in EM.RULE_SETS:
        envs, tags = roots(rule_set)
        win = [e for e, t in zip(envs, tags) if "wins" in t]
        assert win
        got = gpu_search(rule_set, win, 8, 8, 0.0, 300, qtransform=qt)
        for b, env in enumerate(win):
            assert (EM.wins_trial(env) >> int(got["action"][b])) & 1, (rule_set, b, got["action"][b])
            assert got["qvalues"][b][got["action"][b]] == 1.0


def test_refusals_return_their_codes_without_a_launch(cuda):
    E, L, M = _mods()
    envs, _ = roots("default_2p")
    st = EM.device_state(E, "default_2p", envs[:4])
    for kw in (dict(rollout_steps=1001), dict(max_num_considered=0), dict(temperature=-1.0), dict(value_scale=-0.5),
               dict(min_value=1.0, max_value=1.0)):
        with pytest.raises(L.MuzError, match="unsupported"):
            M.env_gumbel_muzero_policy(st, 8, 4, seed=0, turn=0, **kw)
    with pytest.raises(L.MuzError, match="unsupported"):
        M.env_gumbel_muzero_policy(st, 8, 65, seed=0, turn=0)
    with pytest.raises(ValueError, match="unknown qtransform"):
        M.env_gumbel_muzero_policy(st, 8, 4, seed=0, turn=0, qtransform="parent_and_siblings")
    ws = M.EnvSearchWorkspace(4, 8)
    short = M.EnvSearchWorkspace(4, 8)
    short.tree = short.tree[:-1]
    with pytest.raises(L.MuzError, match="invalid"):
        M.env_gumbel_muzero_policy(st, 8, 4, seed=0, turn=0, workspace=short)
    out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    cfg = M.make_cfg(8, 4, 0.0)
    gcfg = L.MuzEnvGumbelCfg(300, L.MUZ_QT_COMPLETED_MIX, -1.0, 1.0)
    so = L.load()
    rc = so.muz_detmadn_gumbel_mcts(st.rules, cfg, gcfg, st.soa(), None, None, 4, L.ptr(ws.tree), L.nbytes(ws.tree),
                                    L.ptr(out), None, None, None, None, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.MUZ_E_INVALID and (out.cpu().numpy() == -7).all()     # nothing was launched
    bad = L.MuzEnvGumbelCfg(300, 7, -1.0, 1.0)
    w = torch.full((4, EM.A), -7.0, device="cuda")
    rc = so.muz_detmadn_gumbel_mcts(st.rules, cfg, bad, st.soa(), None, None, 4, L.ptr(ws.tree), L.nbytes(ws.tree),
                                    L.ptr(out), L.ptr(w), L.ptr(w), None, None, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.MUZ_E_UNSUPPORTED and (out.cpu().numpy() == -7).all() and (w.cpu().numpy() == -7).all()
    rc = so.muz_detmadn_gumbel_mcts(st.rules, cfg, gcfg, st.soa(), None, None, 0, L.ptr(ws.tree), 0, L.ptr(out),
                                    L.ptr(out), L.ptr(out), None, None, L.stream_ptr())
    assert rc == L.MUZ_OK                                                # n == 0: nothing to do


def test_the_puct_agent_is_unmoved(cuda):
    """k_env_mcts takes its model through the header it now shares with k_env_gumbel: one env_muzero_policy call on the
    same roots, rollouts and passes included, still equals tests/_env_mcts.py bit for bit."""
    E, L, M = _mods()
    envs, _ = roots("default_2p")
    gids = 3 * np.arange(len(envs)) + 1
    st = EM.device_state(E, "default_2p", envs)
    ws = M.EnvSearchWorkspace(len(envs), 12)
    noise = gumbel_noise(len(envs), 7)
    pol, rv, visits, q = M.env_muzero_policy(st, 12, 6, 0.0, rollout_steps=30, seed=SEED, turn=TURN, summary=True,
                                             workspace=ws, game_id=torch.from_numpy(gids.astype(np.int32)),
                                             gumbel=torch.from_numpy(noise))
    torch.cuda.synchronize()
    got = dict(action=pol.action.cpu().numpy(), weights=pol.action_weights.cpu().numpy(), value=rv.cpu().numpy(),
               visits=visits.cpu().numpy(), qvalues=q.cpu().numpy(), turns=ws.rollout_turns(len(envs)).cpu().numpy())
    same("env mcts beside env gumbel", got, EM.env_muzero_policy(list(envs), 12, 6, 0.0, 30, SEED, TURN, gids, None,
                                                                 noise))
