"""The classic network-free MCTS kernel (csrc/classic_env_mcts.hip, stochastic.env_stochastic_muzero_policy) against
its NumPy restatement (tests/_classic_env_mcts.py) on the GPU, on the root states of
tests/golden/classic_env_mcts_roots.json.

Every value of the search is in {-1, 0, 1}, the priors are 0, 1/k or the environment's die tables, and the tree
arithmetic is restated operation by operation, so there is no tolerance: actions, visit counts, action weights, root
values, q-values and the number of rollout turns are compared bit for bit.  The final draw's Gumbel noise is passed in
(the device's own draw goes through libm's log and is not restated); the tests of keying and determinism use the
device's draw."""
import functools

import numpy as np
import pytest
import torch

from tests import _classic_env_mcts as CM

pytestmark = pytest.mark.gpu

SEED, TURN = 20271, 5
RULE_SETS = list(CM.RULE_SETS)


def _mods():
    from exploring_muzero_on_dog_amd import classic as E
    from exploring_muzero_on_dog_amd import lib as L
    from exploring_muzero_on_dog_amd import stochastic as ST
    return E, L, ST


@functools.lru_cache(maxsize=None)
def roots(rule_set):
    envs, tags = CM.load_roots(rule_set)
    return tuple(envs), tuple(tuple(t) for t in tags)


def noise(n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.dirichlet(np.full(CM.A, 0.3), n).astype(np.float32), rng.gumbel(size=(n, CM.A)).astype(np.float32))


def gpu_search(rule_set, envs, S, D, temperature, rollout_steps, gids=None, dirichlet=None, gumbel=None, **kw):
    E, L, ST = _mods()
    st = CM.device_state(E, rule_set, envs)
    ws = ST.ClassicEnvSearchWorkspace(len(envs), S)
    pol, rv, visits, q = ST.env_stochastic_muzero_policy(
        st, S, D, temperature, rollout_steps=rollout_steps, seed=SEED, turn=TURN, summary=True, workspace=ws,
        game_id=None if gids is None else torch.from_numpy(np.asarray(gids, np.int32)),
        dirichlet=None if dirichlet is None else torch.from_numpy(dirichlet),
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


def check(label, rule_set, envs, S, D, temperature, rollout_steps, gids=None, dirichlet=None, gumbel=None, **kw):
    n = len(envs)
    gumbel = noise(n)[1] if gumbel is None else gumbel
    got = gpu_search(rule_set, envs, S, D, temperature, rollout_steps, gids, dirichlet, gumbel, **kw)
    want = CM.env_stochastic_muzero_policy(list(envs), S, D, temperature, rollout_steps, SEED, TURN, gids, dirichlet,
                                           gumbel, **kw)
    same(label, got, want)
    return got, want


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_tree_only_matches_restatement(cuda, rule_set):
    """rollout_steps = 0: every leaf value is 0 (a won afterstate's 1), the tree is driven by rewards, discounts, masks
    and the chance priors alone.  21 games: one full 16-row tile and a 5-row tail; among them a finished game and one
    without a legal pin."""
    envs, tags = roots(rule_set)
    got, want = check(f"classic env mcts tree only {rule_set}", rule_set, envs[:21], 50, 25, 0.0, 0,
                      gids=7 * np.arange(21) + 3)
    done = np.array(["done" in t for t in tags[:21]])
    stuck = np.array(["stuck" in t for t in tags[:21]])
    skipped = done | stuck
    assert done.any() and stuck.any() and np.array_equal(got["action"] == -1, skipped)
    assert (got["visits"][~skipped].sum(1) == 50).all() and not got["visits"][skipped].any()
    assert not got["weights"][skipped].any() and not got["value"][skipped].any()
    assert (got["turns"] == 0).all()


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_rollouts_match_restatement(cuda, rule_set):
    envs, tags = roots(rule_set)
    kinds = ("softlock", "bonus", "partner", "wins") if rule_set != "default_2p" else ("bonus", "wins")
    pick = []
    for kind in kinds:
        pick += [i for i, t in enumerate(tags) if kind in t and i not in pick][:1]
    pick += [i for i in range(len(envs) - 1, -1, -1) if i not in pick and "done" not in tags[i]
             and "stuck" not in tags[i]][:5 - len(pick)]
    assert len(pick) == 5 and any("bonus" in tags[i] for i in pick)
    assert rule_set == "default_2p" or any("softlock" in tags[i] for i in pick)
    got, _ = check(f"classic env mcts rollouts {rule_set}", rule_set, [envs[i] for i in pick], 8, 5, 0.0, 40, gids=pick)
    assert (got["turns"] > 0).all() and (got["turns"] <= 9 * 40).all()


def _late(rule_set, k, skip=()):
    """The k unfinished, movable roots with the most pins in a goal (none with a tag in `skip`)."""
    envs, tags = roots(rule_set)
    live = [i for i, t in enumerate(tags) if not {"done", "stuck", *skip} & set(t)]
    live.sort(key=lambda i: -int((envs[i].pins >= envs[i].board_size).sum()))
    return [envs[i] for i in live[:k]]


def test_rollouts_to_the_end_match_restatement(cuda):
    """Late roots without a winning pin: the rollouts play on, most of them to the end of the game."""
    got, _ = check("classic env mcts to the end", "default_2p", _late("default_2p", 2, skip=("wins",)), 3, 3, 0.0, 300)
    # rollouts that reach the end of the game give +-1 leaf values
    assert (got["turns"] > 4).all() and (got["turns"] < 4 * 300).any()
    assert (got["qvalues"] != 0).any() or (got["value"] != 0).any()


@pytest.mark.parametrize("S,D", [(1, 1), (1, 8), (8, 1)])
def test_limits_match_restatement(cuda, S, D):
    envs, _ = roots("selfplay_4p_teams")
    check(f"classic env mcts limits S{S} D{D}", "selfplay_4p_teams", envs[1::4], S, D, 0.0, 12)


def test_root_noise_and_temperature_match_restatement(cuda):
    envs, _ = roots("rethrow_six_2p")
    dirichlet, gumbel = noise(len(envs), 11)
    check("classic env mcts noise", "rethrow_six_2p", envs, 16, 6, 1.0, 0, dirichlet=dirichlet, gumbel=gumbel,
          dirichlet_fraction=0.25)


def test_summary_is_the_restated_trees(cuda):
    """visit_counts and qvalues as search_tree.summary() gives them after _mask_tree: the root's children_visits of the
    4 pins, and children_rewards + children_discounts * children_values with 0 for an unvisited child."""
    pick = _late("selfplay_4p_teams", 4)
    got = gpu_search("selfplay_4p_teams", pick, 12, 6, 0.0, 20, gumbel=noise(4)[1])
    for b, env in enumerate(pick):
        r = CM.search_one(env, 12, 6, 0.0, 20, SEED, TURN, b, np.zeros(CM.A, np.float32), noise(4)[1][b])
        t = r["tree"]
        assert np.array_equal(got["visits"][b], t.c_visits[0, :CM.A])
        q = (t.c_reward[0] + t.c_disc[0] * t.c_value[0]).astype(np.float32)[:CM.A]
        assert np.array_equal(got["qvalues"][b], q)
        assert (got["qvalues"][b][t.c_visits[0, :CM.A] == 0] == 0).all()
        assert np.array_equal(got["weights"][b], (t.c_visits[0, :CM.A] / np.float32(12)).astype(np.float32))
        assert got["value"][b] == np.clip(t.value[0], -1, 1)


def test_a_game_is_keyed_by_its_id_not_its_lane(cuda):
    """A subset of the games under their game ids gives the outputs those games have in the full batch (the device's
    own Gumbel draw included): nothing is keyed by lane or batch position."""
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
    assert (a["action"] >= 0).sum() >= len(envs) - 6


def test_takes_the_win(cuda):
    """Temperature 0, S = 8: every fixture state with a winning pin gets an action inside wins, with q-value 1.0."""
    for rule_set in RULE_SETS:
        envs, tags = roots(rule_set)
        win = [e for e, t in zip(envs, tags) if "wins" in t]
        assert win
        got = gpu_search(rule_set, win, 8, 8, 0.0, 300, gumbel=noise(len(win))[1])
        for b, env in enumerate(win):
            assert (CM.wins_trial(env) >> int(got["action"][b])) & 1, (rule_set, b, got["action"][b])
            assert got["qvalues"][b][got["action"][b]] == 1.0


def test_refusals_return_their_codes_without_a_launch(cuda):
    E, L, ST = _mods()
    envs, _ = roots("default_2p")
    st = CM.device_state(E, "default_2p", envs[:4])
    with pytest.raises(L.MuzError, match="unsupported"):
        ST.env_stochastic_muzero_policy(st, 8, 4, seed=0, turn=0, rollout_steps=1001)
    with pytest.raises(L.MuzError, match="unsupported"):
        ST.env_stochastic_muzero_policy(st, 8, 65, seed=0, turn=0)
    with pytest.raises(L.MuzError, match="unsupported"):
        ST.env_stochastic_muzero_policy(st, 8, 4, seed=0, turn=0, temperature=-1.0)
    ws = ST.ClassicEnvSearchWorkspace(4, 8)
    short = ST.ClassicEnvSearchWorkspace(4, 8)
    short.tree = short.tree[:-1]
    with pytest.raises(L.MuzError, match="invalid"):
        ST.env_stochastic_muzero_policy(st, 8, 4, seed=0, turn=0, workspace=short)
    out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    cfg = ST.make_cfg(8, 4, 0.0)
    rc = L.load().muz_classic_mcts(st.rules, cfg, L.MuzEnvMctsCfg(300), st.soa(), None, None, None, 4,
                                   L.ptr(ws.tree), L.nbytes(ws.tree), L.ptr(out), None, None, None, None,
                                   L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.MUZ_E_INVALID and (out.cpu().numpy() == -7).all()     # nothing was launched
    rc = L.load().muz_classic_mcts(st.rules, cfg, L.MuzEnvMctsCfg(300), st.soa(), None, None, None, 0,
                                   L.ptr(ws.tree), 0, L.ptr(out), L.ptr(out), L.ptr(out), None, None, L.stream_ptr())
    assert rc == L.MUZ_OK                                                # n == 0: nothing to do
