"""The DOG rollout agent on the GPU (csrc/dog_rollout.hip through dog.rollout_policy) against its definition, the NumPy
restatement tests/_dog_rollout.py: action, visits, wins, value and rollout turns bit for bit on every fixture root.

Sizes: R = 2, max_phases = 3, rollout_steps = 24 and the 17 late-game roots of tests/golden/dog_rollout_roots.json (at
most 8 candidates each), which keeps the Python restatement's share of a case at a few seconds; its results are computed
once per (root, configuration, game id) and shared between the tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _dog_rollout as DR
from tests.dog_states import fields_of

pytestmark = pytest.mark.gpu

R, PHASES, STEPS = 2, 3, 24
SEED, TURN = 11, 3
RULE_SETS = sorted(DR.RULE_SETS)


def _D():
    from exploring_muzero_on_dog_amd import dog as D
    return D


@functools.lru_cache(maxsize=None)
def roots(rule_set):
    return DR.load_roots(rule_set)


@functools.lru_cache(maxsize=None)
def want(rule_set, b, det, gid, rollouts=R, phases=PHASES):
    r = DR.search_one(roots(rule_set)[0][b], rollouts, phases, STEPS, det, SEED, TURN, gid)
    for k in ("visits", "wins"):
        r[k].setflags(write=False)
    return r


def to_gpu(rule_set, envs):
    D = _D()
    return D.state_from_host(fields_of(envs), D.make_rules(**DR.RULE_SETS[rule_set]), seed=5)


def search(env, det, game_id=None, rollouts=R, phases=PHASES):
    out = _D().rollout_policy(env, rollouts, max_phases=phases, rollout_steps=STEPS, determinize=bool(det), seed=SEED,
                              turn=TURN, game_id=game_id, summary=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def assert_equal(got, b, w, what):
    action, value, visits, wins, turns = got
    assert int(action[b]) == w["action"], (what, int(action[b]), w["action"])
    assert np.array_equal(visits[b], w["visits"]), (what, "visits", np.flatnonzero(visits[b] != w["visits"]))
    assert np.array_equal(wins[b], w["wins"]), (what, "wins", np.flatnonzero(wins[b] != w["wins"]))
    assert value[b].tobytes() == np.float32(w["value"]).tobytes(), (what, float(value[b]), float(w["value"]))
    assert int(turns[b]) == w["turns"], (what, int(turns[b]), w["turns"])


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_search_equals_the_restatement_bit_for_bit(cuda, rule_set, det):
    envs, tags = roots(rule_set)
    got = search(to_gpu(rule_set, envs), det)
    searched = 0
    for b, ts in enumerate(tags):
        w = want(rule_set, b, det, b)
        assert_equal(got, b, w, (rule_set, det, b, ts))
        searched += len(w["sets"]) > 1
        if "forced" in ts or "stuck" in ts:
            assert not got[2][b].any() and got[1][b] == 0
    assert searched >= 3


def test_three_rollouts_and_ten_phases(cuda):
    """R = 3 and max_phases = 10: every searched root runs down to one candidate."""
    rule_set = "exotic_3p"
    envs, tags = roots(rule_set)
    got = search(to_gpu(rule_set, envs), 1, rollouts=3, phases=10)
    for b, ts in enumerate(tags):
        w = want(rule_set, b, 1, b, 3, 10)
        assert_equal(got, b, w, (rule_set, b, ts))
        assert len(w["sets"][-1]) <= 1
    assert max(len(want(rule_set, b, 1, b, 3, 10)["sets"]) for b in range(len(envs))) >= 4   # three halvings


def test_result_is_keyed_by_game_id_not_by_batch_position(cuda):
    rule_set = "selfplay_4p_teams"
    envs, tags = roots(rule_set)
    x = next(b for b, ts in enumerate(tags) if "joker" in ts)
    n = 64
    batch = [envs[(i * 3 + 1) % len(envs)] for i in range(n)]
    gid = np.arange(n, dtype=np.int32) + 1000
    for pos in (0, 5, 63):
        batch[pos] = envs[x]
        gid[pos] = x
    got = search(to_gpu(rule_set, batch), 1, game_id=torch.from_numpy(gid))
    for pos in (0, 5, 63):
        assert_equal(got, pos, want(rule_set, x, 1, x), ("position", pos))
    # the same roots under other game ids: each follows the restatement at ITS id (shown on the roots with at most 3
    # candidates, which keeps the restatement quick), and the searched ones draw other random numbers than at id b
    small = [b for b in range(len(envs)) if len(DR.candidates(envs[b])) <= 3]
    ids = np.arange(len(envs), dtype=np.int32) + 100
    got = search(to_gpu(rule_set, envs), 1, game_id=torch.from_numpy(ids))
    differ = 0
    for b in small:
        w = want(rule_set, b, 1, int(ids[b]))
        assert_equal(got, b, w, ("game id", b))
        differ += w["turns"] != want(rule_set, b, 1, b)["turns"] or not np.array_equal(w["wins"],
                                                                                       want(rule_set, b, 1, b)["wins"])
    assert len(small) >= 4 and differ >= 1


def test_hidden_cards_do_not_reach_the_result(cuda):
    """Two roots that differ only in how the hidden cards are spread over the non-observers' hands, their swap choices
    and the deck (same hand sizes): with determinize = 1 every output is identical."""
    rule_set = "selfplay_4p_teams"
    envs, tags = roots(rule_set)
    pick = [b for b, ts in enumerate(tags) if "joker" in ts or "swap_partial" in ts or "partner" in ts]
    assert len(pick) >= 3
    base = [envs[b] for b in pick]
    spread = [DR.determinize(e, 0xABCDEF12345 + b) for b, e in zip(pick, base)]
    for e, s in zip(base, spread):
        assert not np.array_equal(e.hands, s.hands) or not np.array_equal(e.deck, s.deck)
        assert np.array_equal(DR.hidden_multiset(e), DR.hidden_multiset(s))
        assert np.array_equal(e.hands.sum(1), s.hands.sum(1))
        for q in DR.observers(e):
            assert np.array_equal(e.hands[q], s.hands[q])
    gid = torch.tensor(pick, dtype=torch.int32)
    a = search(to_gpu(rule_set, base), 1, game_id=gid)
    b = search(to_gpu(rule_set, spread), 1, game_id=gid)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[2].any()


def test_search_leaves_the_state_alone(cuda):
    D = _D()
    rule_set = "selfplay_4p_teams"
    env = to_gpu(rule_set, roots(rule_set)[0])
    fields = list(D.DOGState.ROWS) + list(D.DOGState.VECTORS)
    before = {k: getattr(env, k).clone() for k in fields}
    search(env, 1)
    for k in fields:
        assert torch.equal(before[k], getattr(env, k)), k


def test_empty_batch_launches_nothing(cuda):
    from exploring_muzero_on_dog_amd import lib as L
    D = _D()
    cfg = L.MuzDogRolloutCfg(R, PHASES, STEPS, 1, SEED, TURN)
    rules = D.make_rules(**DR.RULE_SETS["selfplay_4p_teams"])
    soa = L.MuzDogSoA()
    soa.stride = 0
    torch.cuda.synchronize()
    rc = L.load().muz_dog_rollout_search(rules, ctypes.byref(cfg), soa, None, None, None, None, None, None, 0, None, 0,
                                         L.stream_ptr())
    assert rc == L.MUZ_OK
    torch.cuda.synchronize()
