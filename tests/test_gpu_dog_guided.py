"""The DOG rollout agent with greedy-guided playouts on the GPU (csrc/dog_guided.hip through dog.guided_rollout_policy)
against its definition, the NumPy restatement tests/_dog_guided.py: action, value, visits, wins, rollout turns and the
decided count bit for bit on every fixture root.

Sizes: those of tests/test_gpu_dog_rollout.py -- R = 2, max_phases = 3, rollout_steps = 24 and the 17 late-game roots
of tests/golden/dog_rollout_roots.json (at most 8 candidates each) --, which keeps the Python restatement's share of a
case at a few seconds; its results are computed once per (root, configuration, game id) and shared between the tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _dog_guided as DG
from tests import _dog_rollout as DR
from tests.dog_states import fields_of

pytestmark = pytest.mark.gpu

R, PHASES, STEPS = 2, 3, 24
SEED, TURN = 11, 3
RULE_SETS = sorted(DR.RULE_SETS)
NEGATIVE = dict(advance=3, setback=-2, goal=-32768, out=32767, hit=-7, win=-1)   # tests/test_gpu_dog_greedy.py's set


def _D():
    from exploring_muzero_on_dog_amd import dog as D
    return D


@functools.lru_cache(maxsize=None)
def roots(rule_set):
    return DR.load_roots(rule_set)


def _key(weights):
    return None if weights is None else tuple(sorted(weights.items()))


@functools.lru_cache(maxsize=None)
def _want(rule_set, b, det, gid, epsilon, wkey):
    r = DG.search_one(roots(rule_set)[0][b], R, PHASES, STEPS, det, SEED, TURN, gid,
                      weights=None if wkey is None else dict(wkey), epsilon=epsilon)
    for k in ("visits", "wins"):
        r[k].setflags(write=False)
    return r


def want(rule_set, b, det, gid, epsilon=DG.DEFAULT_EPSILON, weights=None):
    return _want(rule_set, b, det, gid, epsilon, _key(weights))


@functools.lru_cache(maxsize=None)
def unguided(rule_set, b, det, gid):
    return DR.search_one(roots(rule_set)[0][b], R, PHASES, STEPS, det, SEED, TURN, gid)


def to_gpu(rule_set, envs):
    D = _D()
    return D.state_from_host(fields_of(envs), D.make_rules(**DR.RULE_SETS[rule_set]), seed=5)


def search(env, det, game_id=None, **kw):
    kw = dict(dict(max_phases=PHASES, rollout_steps=STEPS), **kw)
    out = _D().guided_rollout_policy(env, kw.pop("rollouts", R), determinize=bool(det), seed=SEED, turn=TURN,
                                     game_id=game_id, summary=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def assert_equal(got, b, w, what):
    action, value, visits, wins, turns, decided = got
    assert int(action[b]) == w["action"], (what, int(action[b]), w["action"])
    assert np.array_equal(visits[b], w["visits"]), (what, "visits", np.flatnonzero(visits[b] != w["visits"]))
    assert np.array_equal(wins[b], w["wins"]), (what, "wins", np.flatnonzero(wins[b] != w["wins"]))
    assert value[b].tobytes() == np.float32(w["value"]).tobytes(), (what, float(value[b]), float(w["value"]))
    assert int(turns[b]) == w["turns"], (what, int(turns[b]), w["turns"])
    assert int(decided[b]) == w["decided"], (what, int(decided[b]), w["decided"])


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_search_equals_the_restatement_bit_for_bit(cuda, rule_set, det):
    envs, tags = roots(rule_set)
    got = search(to_gpu(rule_set, envs), det)
    searched = differ = 0
    for b, ts in enumerate(tags):
        w = want(rule_set, b, det, b)
        assert_equal(got, b, w, (rule_set, det, b, ts))
        searched += len(w["sets"]) > 1
        u = unguided(rule_set, b, det, b)
        differ += w["turns"] != u["turns"] or not np.array_equal(w["wins"], u["wins"])
        if "forced" in ts or "stuck" in ts:
            assert not got[2][b].any() and got[1][b] == 0 and got[5][b] == 0
    assert searched >= 3
    assert differ >= 2           # the guided playouts are not the random ones: the comparison tells the two apart


@pytest.mark.parametrize("epsilon,weights", [(0.0, None), (0.125, NEGATIVE)], ids=["epsilon0", "negative"])
def test_other_epsilons_and_weights(cuda, epsilon, weights):
    rule_set = "selfplay_4p_teams"
    envs, tags = roots(rule_set)
    got = search(to_gpu(rule_set, envs), 1, epsilon=epsilon, weights=weights)
    differ = 0
    for b, ts in enumerate(tags):
        w = want(rule_set, b, 1, b, epsilon, weights)
        assert_equal(got, b, w, (epsilon, b, ts))
        d = want(rule_set, b, 1, b)
        differ += w["turns"] != d["turns"] or not np.array_equal(w["wins"], d["wins"])
    assert differ >= 1           # and not the default configuration's playouts either


def _batch67(rule_set):
    envs, _ = roots(rule_set)
    return [envs[(i * 3 + 1) % len(envs)] for i in range(67)]


def test_epsilon_one_is_rollout_policy_byte_for_byte(cuda):
    """67 games, rollout_steps = 60, R = 3: every shared output equals rollout_policy's; no restatement involved."""
    D = _D()
    rule_set = "selfplay_4p_teams"
    env = to_gpu(rule_set, _batch67(rule_set))
    gid = torch.arange(67, dtype=torch.int32) * 7 + 3
    kw = dict(max_phases=PHASES, rollout_steps=60, determinize=True, seed=SEED, turn=TURN, game_id=gid, summary=True)
    a = D.rollout_policy(env, 3, **kw)
    b = D.guided_rollout_policy(env, 3, epsilon=1.0, **kw)
    torch.cuda.synchronize()
    for x, y in zip(a, b[:5]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    visits, wins, decided = b[2].cpu().numpy(), b[3].cpu().numpy(), b[5].cpu().numpy()
    assert visits.any() and decided.any()
    assert (decided <= visits.sum(1)).all() and (decided >= np.abs(wins).max(1)).all()
    assert (decided % 2 == np.abs(wins.sum(1)) % 2).all()         # decided = #(+1) + #(-1), the wins' sum = their difference
    # and the default epsilon plays other playouts on the same batch
    c = D.guided_rollout_policy(env, 3, **kw)
    assert not torch.equal(c[4], b[4])


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
    # the other games of the batch are the same roots under other ids: the same root at two positions with two ids
    # draws other random numbers (shown on the rollout turns of the searched roots)
    same_root = [(i, j) for i in range(n) for j in range(i + 1, n)
                 if i not in (0, 5, 63) and j not in (0, 5, 63) and (i * 3 + 1) % len(envs) == (j * 3 + 1) % len(envs)]
    assert any(got[4][i] != got[4][j] for i, j in same_root)


def test_hidden_cards_do_not_reach_the_result(cuda):
    """tests/test_gpu_dog_rollout.py's ``spread`` construction: two roots that differ only in how the hidden cards are
    spread over the non-observers' hands, their swap choices and the deck give identical outputs."""
    rule_set = "selfplay_4p_teams"
    envs, tags = roots(rule_set)
    pick = [b for b, ts in enumerate(tags) if "joker" in ts or "swap_partial" in ts or "partner" in ts]
    assert len(pick) >= 3
    base = [envs[b] for b in pick]
    spread = [DR.determinize(e, 0xABCDEF12345 + b) for b, e in zip(pick, base)]
    for e, s in zip(base, spread):
        assert not np.array_equal(e.hands, s.hands) or not np.array_equal(e.deck, s.deck)
        assert np.array_equal(DR.hidden_multiset(e), DR.hidden_multiset(s))
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


def test_batch_sizes_one_and_sixty_seven(cuda):
    rule_set = "selfplay_4p_teams"
    envs, tags = roots(rule_set)
    x = next(b for b, ts in enumerate(tags) if "joker" in ts)
    got = search(to_gpu(rule_set, [envs[x]]), 1, game_id=torch.tensor([x], dtype=torch.int32))
    assert_equal(got, 0, want(rule_set, x, 1, x), "batch of one")
    batch = _batch67(rule_set)
    ids = [(i * 3 + 1) % len(envs) for i in range(67)]           # each game under its root's fixture id
    got = search(to_gpu(rule_set, batch), 1, game_id=torch.tensor(ids, dtype=torch.int32))
    for i in range(67):
        assert_equal(got, i, want(rule_set, ids[i], 1, ids[i]), ("batch of 67", i))


def test_empty_batch_launches_nothing(cuda):
    from exploring_muzero_on_dog_amd import lib as L
    D = _D()
    cfg = L.MuzDogGuidedCfg(L.MuzDogRolloutCfg(R, PHASES, STEPS, 1, SEED, TURN),
                            (ctypes.c_int32 * 6)(*DG.DEFAULT_WEIGHTS), 0.125)
    rules = D.make_rules(**DR.RULE_SETS["selfplay_4p_teams"])
    soa = L.MuzDogSoA()
    soa.stride = 0
    torch.cuda.synchronize()
    rc = L.load().muz_dog_guided_rollout_search(rules, ctypes.byref(cfg), soa, None, None, None, None, None, None,
                                                None, 0, None, 0, L.stream_ptr())
    assert rc == L.MUZ_OK
    torch.cuda.synchronize()
