"""The DOG greedy agent on the GPU (csrc/dog_greedy.hip through dog.greedy_policy / dog.afterstate_features) against
its definition, the NumPy restatement tests/_dog_greedy.py: features, scores and the temperature-0 action bit for bit;
the sampled action equal except at a near tie of the restatement's two largest values (the device's logf against
NumPy's: at most 4 ulp, at most 1 % of the cases, each printed).

The roots are the shared batch of tests/_dog_greedy.py (batch_roots): per rule set the roots of
tests/golden/dog_greedy_roots.json, then those of dog_rollout_roots.json; a root's game id is its position.  The
restatement's afterstate features are computed once per root and shared between the tests."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _dog_greedy as G
from tests.dog_states import fields_of

pytestmark = pytest.mark.gpu

RULE_SETS = sorted(G.RULE_SETS)
SEED, TURN = 11, 3
NEGATIVE = dict(advance=3, setback=-2, goal=-32768, out=32767, hit=-7, win=-1)   # a set with negative weights


def _D():
    from exploring_muzero_on_dog_amd import dog as D
    return D


def to_gpu(rule_set, envs):
    D = _D()
    return D.state_from_host(fields_of(envs), D.make_rules(**G.RULE_SETS[rule_set]), seed=5)


def greedy(env, cfg=None, seed=SEED, turn=TURN, game_id=None):
    v = dict(cfg or {})
    temperature = v.pop("temperature", None)
    out = _D().greedy_policy(env, weights=v, temperature=temperature, seed=seed, turn=turn, game_id=game_id,
                             summary=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def want(rule_set, b, cfg, seed=SEED, turn=TURN, gid=None):
    envs, _, roots = G.batch_roots(rule_set)
    return G.greedy_one(envs[b], cfg, seed, turn, b if gid is None else gid, root=roots[b])


@pytest.mark.parametrize("cfg", [None, NEGATIVE], ids=["defaults", "negative"])
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_features_scores_and_the_first_argmax_equal_the_restatement(cuda, rule_set, cfg):
    envs, tags, roots = G.batch_roots(rule_set)
    c0 = dict(cfg or {}, temperature=0.0)
    action, scores, features = greedy(to_gpu(rule_set, envs), c0)
    assert scores.dtype == np.int32 and features.dtype == np.int32 and features.shape == (len(envs), 806, 6)
    stepped = 0
    for b, ts in enumerate(tags):
        w = want(rule_set, b, c0)
        diff = int((features[b] != w["features"]).sum()) + int((scores[b] != w["scores"]).sum())
        assert diff == 0, (rule_set, b, ts, np.argwhere(features[b] != w["features"])[:4].tolist(),
                           np.flatnonzero(scores[b] != w["scores"])[:4].tolist())
        assert int(action[b]) == w["action"], (rule_set, b, ts, int(action[b]), w["action"])
        # legality: a candidate, or -1 exactly where the restatement has none
        assert (int(action[b]) in w["C"]) if w["C"] else int(action[b]) == -1
        stepped += len([a for a in w["C"] if a < 792])
    assert stepped >= 50      # not vacuous: the restatement steps 79 candidates in the smallest batch (exotic_3p)


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_sampled_action_equals_the_restatement_outside_near_ties(cuda, rule_set):
    envs, tags, roots = G.batch_roots(rule_set)
    cases = G.sampled_cases(rule_set)
    env = to_gpu(rule_set, envs)
    got = {(seed, turn): greedy(env, None, seed, turn)[0] for seed, turn in G.SAMPLE_KEYS}
    excused = []
    for b, seed, turn, a, near in cases:
        g = int(got[(seed, turn)][b])
        C = roots[b][0]
        assert (g in C) if C else g == -1
        if g != a:
            assert near, (rule_set, b, tags[b], seed, turn, g, a)
            excused.append((b, seed, turn, g, a))
    for e in excused:
        print("near tie excused (root, seed, turn, device, restatement):", rule_set, e)
    assert len(cases) == 4 * len(envs) and len(excused) <= G.NEAR_TIE_CAP * len(cases)
    # the draw is live: some root with several candidates changes its action over the four keys
    assert any(len({int(got[k][b]) for k in G.SAMPLE_KEYS}) > 1 for b in range(len(envs)))


def test_result_is_keyed_by_game_id_not_by_batch_position(cuda):
    rule_set = "selfplay_4p_teams"
    envs, tags, roots = G.batch_roots(rule_set)
    n = len(envs)
    perm = np.random.default_rng(1).permutation(n)
    ids = torch.arange(n, dtype=torch.int32)
    base = greedy(to_gpu(rule_set, envs), None, game_id=ids)
    moved = greedy(to_gpu(rule_set, [envs[i] for i in perm]), None, game_id=torch.from_numpy(perm.astype(np.int32)))
    for x, y in zip(base, moved):
        assert np.array_equal(x[perm], y)
    assert np.array_equal(base[0], greedy(to_gpu(rule_set, envs), None)[0])      # no ids: the positions
    # other ids: every root follows the restatement at ITS id, and some sampled action changes
    other = np.arange(n, dtype=np.int32) + 1000
    got = greedy(to_gpu(rule_set, envs), None, game_id=torch.from_numpy(other))[0]
    changed = 0
    for b in range(n):
        C, F = roots[b]
        w = want(rule_set, b, None, gid=int(other[b]))
        sc = w["scores"]
        assert int(got[b]) == w["action"] or G.near_tie(C, sc, 0.25, SEED, TURN, int(other[b])), b
        changed += int(got[b]) != int(base[0][b])
    assert changed >= 1


@pytest.mark.parametrize("n", [1, 67])
def test_batch_sizes(cuda, n):
    """One game, and 67 games (no multiple of a wave, of the waves of a workgroup or of the games per block)."""
    rule_set = "exotic_3p"
    envs, tags, roots = G.batch_roots(rule_set)
    pick = [(7 * i + 3) % len(envs) for i in range(n)]
    ids = torch.tensor(pick, dtype=torch.int32)
    action, scores, features = greedy(to_gpu(rule_set, [envs[b] for b in pick]), dict(temperature=0.0), game_id=ids)
    for i, b in enumerate(pick):
        w = want(rule_set, b, dict(temperature=0.0))
        assert int(action[i]) == w["action"] and np.array_equal(scores[i], w["scores"]) and \
            np.array_equal(features[i], w["features"]), (i, b)


def test_empty_batch_launches_nothing(cuda):
    from exploring_muzero_on_dog_amd import lib as L
    D = _D()
    cfg = L.MuzDogGreedyCfg((ctypes.c_int32 * 6)(1, 1, 20, 15, 10, 1000), 0.25, SEED, TURN)
    soa = L.MuzDogSoA()
    soa.stride = 0
    torch.cuda.synchronize()
    rc = L.load().muz_dog_greedy_action(D.make_rules(**G.RULE_SETS["selfplay_4p_teams"]), ctypes.byref(cfg), soa, None,
                                        None, None, None, 0, L.stream_ptr())
    assert rc == L.MUZ_OK
    torch.cuda.synchronize()


def test_state_is_untouched_and_afterstate_features_are_the_summary(cuda):
    D = _D()
    rule_set = "selfplay_4p_teams"
    envs, tags, roots = G.batch_roots(rule_set)
    env = to_gpu(rule_set, envs)
    fields = list(D.DOGState.ROWS) + list(D.DOGState.VECTORS)
    before = {k: getattr(env, k).clone() for k in fields}
    action, scores, features = greedy(env)
    feats = D.afterstate_features(env)
    plain = D.greedy_policy(env, seed=SEED, turn=TURN)                 # no summary: the action alone
    torch.cuda.synchronize()
    for k in fields:
        assert torch.equal(before[k], getattr(env, k)), k
    assert feats.dtype == torch.int32 and np.array_equal(feats.cpu().numpy(), features)
    assert plain.dtype == torch.int32 and np.array_equal(plain.cpu().numpy(), action)
    assert features.any()
