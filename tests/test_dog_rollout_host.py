"""The DOG rollout agent (csrc/dog_rollout.hip, dog.rollout_policy, the 'rollout_agent' seat of evaluate.py), everything
that needs no GPU: the restatement's pieces (tests/_dog_rollout.py) on the fixture roots, the halving schedule,
muz_dog_rollout_search's refusals (all checks come before any launch, so they run on a host without a GPU), the pinned
workspace size and the refusals of the Python entry points."""
import ctypes

import numpy as np
import pytest

from oracle import dog as dg
from tests import _dog_rollout as DR
from tests.make_dog_rollout_roots import tags_of, wanted_tags, winning_actions

RULE_SETS = sorted(DR.RULE_SETS)


def _tagged(rule_set, tag):
    envs, tags = DR.load_roots(rule_set)
    return [e for e, ts in zip(envs, tags) if tag in ts]


# ---- the fixture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_fixture_holds_the_kinds_of_root_the_tests_need(rule_set):
    envs, tags = DR.load_roots(rule_set)
    assert 4 <= len(envs) <= 7
    assert wanted_tags(rule_set) <= {t for ts in tags for t in ts}
    for env, ts in zip(envs, tags):
        assert sorted(ts) == sorted(tags_of(env))
        assert not env.done and len(DR.candidates(env)) <= 8
        assert np.array_equal(env.board, dg.set_pins_on_board(env.board, env.pins))


def test_rule_sets_are_the_ones_named():
    from tests.dog_states import RULE_SETS as DOG_SETS
    assert DR.RULE_SETS["selfplay_4p_teams"] == DOG_SETS["selfplay_4p_teams"]
    assert DR.RULE_SETS["exotic_3p"] == DOG_SETS["exotic_3p"]
    off = DR.RULE_SETS["selfplay_4p_noteams"]
    assert not off["enable_teams"] and {**off, "enable_teams": True} == DOG_SETS["selfplay_4p_teams"]


def test_streams_are_new():
    consts = {DR.ROLLOUT_STREAM, DR.DET_STREAM, dg.DEAL_STREAM, dg.RANDOM_ACTION_STREAM, 0x57A27C0DE5, 0x5DEECE66D,
              0x9011C7A6E47, 0xD37A11D0}
    assert len(consts) == 8
    keys = [(11, 3, 5, 0), (12, 3, 5, 0), (11, 4, 5, 0), (11, 3, 6, 0), (11, 3, 5, 1)]
    seeds = [DR.rollout_seed(*k) for k in keys]
    assert len(set(seeds)) == len(keys)
    draws = [DR.det_uniform(seeds[0], i) for i in range(16)]
    assert all(0.0 <= u < 1.0 for u in draws) and len(set(draws)) == 16


# ---- determinization ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_determinization_conserves_the_hidden_cards_and_touches_nothing_else(rule_set):
    envs, tags = DR.load_roots(rule_set)
    changed = 0
    for b, env in enumerate(envs):
        obs = DR.observers(env)
        assert env.current_player in obs and dg.sub_player(env) in obs
        for j in range(4):
            d = DR.determinize(env, DR.rollout_seed(11, b, 3, j))
            assert np.array_equal(DR.hidden_multiset(d), DR.hidden_multiset(env))
            assert (d.hands >= 0).all() and (d.deck >= 0).all()
            assert np.array_equal(d.hands.astype(int).sum(1), env.hands.astype(int).sum(1))      # every hand size
            for q in range(env.num_players):
                if q in obs:
                    assert np.array_equal(d.hands[q], env.hands[q]) and d.swap_choices[q] == env.swap_choices[q]
                else:
                    assert (d.swap_choices[q] >= 0) == (env.swap_choices[q] >= 0)
            for k in ("board", "pins"):
                assert np.array_equal(getattr(d, k), getattr(env, k))
            for k in ("current_player", "round_starter", "phase", "hand_size", "deal", "done", "reward"):
                assert getattr(d, k) == getattr(env, k)
            assert DR.candidates(d) == DR.candidates(env)          # the mover's options do not depend on hidden cards
            changed += not np.array_equal(d.hands, env.hands)
    assert changed >= len(envs)


def test_a_hidden_swap_choice_is_redrawn_with_the_hand():
    env = _tagged("selfplay_4p_teams", "swap_partial")[0]
    hidden = [q for q in DR.hidden_seats(env) if env.swap_choices[q] >= 0]
    assert hidden
    H = DR.hidden_multiset(env)
    assert H.sum() == env.deck.astype(int).sum() + sum(int(env.hands[q].astype(int).sum()) for q in DR.hidden_seats(env)) \
        + len(hidden)
    seen = {int(DR.determinize(env, DR.rollout_seed(1, 0, 0, j)).swap_choices[hidden[0]]) for j in range(24)}
    assert len(seen) > 1


def test_a_finished_team_player_observes_through_the_partner():
    env = _tagged("selfplay_4p_teams", "partner")[0]
    m = env.current_player
    assert dg.sub_player(env) == (m + 2) % 4 and DR.observers(env) == {m, (m + 2) % 4}
    assert DR.side_of(env) == m % 2
    assert DR.hidden_seats(env) == sorted({0, 1, 2, 3} - {m, (m + 2) % 4})
    solo = DR.load_roots("selfplay_4p_noteams")[0][0]
    assert DR.observers(solo) == {solo.current_player} and DR.side_of(solo) == solo.current_player


# ---- the halving schedule -------------------------------------------------------------------------------------------
def _scripted(scores):
    """A rollout whose outcome depends on the action alone: +1 / -1 / 0 by ``scores[a]`` (every visit the same)."""
    calls = []

    def fn(env, a, seed, game_id, turn, j, steps, det):
        calls.append((a, j))
        return scores.get(a, 0), 1
    return fn, calls


def test_halving_schedule_set_sizes_visits_and_ties():
    env = _tagged("selfplay_4p_teams", "joker")[0]
    C = DR.candidates(env)
    m = len(C)
    assert m >= 6
    scores = {C[1]: 1, C[4]: 1, C[2]: -1}
    fn, calls = _scripted(scores)
    r = DR.search_one(env, 2, 10, 24, 1, 0, 0, 0, rollout_fn=fn)
    sizes = [len(s) for s in r["sets"]]
    assert sizes[0] == m and sizes[-1] == 1
    for a, b in zip(sizes, sizes[1:]):
        assert b == (a + 1) // 2
    # equal visits within a phase, rollouts j = p R .. p R + R - 1 in phase p
    for p, S in enumerate(r["sets"][:-1]):
        for a in S:
            assert sorted(j for x, j in calls if x == a)[2 * p:2 * p + 2] == [2 * p, 2 * p + 1]
        later = set(r["sets"][p + 1])
        for a in set(S) - later:
            assert r["visits"][a] == 2 * (p + 1)
    # the tie rule: wins descending, then the smaller action; C[1] and C[4] tie at the top, C[2] is dropped first
    assert r["sets"][1][:2] == [C[1], C[4]] and C[2] not in r["sets"][1]
    assert r["sets"][1][2:] == [a for a in C if a not in (C[1], C[2], C[4])][:len(r["sets"][1]) - 2]
    assert r["action"] == C[1] and r["value"] == np.float32(1.0)
    assert r["turns"] == len(calls) == int(r["visits"].sum())
    assert DR.rank([5, 3, 9], {5: 0, 3: 0, 9: 1}) == [9, 3, 5]


def test_max_phases_cuts_the_schedule():
    env = _tagged("selfplay_4p_teams", "joker")[0]
    C = DR.candidates(env)
    fn, calls = _scripted({C[-1]: 1})
    r = DR.search_one(env, 3, 1, 24, 0, 0, 0, 0, rollout_fn=fn)
    assert [len(s) for s in r["sets"]] == [len(C), (len(C) + 1) // 2]
    assert r["action"] == C[-1] and all(r["visits"][a] == 3 for a in C) and r["value"] == np.float32(1.0)


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_forced_and_empty_roots_cost_nothing(rule_set):
    def never(*a):
        raise AssertionError("a forced root ran a rollout")
    forced = _tagged(rule_set, "forced")[0]
    r = DR.search_one(forced, 2, 3, 24, 1, 0, 0, 0, rollout_fn=never)
    assert r["action"] == DR.candidates(forced)[0] and not r["visits"].any() and r["value"] == 0 and r["turns"] == 0
    stuck = _tagged(rule_set, "stuck")[0]
    r = DR.search_one(stuck, 2, 3, 24, 1, 0, 0, 0, rollout_fn=never)
    assert r["action"] == -1 and not r["visits"].any() and r["value"] == 0
    done = stuck.replace(done=True)
    assert DR.search_one(done, 2, 3, 24, 1, 0, 0, 0, rollout_fn=never)["action"] == -1


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_the_winning_move_is_found_with_value_one(rule_set):
    env = next(e for e in _tagged(rule_set, "wins") if len(DR.candidates(e)) > 1)
    wins = winning_actions(env)
    assert wins
    r = DR.search_one(env, 2, 3, 24, 1, 11, 3, 0)
    assert r["action"] in wins and r["value"] == np.float32(1.0)
    z, t = DR.rollout(env, wins[0], 11, 0, 3, 0, 24, 1)
    assert (z, t) == (1, 0)                                    # decided by the root action: no random turn


def test_rollouts_cross_a_deal_within_the_cap():
    env = _tagged("selfplay_4p_teams", "deal")[0]
    z, t = DR.rollout(env, DR.candidates(env)[0], 11, 0, 3, 0, 24, 1)
    assert z in (-1, 0, 1) and 0 < t <= 24


# ---- the C entry point's refusals (no launch) -------------------------------------------------------------------------
class _Call:
    """muz_dog_rollout_search with never-dereferenced dummy pointers: every case here must return before any launch."""

    def __init__(self):
        from exploring_muzero_on_dog_amd import dog as D
        from exploring_muzero_on_dog_amd import lib as L
        self.L, self.D, self.so = L, D, L.load()
        self.buf = (ctypes.c_char * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.rules = D.make_rules(**DR.RULE_SETS["selfplay_4p_teams"])

    FIELDS = ("board", "pins", "deck", "hands", "swap_choices", "current_player", "round_starter", "phase", "hand_size",
              "reward", "done", "deal")

    def soa(self, n=1, null=None):
        s = self.L.MuzDogSoA()
        for name in self.FIELDS:
            setattr(s, name, None if name == null else self.p)
        s.stride = n
        return s

    def cfg(self, **kw):
        v = dict(rollouts=4, max_phases=10, rollout_steps=300, determinize=1, seed=1, turn=0)
        v.update(kw)
        return self.L.MuzDogRolloutCfg(v["rollouts"], v["max_phases"], v["rollout_steps"], v["determinize"], v["seed"],
                                       v["turn"])

    def __call__(self, cfg="default", n=1, ws_bytes=1 << 40, rules="dog", null=None, soa=None, ws=None):
        P = [self.p] * 7   # game_id, action, value, visits, wins, rollout_turns, workspace
        if null is not None:
            P[null] = None
        if ws is not None:
            P[6] = ws
        c = self.cfg() if cfg == "default" else cfg
        return self.so.muz_dog_rollout_search(self.rules if rules == "dog" else rules,
                                              ctypes.byref(c) if c is not None else None,
                                              self.soa(n) if soa is None else soa, P[0], P[1], P[2], P[3], P[4], P[5],
                                              n, P[6], ws_bytes, None)


@pytest.fixture(scope="module")
def call():
    return _Call()


ROLLOUT_BYTES = {1: 10752, 17: 165888, 4096: 39665920}


def test_rollout_bytes_are_pinned(call):
    """wins, visits and the candidate lists [n][806] int32, then the counts [n], the turns [n] and the offsets [n + 1],
    each block rounded up to 256 bytes; one byte less is MUZ_E_INVALID."""
    def up(x):
        return (x + 255) // 256 * 256
    for n, want in ROLLOUT_BYTES.items():
        assert want == 3 * up(n * 806 * 4) + 2 * up(n * 4) + up((n + 1) * 4)
        assert call.so.muz_dog_rollout_bytes(n) == want
        assert call(n=n, ws_bytes=want - 1) == call.L.MUZ_E_INVALID
    assert call.so.muz_dog_rollout_bytes(-1) == -1
    assert call.so.muz_dog_rollout_bytes(0) == 256


@pytest.mark.parametrize("change", [
    dict(rollouts=0), dict(rollouts=65), dict(max_phases=0), dict(max_phases=11), dict(rollout_steps=0),
    dict(rollout_steps=1001), dict(rollouts=-1)])
def test_search_refuses_a_cfg_out_of_range(call, change):
    assert call(call.cfg(**change)) == call.L.MUZ_E_INVALID
    assert call(call.cfg(**change), n=0) == call.L.MUZ_E_INVALID


def test_search_accepts_the_limits(call):
    for kw in (dict(rollouts=1, max_phases=1, rollout_steps=1), dict(rollouts=64, max_phases=10, rollout_steps=1000)):
        assert call(call.cfg(**kw), ws_bytes=0) == call.L.MUZ_E_INVALID      # the next check (the workspace) answers
        assert call(call.cfg(**kw), n=0, ws_bytes=0) == call.L.MUZ_OK


def test_search_refuses_null_pointers_and_bad_workspaces(call):
    L = call.L
    assert call(None) == L.MUZ_E_INVALID
    assert call(rules=None) == L.MUZ_E_INVALID
    assert call(n=-1) == L.MUZ_E_INVALID
    assert call(n=2, soa=call.soa(1)) == L.MUZ_E_INVALID               # fewer games in the state than searched
    for i in (1, 2, 6):            # action, value, workspace; game_id (0), visits, wins, rollout_turns (3-5) may be null
        assert call(null=i) == L.MUZ_E_INVALID, i
    for name in _Call.FIELDS:
        assert call(soa=call.soa(1, null=name)) == L.MUZ_E_INVALID, name
    off = ctypes.c_void_p(ctypes.addressof(call.buf) + 4)               # not 16-byte aligned
    assert ctypes.addressof(call.buf) % 16 == 0
    assert call(ws=off) == L.MUZ_E_INVALID
    assert call(n=0, ws_bytes=0, null=6) == L.MUZ_OK                    # an empty batch needs nothing


def test_search_refuses_a_batch_whose_items_overflow_int32(call):
    """The items of a phase (at most n * 806 * rollouts) are indexed in int32 with a grid stride of 2048."""
    L = call.L
    bad = call.D.make_rules(**{**DR.RULE_SETS["selfplay_4p_teams"], "disable_joker": True})
    for rollouts, most in ((64, 41630), (4, 666092)):
        assert most == (2 ** 31 - 1 - 2048) // (806 * rollouts)
        cfg = call.cfg(rollouts=rollouts)
        assert call(cfg, n=most + 1, soa=call.soa(most + 1)) == L.MUZ_E_INVALID
        assert call(cfg, n=most + 1, soa=call.soa(most + 1), rules=bad) == L.MUZ_E_INVALID
        assert call(cfg, n=most, soa=call.soa(most), rules=bad) == L.MUZ_E_UNSUPPORTED   # the largest batch passes on


def test_search_refuses_the_rules_the_dog_entry_points_refuse(call):
    L, D = call.L, call.D
    kw = DR.RULE_SETS["selfplay_4p_teams"]
    for bad in (dict(disable_joker=True), dict(disable_hot_seven=True), dict(disable_swapping=True)):
        assert call(rules=D.make_rules(**{**kw, **bad})) == L.MUZ_E_UNSUPPORTED


# ---- the Python entry points -------------------------------------------------------------------------------------------
def test_python_entry_points():
    from exploring_muzero_on_dog_amd import dog as D
    from exploring_muzero_on_dog_amd import evaluate as EV
    assert EV.ROLLOUT_AGENT == "rollout_agent"
    assert EV._seat(EV._Dog, "rollout_agent", 0, 0, "cpu") == EV.ROLLOUT_AGENT
    assert EV._Dog.ROLLOUT_SEAT == EV.ROLLOUT_AGENT and EV._Det.ROLLOUT_SEAT is None and EV._Classic.ROLLOUT_SEAT is None
    assert EV._Dog.ENV_SEAT is None                                       # the rollout seat is not an environment-search seat
    assert EV._mcts_workspace(EV._Dog, ["rollout_agent", "random_agent"] * 2, 4, 8, "cpu") is None
    assert EV._rollout_workspace(EV._Dog, ["random_agent"] * 4, 4, "cpu") is None
    assert EV._rollout_workspace(EV._Det, ["random_agent"] * 4, 4, "cpu") is None
    with pytest.raises(ValueError, match="'mcts_agent'"):
        EV._seat(EV._Det, "rollout_agent", 0, 0, "cpu")
    with pytest.raises(ValueError, match="'stochastic_mcts_agent'"):
        EV._seat(EV._Classic, "rollout_agent", 0, 0, "cpu")
    for name, text in (("mcts_agent", "no environment-model search kernel"), ("stochastic_mcts_agent", "chance nodes")):
        with pytest.raises(ValueError, match=text) as e:
            EV._seat(EV._Dog, name, 0, 0, "cpu")
        assert "rollout_agent" in str(e.value)
    with pytest.raises(TypeError, match="DOG state"):
        D.rollout_policy(object(), 4, seed=0, turn=0)
    with pytest.raises(TypeError):
        D.rollout_policy(None, 4)            # seed and turn are required: the rollouts are keyed by them
    import inspect
    sig = inspect.signature(EV.evaluate_agent_parallel_dog)
    assert [sig.parameters[k].default for k in ("rollouts", "rollout_steps", "determinize")] == [4, 300, True]
    sig = inspect.signature(D.rollout_policy)
    assert [sig.parameters[k].default for k in ("rollouts", "max_phases", "rollout_steps", "determinize")] == \
        [4, 10, 300, True]
