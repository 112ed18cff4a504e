"""The DOG greedy agent (csrc/dog_greedy.hip, dog.greedy_policy, dog.afterstate_features, the 'greedy_agent' seat of
evaluate.py), everything that needs no GPU: the restatement (tests/_dog_greedy.py) on the fixture roots and on
hand-checked positions, its choice rules, the near-tie census of the cases the GPU test compares, its strength against
random play in the oracle, muz_dog_greedy_action's refusals (all checks come before the launch, so they run on a host
without a GPU) and the Python entry points."""
import ctypes
import os

import numpy as np
import pytest

from oracle import dog as dg
from oracle import evaluate as oe
from tests import _dog_greedy as G
from tests import _dog_rollout as DR
from tests.make_dog_greedy_roots import tags_of, wanted_tags
from tests.test_oracle_golden import DOG_CASES, dog_env_from_case

RULE_SETS = sorted(G.RULE_SETS)
EVAL_DOG_RULES = dict(enable_teams=True, enable_initial_free_pin=False, enable_circular_board=True,
                      enable_friendly_fire=True, enable_start_blocking=True, enable_jump_in_goal_area=False,
                      must_traverse_start=True, disable_swapping=False, disable_hot_seven=False, disable_joker=False)


def _tagged(tag):
    out = []
    for rs in RULE_SETS:
        envs, tags = G.load_roots(rs)
        out += [e for e, ts in zip(envs, tags) if tag in ts]
    return out


# ---- the fixture ----------------------------------------------------------------------------------------------------
def test_fixture_covers_the_kinds_of_root_and_candidate():
    assert os.path.getsize(G.ROOTS) < 64 * 1024
    have = set()
    for rs in RULE_SETS:
        envs, tags = G.load_roots(rs)
        assert len(envs) >= 8
        for env, ts in zip(envs, tags):
            assert sorted(ts) == sorted(tags_of(env))
            assert np.array_equal(env.board, dg.set_pins_on_board(env.board, env.pins))
            have |= set(ts)
    assert wanted_tags() <= have, wanted_tags() - have
    assert any(len(DR.candidates(e)) >= 60 for e in _tagged("many"))
    # with teams, a mover who has finished and plays the partner's pins
    assert any(e.rules["enable_teams"] and dg.sub_player(e) == (e.current_player + 2) % 4 for e in _tagged("partner"))


def test_defaults_are_the_ones_named():
    assert G.GREEDY_DEFAULTS == dict(advance=1, setback=1, goal=20, out=15, hit=10, win=1000, temperature=0.25)
    assert G.weights_of() == ([1, 1, 20, 15, 10, 1000], np.float32(0.25))
    assert G.weights_of(dict(hit=-3, temperature=0))[0][4] == -3


# ---- progress and features ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_prog_is_calculate_progress_an_exact_integer(rule_set):
    for env in G.load_roots(rule_set)[0]:
        for p in range(env.num_players):
            v = oe.calculate_progress(env, p)
            assert float(v) == G.prog(env, p) and float(v).is_integer()


def _case(kind, source, action):
    c = next(c for c in DOG_CASES[kind] if c["source"] == source)
    env = dog_env_from_case(c)
    hands = np.zeros_like(env.hands)
    hands[env.current_player] = 1                       # one of every card: the move's card is in the hand
    env = env.replace(hands=hands, phase=0)
    assert dg.valid_actions(env)[action]
    return env


def test_features_of_hand_checked_positions():
    """Two players, so ME = {mover}, OP = {the other}; calculate_progress rotates by 40 // 2 = 20 cells per seat.

    DOG/test.py:52  seat 0 (all pins home) leaves home with a 13 onto cell 0, where seat 1's pin stands.
      seat 0: rotated pins -6 -6 -6 -6 -> 46 + 47 + 48 + 49 = 190; after -6 -6 -6 -1 -> 41 + 47 + 48 + 49 = 185.
      seat 1: pins 6 14 44 0 -> rotated 25 33 40 19 -> 0 + 8 + 17 + 24 = 49; the pin on 0 goes home:
              -6 25 33 40 -> 0 + 8 + 17 + 49 = 74.
      advance 5, setback 25, goal 0, out 1, hit 1, win 0.
    DOG/test.py:559 seat 0 swaps its pin on 1 with seat 1's pin on 10.
      seat 0: -1 1 41 38 -> rotated -6 0 41 37 -> 0 + 3 + 42 + 49 = 94; after (10 -> 9) 0 + 3 + 33 + 49 = 85.
      seat 1: 6 14 44 10 -> 25 33 40 29 -> 0 + 8 + 13 + 18 = 39; after (1 -> 20) 0 + 8 + 17 + 23 = 48.
      advance 9, setback 9, nothing else.
    DOG/test.py:814 (must_traverse_start off) seat 0 moves its pin on 37 seven cells to 4, over its own pin on 1 and
      seat 1's pin on 2: both go home.
      seat 0: 37 36 41 1 -> 0 + 3 + 6 + 42 = 51; after 4 36 41 -1 -> rotated 4 36 41 -6 -> 0 + 4 + 38 + 49 = 91.
      seat 1: 9 2 45 12 -> 29 22 41 32 -> 0 + 8 + 13 + 21 = 42; after (2 -> home) 0 + 8 + 13 + 49 = 70.
      advance -40, setback 28, goal 0, out -1 (the friendly hit), hit 1, win 0."""
    leave = 396 + 344 + 2 * 12 + dg.NORMAL_MOVES.index(13)
    env = _case("normal_move", "DOG/test.py:52", leave)
    assert [G.prog(env, 0), G.prog(env, 1)] == [190, 49]
    assert G.features_of(env, leave) == [5, 25, 0, 1, 1, 0]
    swap = 396 + 1 * 56 + 10
    env = _case("swap_move", "DOG/test.py:559", swap)
    assert [G.prog(env, 0), G.prog(env, 1)] == [94, 39]
    assert G.features_of(env, swap) == [9, 9, 0, 0, 0, 0]
    seven = 396 + 224 + [tuple(d) for d in dg.DISTS_7_4.tolist()].index((7, 0, 0, 0))
    env = _case("hot7_move", "DOG/test.py:814", seven)
    assert [G.prog(env, 0), G.prog(env, 1)] == [51, 42]
    assert G.features_of(env, seven) == [-40, 28, 0, -1, 1, 0]
    # the joker copy of a move has the move's features
    assert G.features_of(env, seven - 396) == [-40, 28, 0, -1, 1, 0]


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_illegal_actions_score_int32_min_and_have_no_features(rule_set):
    envs, tags, roots = G.batch_roots(rule_set)
    for env, (C, F) in zip(envs, roots):
        r = G.greedy_one(env, None, 1, 0, 0, root=(C, F))
        out = np.ones(G.A, bool)
        out[C] = False
        assert (r["scores"][out] == G.INT32_MIN).all() and not r["features"][out].any()
        assert (r["scores"][C] > G.INT32_MIN).all()
        assert np.abs(F).max(initial=0) < 1000
        if env.done or not C:
            assert r["action"] == -1
        else:
            assert r["action"] in C


def test_sides():
    teams = G.load_roots("selfplay_4p_teams")[0][0]
    assert G.sides(teams.replace(current_player=3)) == ([1, 3], [0, 2])
    solo = G.load_roots("selfplay_4p_noteams")[0][0]
    assert G.sides(solo.replace(current_player=3)) == ([3], [0, 1, 2])
    three = G.load_roots("exotic_3p")[0][0]
    assert G.sides(three.replace(current_player=1)) == ([1], [0, 2])


# ---- the choice -------------------------------------------------------------------------------------------------------
def test_a_winning_candidate_is_chosen():
    roots = _tagged("win")
    assert roots
    for env in roots:
        C, F = G.evaluate_root(env)
        for temperature in (0.0, 0.25):
            for gid in range(8):
                a = G.greedy_one(env, dict(temperature=temperature), 7, 5, gid, root=(C, F))["action"]
                assert F[a, 5] == 1, (temperature, gid, a)


def test_swap_phase_roots_score_every_card_alike_and_sample_by_game_id():
    roots = _tagged("swap_phase")
    assert roots
    for env in roots:
        C, F = G.evaluate_root(env)
        assert C and min(C) >= 792 and not F.any()
        r = G.greedy_one(env, None, 7, 5, 0, root=(C, F))
        assert (r["scores"][C] == 0).all()
        if len(C) > 1:
            seen = {G.greedy_one(env, None, 7, 5, gid, root=(C, F))["action"] for gid in range(32)}
            assert len(seen) > 1 and seen <= set(C)
        assert G.greedy_one(env, dict(temperature=0), 7, 5, 3, root=(C, F))["action"] == C[0]


def test_temperature_zero_takes_the_first_argmax():
    sc = np.full(G.A, G.INT32_MIN, np.int32)
    C = [3, 9, 400, 791]
    sc[C] = [5, 7, 7, -2]
    assert G.choose(C, sc, 0.0, 1, 2, 3) == 9
    sc[C] = [-4, -4, -4, -4]
    assert G.choose(C, sc, 0.0, 1, 2, 3) == 3
    assert G.choose([], sc, 0.0, 1, 2, 3) == -1 and G.choose([], sc, 0.25, 1, 2, 3) == -1
    # a sampled choice: the first strictly greatest v; with one overwhelming score, that action under every key
    sc[C] = [0, 0, 1000, 0]
    assert {G.choose(C, sc, 0.25, s, t, g) for s in range(3) for t in range(3) for g in range(3)} == {400}
    # and at a high temperature the draw decides: several actions over the keys, never one outside C
    seen = {G.choose(C, sc, 32767.0, 1, t, 0) for t in range(64)}
    assert len(seen) > 1 and seen <= set(C)


def test_gumbel_is_the_scripted_agents_draw():
    """policy_gumbel(key, a) for a < 24 is oracle/evaluate.py's draw of the det and classic scripted agents."""
    want = oe.policy_gumbel(77, 5, 9)
    key = G.policy_key(77, 5, 9)
    got = np.array([G.policy_gumbel(key, a) for a in range(24)], np.float32)
    assert got.tobytes() == want.tobytes()
    assert len({float(G.policy_gumbel(key, a)) for a in range(806)}) > 790


def test_near_ties_stay_within_the_cap():
    """The census of the cases tests/test_gpu_dog_greedy.py compares at temperature 0.25: a case whose two largest v
    are within 4 ulp may go either way under the device's logf and is excused there; at most 1 % may be."""
    cases = [c for rs in RULE_SETS for c in G.sampled_cases(rs)]
    near = [c for c in cases if c[4]]
    assert len(cases) == 4 * sum(len(G.batch_roots(rs)[0]) for rs in RULE_SETS) and len(cases) >= 4 * (24 + 17)
    assert len(near) <= G.NEAR_TIE_CAP * len(cases), (len(near), len(cases))
    # the margin itself: equal values are a near tie, values a part in a thousand apart are not
    sc = np.full(G.A, G.INT32_MIN, np.int32)
    sc[[1, 2]] = [0, 4000]
    assert not G.near_tie([1, 2], sc, 0.25, 1, 2, 3) and not G.near_tie([1], sc, 0.25, 1, 2, 3)


# ---- strength ---------------------------------------------------------------------------------------------------------
def test_greedy_beats_random_in_the_oracle():
    """16 oracle games under evaluate.DOG_RULES, seats 0 + 2 the greedy agent with its defaults, seats 1 + 3
    engine_random_action, starting player game % 4.  The bar is derived: the smallest k with
    P(Bin(16, 1/2) >= k) < 1e-3, which is 15."""
    games, seed = 16, 5
    need = G.binomial_bar(games)
    assert need == 15 and G.binomial_bar(256) == 154
    wins = turns = 0
    for game in range(games):
        keys = dg.engine_shuffle_keys(seed, game)
        env = dg.env_reset(num_players=4, starting_player=game % 4, shuffle_keys=keys, **EVAL_DOG_RULES)
        t = 0
        while not env.done and t < 2000:
            if env.current_player in (0, 2):
                a = G.greedy_one(env, None, seed, t, game)["action"]
            else:
                a = dg.engine_random_action(dg.valid_actions(env), seed, game, t)
            env = dg.no_step(env, shuffle_keys=keys)[0] if a < 0 else dg.env_step(env, a, shuffle_keys=keys)[0]
            t += 1
        wins += bool(env.done and dg.get_winner(env, env.board)[0])
        turns += t
    print(f"greedy (seats 0 + 2) vs random in the oracle: {wins} of {games} wins, {turns / games:.0f} turns per game")
    assert wins >= need


# ---- the C entry point's refusals (no launch) -------------------------------------------------------------------------
class _Call:
    """muz_dog_greedy_action with never-dereferenced dummy pointers: every case here must return before the launch."""

    FIELDS = ("board", "pins", "deck", "hands", "swap_choices", "current_player", "round_starter", "phase", "hand_size",
              "reward", "done", "deal")

    def __init__(self):
        from exploring_muzero_on_dog_amd import dog as D
        from exploring_muzero_on_dog_amd import lib as L
        self.L, self.D, self.so = L, D, L.load()
        self.buf = (ctypes.c_char * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.rules = D.make_rules(**G.RULE_SETS["selfplay_4p_teams"])

    def soa(self, n=1, null=None):
        s = self.L.MuzDogSoA()
        for name in self.FIELDS:
            setattr(s, name, None if name == null else self.p)
        s.stride = n
        return s

    def cfg(self, w=(1, 1, 20, 15, 10, 1000), temperature=0.25):
        return self.L.MuzDogGreedyCfg((ctypes.c_int32 * 6)(*w), temperature, 1, 0)

    def __call__(self, cfg="default", n=1, rules="dog", null=None, soa=None):
        P = [self.p] * 4   # game_id, action, scores, features
        if null is not None:
            P[null] = None
        c = self.cfg() if cfg == "default" else cfg
        return self.so.muz_dog_greedy_action(self.rules if rules == "dog" else rules,
                                             ctypes.byref(c) if c is not None else None,
                                             self.soa(n) if soa is None else soa, P[0], P[1], P[2], P[3], n, None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_cfg_layout_matches_the_header():
    from exploring_muzero_on_dog_amd import lib as L
    c = L.MuzDogGreedyCfg
    assert (c.w.offset, c.temperature.offset, c.seed.offset, c.turn.offset) == (0, 24, 32, 40)
    assert ctypes.sizeof(c) == 48


def test_action_refuses_weights_and_temperatures_out_of_range(call):
    L = call.L
    for i in range(6):
        for bad in (-32769, 32768, 2 ** 31 - 1):
            w = [0] * 6
            w[i] = bad
            assert call(call.cfg(w=w)) == L.MUZ_E_INVALID
            assert call(call.cfg(w=w), n=0) == L.MUZ_E_INVALID
    for t in (-0.25, float("inf"), float("nan"), -float("inf")):
        assert call(call.cfg(temperature=t)) == L.MUZ_E_INVALID
        assert call(call.cfg(temperature=t), n=0) == L.MUZ_E_INVALID
    for w in ([-32768] * 6, [32767] * 6):                     # the limits pass on to the next check (a null action)
        assert call(call.cfg(w=w, temperature=0.0), null=1) == L.MUZ_E_INVALID
        assert call(call.cfg(w=w, temperature=0.0), n=0, null=1) == L.MUZ_OK


def test_action_refuses_null_pointers(call):
    L = call.L
    assert call(None) == L.MUZ_E_INVALID
    assert call(rules=None) == L.MUZ_E_INVALID
    assert call(n=-1) == L.MUZ_E_INVALID
    assert call(n=2, soa=call.soa(1)) == L.MUZ_E_INVALID               # fewer games in the state than asked for
    assert call(null=1) == L.MUZ_E_INVALID                             # action; game_id, scores, features may be null
    for name in _Call.FIELDS:
        assert call(soa=call.soa(1, null=name)) == L.MUZ_E_INVALID, name
    assert call(n=0, null=1, soa=call.soa(0, null="board")) == L.MUZ_OK   # an empty batch needs nothing


def test_action_refuses_the_rules_the_dog_entry_points_refuse(call):
    L, D = call.L, call.D
    kw = G.RULE_SETS["selfplay_4p_teams"]
    for bad in (dict(disable_joker=True), dict(disable_hot_seven=True), dict(disable_swapping=True)):
        assert call(rules=D.make_rules(**{**kw, **bad})) == L.MUZ_E_UNSUPPORTED


# ---- the Python entry points -------------------------------------------------------------------------------------------
def test_python_entry_points():
    import inspect

    from exploring_muzero_on_dog_amd import dog as D
    from exploring_muzero_on_dog_amd import evaluate as EV
    assert D.GREEDY_DEFAULTS == G.GREEDY_DEFAULTS and D.GREEDY_FEATURES == G.FEATURES
    assert EV.GREEDY_AGENT == "greedy_agent" and EV.DOG_RULES == EVAL_DOG_RULES
    assert EV._seat(EV._Dog, "greedy_agent", 0, 0, "cpu") == EV.GREEDY_AGENT
    assert EV._Game.GREEDY_SEAT is None and EV._Dog.GREEDY_SEAT == EV.GREEDY_AGENT
    assert EV._Det.GREEDY_SEAT is None and EV._Classic.GREEDY_SEAT is None
    assert EV._rollout_workspace(EV._Dog, ["greedy_agent", "random_agent"] * 2, 4, "cpu") is None   # no workspace
    for game in (EV._Det, EV._Classic):
        with pytest.raises(ValueError, match="greedy agent") as e:
            EV._seat(game, "greedy_agent", 0, 0, "cpu")
        assert "'rule_based_agent'" in str(e.value)
        assert EV._seat(game, "rule_based_agent", 0, 0, "cpu") == "rule_based_agent"
    with pytest.raises(ValueError) as e:
        EV._seat(EV._Dog, "rule_based_agent", 0, 0, "cpu")
    assert str(e.value) == ("MuZero_DOG/evaluate_agent.py's rule-based agent reshapes the 806-action mask to (4, 6) and "
                            "cannot run; use 'random_agent' or a MuZero agent")
    with pytest.raises(TypeError, match="DOG state"):
        D.greedy_policy(object(), seed=0, turn=0)
    with pytest.raises(TypeError, match="DOG state"):
        D.afterstate_features(object())
    with pytest.raises(TypeError):
        D.greedy_policy(None)                 # seed and turn are required: the draw is keyed by them
    sig = inspect.signature(D.greedy_policy)
    assert [sig.parameters[k].default for k in ("weights", "temperature", "game_id", "summary")] == \
        [None, None, None, False]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[1:])
    sig = inspect.signature(EV.evaluate_agent_parallel_dog)
    assert sig.parameters["greedy"].default is None
    assert sig.parameters["greedy"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [sig.parameters[k].default for k in ("rollouts", "rollout_steps", "determinize")] == [4, 300, True]
