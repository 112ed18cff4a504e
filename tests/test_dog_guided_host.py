"""The DOG rollout agent with greedy-guided playouts (csrc/dog_guided.hip, dog.guided_rollout_policy, the
'guided_rollout_agent' seat of evaluate.py), everything that needs no GPU: the restatement tests/_dog_guided.py on the
fixture roots (epsilon 1 is the rollout agent, the argmax-set choice, the swap phase, the census of greedy turns with
ties, the mid-game playout that decides where the random one hits the cap), muz_dog_guided_rollout_search's refusals
(all checks come before any launch, so they run on a host without a GPU), the cfg layout and the refusals of the Python
entry points."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest

from oracle import detmadn as dm
from oracle import dog as dg
from oracle import evaluate as oe
from oracle import root_noise as rn
from tests import _dog_greedy as DGR
from tests import _dog_guided as DG
from tests import _dog_rollout as DR

RULE_SETS = sorted(DR.RULE_SETS)
R, PHASES, STEPS, SEED, TURN = 2, 3, 24, 11, 3          # tests/test_gpu_dog_rollout.py's sizes
F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "muz.h")


def _tagged(rule_set, tag):
    envs, tags = DR.load_roots(rule_set)
    return [e for e, ts in zip(envs, tags) if tag in ts]


@functools.lru_cache(maxsize=None)
def _census(rule_set):
    """The fixture searches of one rule set at the default epsilon and weights -> (results, census of their turns)."""
    cen = DG.new_census()
    envs, _ = DR.load_roots(rule_set)
    return [DG.search_one(e, R, PHASES, STEPS, 1, SEED, TURN, b, census=cen) for b, e in enumerate(envs)], cen


# ---- the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_epsilon_one_is_the_rollout_agent(rule_set):
    envs, _ = DR.load_roots(rule_set)
    searched = 0
    for b, e in enumerate(envs):
        cen = DG.new_census()
        g = DG.search_one(e, R, PHASES, STEPS, 1, SEED, TURN, b, epsilon=1.0, census=cen)
        u = DR.search_one(e, R, PHASES, STEPS, 1, SEED, TURN, b)
        assert g["action"] == u["action"] and g["turns"] == u["turns"] and g["sets"] == u["sets"]
        assert F32(g["value"]).tobytes() == F32(u["value"]).tobytes()
        assert np.array_equal(g["visits"], u["visits"]) and np.array_equal(g["wins"], u["wins"])
        assert cen["greedy"] == cen["swap"] == cen["single"] == 0          # every turn with a legal action explored
        assert 0 <= g["decided"] <= int(g["visits"].sum())
        assert g["decided"] >= int(np.abs(g["wins"]).max(initial=0))
        searched += len(u["sets"]) > 1
    assert searched >= 3


def test_defaults_are_the_ones_named():
    assert DG.DEFAULT_WEIGHTS == (1, 1, 20, 15, 10, 1000) and DG.weights_of() == list(DG.DEFAULT_WEIGHTS)
    assert DG.weights_of(dict(goal=-5)) == [1, 1, -5, 15, 10, 1000]
    assert F32(DG.DEFAULT_EPSILON) == DG.DEFAULT_EPSILON == 0.125                 # exact in float32
    with pytest.raises(AssertionError):
        DG.weights_of(dict(temperature=0.25))


def test_explore_stream_is_new():
    from tests.test_gpu_env_round import STREAM as DET_RANDOM_STREAM      # det-MADN's random round (the module's name for it)
    consts = {DG.EXPLORE_STREAM, DR.ROLLOUT_STREAM, DR.DET_STREAM, dg.DEAL_STREAM, dg.RANDOM_ACTION_STREAM,
              oe.POLICY_STREAM, dm.START_STREAM, rn.ROOT_NOISE_STREAM, DET_RANDOM_STREAM}
    assert len(consts) == 9 and DG.EXPLORE_STREAM < 2 ** 40
    rseed = DR.rollout_seed(SEED, 0, TURN, 0)
    draws = [DG.explore_uniform(rseed, 0, t) for t in range(32)]
    assert all(0.0 <= u < 1.0 for u in draws) and len(set(draws)) == 32
    # its own stream: the explore draw of a turn is not the turn's action uniform
    acts = [dg._u24(dg._mix64(dg._game_key(rseed ^ dg.RANDOM_ACTION_STREAM, 0, t))) for t in range(32)]
    assert not set(draws) & set(acts)
    # one float32 compare: epsilon 1 always explores, epsilon 0 never does
    assert all(DG.explores(rseed, 0, t, 1.0) for t in range(32))
    assert not any(DG.explores(rseed, 0, t, 0.0) for t in range(32))
    share = sum(DG.explores(DR.rollout_seed(SEED, g, TURN, 0), g, t, 0.125) for g in range(64) for t in range(64))
    assert 0.09 < share / 4096 < 0.16                                   # 0.125 +- 7 sigma of Bin(4096, 1/8)


def test_argmax_set_takes_the_floor_u_m_th_tied_action():
    """A joker in hand makes every move legal twice, as the joker copy a < 396 and (where the card is held) the real
    copy a + 396; both lead to the same board, so they tie.  The choice is the floor(u_t |M|)-th member of the argmax
    set in action order, not the smallest one."""
    w = DG.weights_of()

    def argmax_set(e):
        C = DR.candidates(e)
        sc = DG.turn_scores(e, C, w)
        best = max(int(sc[a]) for a in C)
        return C, [a for a in C if int(sc[a]) == best]

    # a hand-built tie: the first play-phase root of the greedy agent's shared batch that holds no joker, with a joker
    # put into the mover's hand -- each of its moves is then legal as both copies, among other, worse candidates
    def with_joker(e):
        hands = e.hands.copy()
        hands[int(dg.sub_player(e)), 0] += 1
        return e.replace(hands=hands)

    envs = [with_joker(e) for e in DGR.batch_roots("selfplay_4p_teams")[0]
            if e.phase == 0 and not e.done and e.hands[int(dg.sub_player(e)), 0] == 0 and len(DR.candidates(e)) >= 2]
    env = next(e for e in envs if 2 <= len(argmax_set(e)[1]) < len(argmax_set(e)[0]))
    C, M = argmax_set(env)
    assert DG.choice_set(env, C, w, 0.0, 1, 0, 0) == M
    assert DG.choice_set(env, C, w, 1.0, 1, 0, 0) == C
    keys = dg.engine_shuffle_keys(0, 0)
    chosen = set()
    for t in range(24):
        rseed = DR.rollout_seed(SEED, 5, TURN, t)
        u = dg._u24(dg._mix64(dg._game_key(rseed ^ dg.RANDOM_ACTION_STREAM, 5, t)))
        k = min(int(F32(u) * F32(len(M))), len(M) - 1)
        assert DG.pick(M, rseed, 5, t) == M[k]
        after = DG.guided_turn(env, w, 0.0, rseed, 5, t, keys)
        want = dg.env_step(env, M[k], shuffle_keys=keys)[0]
        assert np.array_equal(after.pins, want.pins) and np.array_equal(after.hands, want.hands)
        chosen.add(M[k])
    assert len(chosen) >= 2                                             # ties are broken uniformly
    # all weights 0 make every candidate's score 0, so M = C without exploring
    assert DG.choice_set(env, C, [0] * 6, 0.0, 1, 0, 0) == C


def test_a_swap_phase_turn_is_uniform_over_the_cards():
    env = next(e for e in DR.load_roots("selfplay_4p_teams")[0] if e.phase == 1 and len(DR.candidates(e)) >= 2)
    C = DR.candidates(env)
    assert all(a >= 792 for a in C)
    for a in C:
        assert DGR.features_of(env, a) == [0] * 6                       # the card to hand over leaves the board alone
    assert not DG.turn_scores(env, C, DG.weights_of())[C].any()
    cen = DG.new_census()
    assert DG.choice_set(env, C, DG.weights_of(), 0.0, 1, 0, 0, cen) == C and cen["swap"] == 1
    picks = set()
    for t in range(32):
        rseed = DR.rollout_seed(SEED, 2, TURN, t)
        a = DG.pick(DG.choice_set(env, C, DG.weights_of(), 0.0, rseed, 2, t), rseed, 2, t)
        assert a == dg.engine_random_action(dg.valid_actions(env), rseed, 2, t)   # the random playout's own choice
        picks.add(a)
    assert len(picks) >= 2


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_fixture_searches_meet_greedy_turns_with_ties(rule_set):
    results, cen = _census(rule_set)
    assert cen["greedy"] >= 50 and cen["ties"] >= 5 and cen["explore"] >= 10, cen
    if rule_set == "selfplay_4p_teams":
        assert cen["swap"] >= 10, cen
    envs, _ = DR.load_roots(rule_set)
    differ = 0
    for b, (e, g) in enumerate(zip(envs, results)):
        u = DR.search_one(e, R, PHASES, STEPS, 1, SEED, TURN, b)
        assert int(g["visits"].sum()) == int(u["visits"].sum())         # the schedule is the same, the survivors not
        differ += g["turns"] != u["turns"] or not np.array_equal(g["wins"], u["wins"])
    assert differ >= 2                                                  # the guided playouts are other playouts


def _midgame(seed, turns=150):
    """The teams self-play game ``seed`` after ``turns`` engine-random turns."""
    keys = dg.engine_shuffle_keys(seed, 0)
    e = dg.env_reset(shuffle_keys=keys, **DR.RULE_SETS["selfplay_4p_teams"])
    for t in range(turns):
        a = dg.engine_random_action(dg.valid_actions(e), seed, 0, t)
        e = dg.no_step(e, shuffle_keys=keys)[0] if a < 0 else dg.env_step(e, a, shuffle_keys=keys)[0]
    return e


def test_a_mid_game_guided_playout_decides_where_the_random_one_hits_the_cap():
    """Root: game 1 after 150 random turns; rollout 0 of (seed 7, turn 150) on its first candidate, cap 300."""
    env = _midgame(1)
    assert not env.done
    a = DR.candidates(env)[0]
    assert DR.rollout(env, a, 7, 0, 150, 0, 300, 1) == (0, 300)
    z, t = DG.rollout(env, a, 7, 0, 150, 0, 300, 1)
    assert z != 0 and t < 300


# ---- the C entry point's refusals (no launch) -------------------------------------------------------------------------
def test_cfg_layout_matches_the_header():
    from exploring_muzero_on_dog_amd import lib as L
    c = L.MuzDogGuidedCfg
    assert (c.rollout.offset, c.w.offset, c.epsilon.offset) == (0, 32, 56)
    assert ctypes.sizeof(L.MuzDogRolloutCfg) == 32 and ctypes.sizeof(c) == 64
    text = open(HEADER).read()
    body = re.search(r"typedef struct muz_dog_guided_cfg \{(.*?)\} muz_dog_guided_cfg;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["muz_dog_rollout_cfg rollout", "int32_t w[6]", "float epsilon"]
    assert [n for n, _ in c._fields_] == ["rollout", "w", "epsilon"]
    assert "UNPINNED" in text[text.index("DOG guided rollout agent"):text.index("typedef struct muz_dog_guided_cfg")]


class _Call:
    """muz_dog_guided_rollout_search with never-dereferenced dummy pointers: every case must return before any launch."""

    FIELDS = ("board", "pins", "deck", "hands", "swap_choices", "current_player", "round_starter", "phase", "hand_size",
              "reward", "done", "deal")

    def __init__(self):
        from exploring_muzero_on_dog_amd import dog as D
        from exploring_muzero_on_dog_amd import lib as L
        self.L, self.D, self.so = L, D, L.load()
        self.buf = (ctypes.c_char * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.rules = D.make_rules(**DR.RULE_SETS["selfplay_4p_teams"])

    def soa(self, n=1, null=None):
        s = self.L.MuzDogSoA()
        for name in self.FIELDS:
            setattr(s, name, None if name == null else self.p)
        s.stride = n
        return s

    def cfg(self, w=DG.DEFAULT_WEIGHTS, epsilon=0.125, **kw):
        v = dict(rollouts=4, max_phases=10, rollout_steps=300, determinize=1, seed=1, turn=0)
        v.update(kw)
        r = self.L.MuzDogRolloutCfg(v["rollouts"], v["max_phases"], v["rollout_steps"], v["determinize"], v["seed"],
                                    v["turn"])
        return self.L.MuzDogGuidedCfg(r, (ctypes.c_int32 * 6)(*w), epsilon)

    def __call__(self, cfg="default", n=1, ws_bytes=1 << 40, rules="dog", null=None, soa=None, ws=None):
        P = [self.p] * 8   # game_id, action, value, visits, wins, rollout_turns, decided, workspace
        if null is not None:
            P[null] = None
        if ws is not None:
            P[7] = ws
        c = self.cfg() if cfg == "default" else cfg
        return self.so.muz_dog_guided_rollout_search(self.rules if rules == "dog" else rules,
                                                     ctypes.byref(c) if c is not None else None,
                                                     self.soa(n) if soa is None else soa, P[0], P[1], P[2], P[3], P[4],
                                                     P[5], P[6], n, P[7], ws_bytes, None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_search_refuses_weights_and_epsilons_out_of_range(call):
    L = call.L
    for i in range(6):
        for bad in (-32769, 32768, 2 ** 31 - 1):
            w = [0] * 6
            w[i] = bad
            assert call(call.cfg(w=w)) == L.MUZ_E_INVALID
            assert call(call.cfg(w=w), n=0) == L.MUZ_E_INVALID
    for eps in (-0.125, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert call(call.cfg(epsilon=eps)) == L.MUZ_E_INVALID, eps
        assert call(call.cfg(epsilon=eps), n=0) == L.MUZ_E_INVALID, eps
    for w in ([-32768] * 6, [32767] * 6):                    # the limits pass on to the next check (the workspace)
        for eps in (0.0, 1.0):
            assert call(call.cfg(w=w, epsilon=eps), ws_bytes=0) == L.MUZ_E_INVALID
            assert call(call.cfg(w=w, epsilon=eps), n=0, ws_bytes=0) == L.MUZ_OK


@pytest.mark.parametrize("change", [
    dict(rollouts=0), dict(rollouts=65), dict(max_phases=0), dict(max_phases=11), dict(rollout_steps=0),
    dict(rollout_steps=1001), dict(rollouts=-1)])
def test_search_refuses_a_rollout_cfg_out_of_range(call, change):
    assert call(call.cfg(**change)) == call.L.MUZ_E_INVALID
    assert call(call.cfg(**change), n=0) == call.L.MUZ_E_INVALID


def test_search_refuses_null_pointers_and_bad_workspaces(call):
    L = call.L
    assert call(None) == L.MUZ_E_INVALID
    assert call(rules=None) == L.MUZ_E_INVALID
    assert call(n=-1) == L.MUZ_E_INVALID
    assert call(n=2, soa=call.soa(1)) == L.MUZ_E_INVALID               # fewer games in the state than searched
    for i in (1, 2, 7):   # action, value, workspace; game_id (0), visits, wins, rollout_turns, decided (3-6) may be null
        assert call(null=i) == L.MUZ_E_INVALID, i
    for name in _Call.FIELDS:
        assert call(soa=call.soa(1, null=name)) == L.MUZ_E_INVALID, name
    want = call.so.muz_dog_rollout_bytes(17)                            # the rollout search's workspace, nothing more
    assert call(n=17, soa=call.soa(17), ws_bytes=want - 1) == L.MUZ_E_INVALID
    off = ctypes.c_void_p(ctypes.addressof(call.buf) + 4)               # not 16-byte aligned
    assert ctypes.addressof(call.buf) % 16 == 0
    assert call(ws=off) == L.MUZ_E_INVALID
    assert call(n=0, ws_bytes=0, null=7) == L.MUZ_OK                    # an empty batch needs nothing


def test_search_refuses_a_batch_whose_items_overflow_int32(call):
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
    assert EV.GUIDED_ROLLOUT_AGENT == "guided_rollout_agent" and D.GUIDED_EPSILON == DG.DEFAULT_EPSILON
    assert EV._seat(EV._Dog, "guided_rollout_agent", 0, 0, "cpu") == EV.GUIDED_ROLLOUT_AGENT
    assert EV._Game.GUIDED_SEAT is None and EV._Dog.GUIDED_SEAT == EV.GUIDED_ROLLOUT_AGENT
    assert EV._Det.GUIDED_SEAT is None and EV._Classic.GUIDED_SEAT is None
    with pytest.raises(ValueError, match="guided rollout agent") as e:
        EV._seat(EV._Det, "guided_rollout_agent", 0, 0, "cpu")
    assert "'mcts_agent'" in str(e.value) and "'rule_based_agent'" in str(e.value)
    with pytest.raises(ValueError, match="guided rollout agent") as e:
        EV._seat(EV._Classic, "guided_rollout_agent", 0, 0, "cpu")
    assert "'stochastic_mcts_agent'" in str(e.value) and "'rule_based_agent'" in str(e.value)
    # the seats and the messages that were there keep their text
    assert EV._NO_ROLLOUT_DET == ("the rollout agent (dog.rollout_policy) is DOG's: det-MADN's network-free seat is "
                                  "'mcts_agent'; its other named seats are 'rule_based_agent' and 'random_agent'")
    assert EV._rollout_workspace(EV._Dog, ["random_agent", "greedy_agent"] * 2, 4, "cpu") is None
    assert EV._rollout_workspace(EV._Det, ["random_agent"] * 4, 4, "cpu") is None
    with pytest.raises(ValueError, match="'epsilon' and 'weights'"):
        EV._guided_kwargs(dict(rollouts=2))
    assert EV._guided_kwargs(None) == {} and EV._guided_kwargs(dict(epsilon=0.5)) == dict(epsilon=0.5)
    sig = inspect.signature(EV.evaluate_agent_parallel_dog)
    assert sig.parameters["guided"].default is None
    assert sig.parameters["guided"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [sig.parameters[k].default for k in ("rollouts", "rollout_steps", "determinize")] == [4, 300, True]
    sig = inspect.signature(D.guided_rollout_policy)
    names = ["rollouts", "weights", "epsilon", "max_phases", "rollout_steps", "determinize", "game_id", "workspace",
             "summary"]
    assert [sig.parameters[k].default for k in names] == [4, None, 0.125, 10, 300, True, None, None, False]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    with pytest.raises(TypeError, match="DOG state"):
        D.guided_rollout_policy(object(), 4, seed=0, turn=0)
    with pytest.raises(TypeError):
        D.guided_rollout_policy(None, 4)      # seed and turn are required: the playouts are keyed by them
    rules = D.make_rules(**DR.RULE_SETS["selfplay_4p_teams"])
    env = D.DOGState.alloc(1, 4, rules, "cpu")
    with pytest.raises(ValueError, match="no temperature"):
        D.guided_rollout_policy(env, weights=dict(temperature=0.25), seed=0, turn=0)
    with pytest.raises(ValueError, match="unknown greedy weights"):
        D.guided_rollout_policy(env, weights=dict(speed=1), seed=0, turn=0)
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            D.guided_rollout_policy(env, epsilon=eps, seed=0, turn=0)
