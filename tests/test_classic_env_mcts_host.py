"""The network-free MCTS agent for classic MADN (csrc/classic_env_mcts.hip, stochastic.env_stochastic_muzero_policy,
the 'stochastic_mcts_agent' seat), everything that needs no GPU: the restatement's pieces
(tests/_classic_env_mcts.py) on oracle/classic_madn.py states, the fixture of root states, muz_classic_mcts's refusals
(argument checks come before any launch, so they run on a host without a GPU) and the refusals of the Python entry
points."""
import ctypes

import numpy as np
import pytest

from oracle import classic_madn as cm
from tests import _classic_env_mcts as CM
from tests.make_classic_env_mcts_roots import tags_of, wanted_tags

RULE_SETS = list(CM.RULE_SETS)
ZERO = np.zeros(CM.A, np.float32)


def _lib():
    from exploring_muzero_on_dog_amd import lib as L
    return L


def _tagged(rule_set, tag):
    envs, tags = CM.load_roots(rule_set)
    return [e for e, ts in zip(envs, tags) if tag in ts]


def random_game_states(rule_set, seed, max_plies=6000):
    """Every state (its die thrown) of one seeded game under the rollout policy (it ends games: a winning pin when
    there is one)."""
    rng = np.random.default_rng(seed)
    env = cm.env_reset(**CM.RULE_SETS[rule_set])
    for _ in range(max_plies):
        if env.done:
            yield env
            return
        env = cm.throw_die(env, float(np.float32(rng.random())))
        yield env
        lm = CM.legal_bits(env)
        if lm == 0:
            env = cm.no_step(env)[0]
            continue
        wm = CM.wins_trial(env, lm)
        env = cm.env_step(env, int(rng.choice([a for a in range(CM.A) if ((wm if wm else lm) >> a) & 1])))[0]


# ---- the fixture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_fixture_holds_the_kinds_of_root_the_tests_need(rule_set):
    envs, tags = CM.load_roots(rule_set)
    assert 20 <= len(envs) <= 28
    assert wanted_tags(rule_set) <= {t for ts in tags for t in ts}
    assert ("softlock" in wanted_tags(rule_set)) == CM.RULE_SETS[rule_set]["enable_dice_rethrow"]
    assert ("partner" in wanted_tags(rule_set)) == (rule_set == "selfplay_4p_teams")
    for env, ts in zip(envs, tags):
        assert 1 <= env.die <= 6
        assert sorted(ts) == sorted(tags_of(env))
        lm = CM.legal_bits(env)
        assert ("done" in ts) == bool(env.done)
        assert ("stuck" in ts) == (not env.done and lm == 0)
        assert ("wins" in ts) == (not env.done and CM.wins_trial(env, lm) != 0)


def test_rule_sets_are_the_ones_named():
    assert CM.RULE_SETS["selfplay_4p_teams"] == dict(num_players=4, **cm.SELFPLAY_RULES)
    assert CM.RULE_SETS["default_2p"] == dict(num_players=2, **cm.DEFAULT_RULES)
    r = CM.RULE_SETS["rethrow_six_2p"]
    assert r["enable_dice_rethrow"] and not r["enable_start_on_1"] and r["num_players"] == 2
    assert {k: v for k, v in r.items() if k not in ("enable_dice_rethrow", "enable_start_on_1", "num_players")} == \
        {k: v for k, v in cm.DEFAULT_RULES.items() if k not in ("enable_dice_rethrow", "enable_start_on_1")}


# ---- wins: the kernel's formulation against the trial steps --------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_fast_wins_equal_trial_steps_on_every_state_of_random_games(rule_set):
    states = with_win = finished = 0
    for seed in range(4):
        for env in random_game_states(rule_set, 1000 + seed):
            lm = CM.legal_bits(env)
            trial = CM.wins_trial(env, lm)
            assert CM.wins_fast(env, lm) == trial, (rule_set, seed, env.pins.tolist(), env.die)
            states += 1
            with_win += trial != 0 and not env.done
            finished += env.done
    assert finished == 4 and with_win >= 4 and states > 400, (states, with_win, finished)


# ---- the decision -> chance edge: discount and chance priors -------------------------------------------------------
def test_discount_is_plus_one_on_a_bonus_turn_and_minus_one_otherwise():
    """2 players, bonus turn on 6: a legal 6 that does not end the game keeps the mover, discount +1 (hand-checked:
    env_step leaves current_player alone when move == 6); every other legal pin hands the turn over, -1."""
    for rule_set in ("default_2p", "rethrow_six_2p"):
        seen = {1.0: 0, -1.0: 0}
        for env in CM.load_roots(rule_set)[0]:
            lm = 0 if env.done else CM.legal_bits(env)
            for a in range(CM.A):
                if not (lm >> a) & 1:
                    continue
                nxt, reward, disc = CM.decision_step(env, a, False)
                if nxt.done:
                    assert disc == 0.0 and reward == 1
                    continue
                assert reward == 0
                assert disc == (1.0 if env.die == 6 else -1.0)
                assert (nxt.current_player == env.current_player) == (env.die == 6)
                seen[disc] += 1
        assert seen[1.0] >= 2 and seen[-1.0] > 10, (rule_set, seen)
        for env in _tagged(rule_set, "bonus"):
            assert env.die == 6
            assert any(CM.decision_step(env, a, False)[2] == 1.0 for a in range(CM.A) if (CM.legal_bits(env) >> a) & 1)


def test_discount_follows_the_team_not_the_seat():
    """4 players in teams, side(p) = p % 2: a finished player moving its partner's pins is followed by an opponent
    (-1) unless the die is 6 (+1: the same seat again); the next seat is always the other side."""
    partner = _tagged("selfplay_4p_teams", "partner")
    assert partner
    for env in CM.load_roots("selfplay_4p_teams")[0]:
        lm = 0 if env.done else CM.legal_bits(env)
        for a in range(CM.A):
            if (lm >> a) & 1:
                nxt, _, disc = CM.decision_step(env, a, False)
                if not nxt.done:
                    assert disc == (1.0 if nxt.current_player % 2 == env.current_player % 2 else -1.0)
                    assert disc == (1.0 if env.die == 6 else -1.0)
    for env in partner:
        assert cm._sub_player(env) == (env.current_player + 2) % 4
    # a pass (no_step) goes to the next seat: the other side, -1; of a finished game 0
    stuck = _tagged("selfplay_4p_teams", "stuck")[0]
    assert CM.decision_step(stuck, 0, True)[1:] == (0, -1.0)
    done = _tagged("selfplay_4p_teams", "done")[0]
    assert CM.decision_step(done, 0, True)[1:] == (0, 0.0)


def test_chance_priors_of_soft_locked_afterstates_are_the_environments_tables():
    tables = {"selfplay_4p_teams": np.array([76, 16, 16, 16, 16, 76], np.float64) / 216,
              "rethrow_six_2p": np.array([25, 25, 25, 25, 25, 91], np.float64) / 216}
    for rule_set, tab in tables.items():
        hits = 0
        for env in _tagged(rule_set, "softlock"):
            lm = CM.legal_bits(env)
            for a in range(CM.A):
                if (lm >> a) & 1:
                    after = CM.decision_step(env, a, False)[0]
                    p = CM.chance_priors(after)
                    assert p.dtype == np.float32
                    if cm.is_soft_locked(after):
                        hits += 1
                        assert p.tobytes() == tab.astype(np.float32).tobytes()        # bit for bit
                    else:
                        assert p.tobytes() == np.full(6, 1 / 6, np.float32).tobytes()
        assert hits
    for env in CM.load_roots("default_2p")[0]:                                      # no rethrow: always uniform
        assert CM.chance_priors(env).tobytes() == np.full(6, 1 / 6, np.float32).tobytes()


def test_decision_priors_mask_illegal_pins():
    assert CM.decision_prior(0b1011, 0b0010).tolist() == [0.0, 1.0, 0.0, 0.0]       # the winning pin takes it all
    assert CM.decision_prior(0b1010, 0).tolist() == [0.0, 0.5, 0.0, 0.5]
    assert CM.decision_prior(1, 0).tolist() == [1.0, 0.0, 0.0, 0.0]                 # a passing node
    assert CM.root_prior(0b0110, 0, ZERO, 0.0).tolist() == [0.0, 0.5, 0.5, 0.0]


# ---- the rollout ---------------------------------------------------------------------------------------------------
def test_rollout_is_deterministic_in_its_keys_and_has_its_own_stream():
    from tests import _env_mcts as EM
    env = CM.load_roots("default_2p")[0][-1]
    assert not env.done
    base = CM.rollout(env, 0, 11, 3, 5, 2, 60, True)
    assert base == CM.rollout(env, 0, 11, 3, 5, 2, 60, True)
    assert base[1] <= 60 and base[0] in (-1.0, 0.0, 1.0)
    assert CM.rollout(env, 0, 11, 3, 5, 2, 0, True) == (0.0, 0)
    keys = [(11, 3, 5, 2), (12, 3, 5, 2), (11, 4, 5, 2), (11, 3, 6, 2), (11, 3, 5, 3)]
    draws = [[CM.rollout_uniform(*k, i) for i in range(8)] for k in keys]
    assert all(0.0 <= u < 1.0 for d in draws for u in d)
    assert len({tuple(d) for d in draws}) == len(keys)
    assert CM.ROLLOUT_STREAM != EM.ROLLOUT_STREAM
    assert draws[0] != [EM.rollout_uniform(*keys[0], i) for i in range(8)]


def test_rollout_keeps_the_die_of_a_decision_node_on_its_first_turn():
    """A root with a winning pin: keeping the die the mover wins at once (+1, one turn), from either side's view the
    sign follows the side; with trial-step wins it is the same rollout."""
    env = _tagged("default_2p", "wins")[0]
    mover = env.current_player
    assert CM.rollout(env, mover, 1, 0, 0, 0, 300, True) == (1.0, 1)
    assert CM.rollout(env, 1 - mover, 1, 0, 0, 0, 300, True) == (-1.0, 1)
    for rule_set in RULE_SETS:
        e = _tagged(rule_set, "bonus")[0]
        assert CM.rollout(e, 0, 5, 1, 2, 3, 200, False) == CM.rollout(e, 0, 5, 1, 2, 3, 200, False,
                                                                      wins_fn=CM.wins_trial)


# ---- the restated search at rollout_steps = 0 ----------------------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_restated_tree_invariants(rule_set):
    envs, tags = CM.load_roots(rule_set)
    S, D = 40, 20
    searched = chance_nodes = passing_nodes = 0
    for b, (env, ts) in enumerate(zip(envs, tags)):
        r = CM.search_one(env, S, D, 0.0, 0, 9, 1, b, ZERO, ZERO)
        if "done" in ts or "stuck" in ts:
            assert r["action"] == -1 and r["tree"] is None and not r["weights"].any() and r["value"] == 0
            continue
        searched += 1
        t = r["tree"]
        assert r["visits"].sum() == S and r["turns"] == 0                      # root visits sum to S
        assert not t.c_visits[0, CM.A:].any()
        assert np.array_equal(r["weights"], (r["visits"] / np.float32(S)).astype(np.float32))
        lm = CM.legal_bits(env)
        assert all((lm >> a) & 1 for a in range(CM.A) if r["visits"][a])       # only legal pins are visited
        for n in range(S + 1):
            if t.visits[n] == 0:
                continue
            kids = t.c_visits[n]
            if not t.is_dec[n]:
                # a chance node's child visits follow argmax p / (n + 1): replay them
                chance_nodes += 1
                assert not kids[:CM.A].any()
                p = t.c_prior[n, CM.A:]
                cnt = np.zeros(CM.C, np.int32)
                for _ in range(int(kids[CM.A:].sum())):
                    cnt[int(np.argmax(p / (cnt + 1).astype(np.float32)))] += 1
                assert np.array_equal(cnt, kids[CM.A:])
            else:
                assert not kids[CM.A:].any()
                if n and r["passing"][n]:
                    passing_nodes += 1
                    assert (t.c_index[n, 1:] == -1).all() and not kids[1:].any()   # a passing node has one child
                    assert t.c_prior[n, :CM.A].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert searched >= 18 and chance_nodes > 50 and passing_nodes > 5


def test_restated_search_on_a_winning_root():
    env = _tagged("default_2p", "wins")[0]
    r = CM.search_one(env, 8, 4, 0.0, 20, 3, 0, 0, ZERO, ZERO)
    wm = CM.wins_trial(env)
    assert (wm >> r["action"]) & 1 and r["visits"].sum() == 8 and r["qvalues"][r["action"]] == 1.0


# ---- the C entry point's refusals (no launch) ----------------------------------------------------------------------
class _Call:
    """muz_classic_mcts with never-dereferenced dummy pointers: every case here must return before any launch."""

    def __init__(self):
        from exploring_muzero_on_dog_amd import classic as E
        from exploring_muzero_on_dog_amd import stochastic as ST
        self.L = _lib()
        self.so = self.L.load()
        self.ST, self.E = ST, E
        self.buf = (ctypes.c_char * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.rules = E.make_rules(num_players=2, **cm.DEFAULT_RULES)

    def soa(self, n=1, null=None):
        s = self.L.MuzClassicSoA()
        for name in ("board", "pins", "current_player", "reward", "done", "die"):
            setattr(s, name, None if name == null else self.p)
        s.stride = n
        return s

    def __call__(self, cfg, rollout_steps=300, n=1, ws_bytes=1 << 40, rules="classic", mcfg="cfg", null=None,
                 soa=None, ws=None):
        P = [self.p] * 9   # dirichlet, gumbel, game_id, workspace, action, weights, value, visits, qvalues
        if null is not None:
            P[null] = None
        if ws is not None:
            P[3] = ws
        m = self.L.MuzEnvMctsCfg(rollout_steps)
        return self.so.muz_classic_mcts(self.rules if rules == "classic" else rules,
                                        ctypes.byref(cfg) if cfg is not None else None,
                                        ctypes.byref(m) if mcfg == "cfg" else None, self.soa(n) if soa is None else soa,
                                        P[0], P[1], P[2], n, P[3], ws_bytes, P[4], P[5], P[6], P[7], P[8], None)


@pytest.fixture(scope="module")
def call():
    return _Call()


TREE_BYTES = {(1, 1): 1152, (1, 50): 23104, (17, 1): 15488, (17, 50): 388672}


def test_mcts_workspace_is_the_trees_own_carve(call):
    """Per game an int32 turn counter (the block rounded up to 256 bytes), per node six 16-wide children arrays and a
    64-byte state row; one byte less is MUZ_E_INVALID, n = 0 with nothing MUZ_OK."""
    L, ST = call.L, call.ST
    for (n, S), want in TREE_BYTES.items():
        assert want == (n * 4 + 255) // 256 * 256 + n * (S + 1) * (6 * 16 * 4 + 64)
        cfg = ST.make_cfg(S, min(S, 64))
        assert call.so.muz_classic_mcts_tree_bytes(n, ctypes.byref(cfg)) == want
        assert call(cfg, n=n, ws_bytes=want - 1) == L.MUZ_E_INVALID, (n, S)
        assert call(cfg, n=0, ws_bytes=0) == L.MUZ_OK
    assert call.so.muz_classic_mcts_tree_bytes(4, None) == -1
    assert call.so.muz_classic_mcts_tree_bytes(-1, ctypes.byref(ST.make_cfg(8, 8))) == -1
    assert call.so.muz_classic_mcts_tree_bytes(4, ctypes.byref(ST.make_cfg(101, 8))) == -1
    assert call.so.muz_classic_mcts_tree_bytes(4, ctypes.byref(ST.make_cfg(8, 65))) == -1


@pytest.mark.parametrize("change", [
    dict(num_simulations=0), dict(num_simulations=101), dict(max_depth=0), dict(max_depth=65),
    dict(dirichlet_fraction=1.01), dict(dirichlet_fraction=-0.1), dict(dirichlet_alpha=0.0), dict(pb_c_base=0.0),
    dict(pb_c_init=float("nan")), dict(temperature=-0.5), dict(temperature=float("nan")), dict(rollout_steps=-1),
    dict(rollout_steps=1001)])
def test_mcts_refuses_unsupported_configurations(call, change):
    cfg = call.ST.make_cfg(50, 25, 0.0)
    change = dict(change)
    steps = change.pop("rollout_steps", 300)
    for k, v in change.items():
        setattr(cfg, k, v)
    assert call(cfg, rollout_steps=steps) == call.L.MUZ_E_UNSUPPORTED
    assert call(cfg, rollout_steps=steps, null=4) == call.L.MUZ_E_UNSUPPORTED   # even with a null pointer beside it


def test_mcts_accepts_the_rollout_limits_and_refuses_rules(call):
    L, E = call.L, call.E
    cfg = call.ST.make_cfg(50, 25, 0.0)
    for steps in (0, 1000):                    # accepted: the next check (a short workspace) answers
        assert call(cfg, rollout_steps=steps, ws_bytes=0) == L.MUZ_E_INVALID
    assert call(cfg, rules=E.make_rules(num_players=2, starting_player=-1, **cm.DEFAULT_RULES)) == L.MUZ_E_UNSUPPORTED
    assert call(cfg, rules=E.make_rules(num_players=2, distance=12, **cm.DEFAULT_RULES)) == L.MUZ_E_UNSUPPORTED


def test_mcts_refuses_null_pointers_and_bad_workspaces(call):
    L = call.L
    cfg = call.ST.make_cfg(50, 25, 0.0)
    assert call(None) == L.MUZ_E_INVALID
    assert call(cfg, mcfg=None) == L.MUZ_E_INVALID
    assert call(cfg, rules=None) == L.MUZ_E_INVALID
    assert call(cfg, n=-1) == L.MUZ_E_INVALID
    assert call(cfg, n=2, soa=call.soa(1)) == L.MUZ_E_INVALID          # fewer games in the state than searched
    for i in (3, 4, 5, 6):        # dirichlet, gumbel, game_id (0-2) and visit_counts, qvalues (7, 8) may be null
        assert call(cfg, null=i) == L.MUZ_E_INVALID, i
    for name in ("board", "pins", "die", "current_player", "done", "reward"):
        assert call(cfg, soa=call.soa(1, null=name)) == L.MUZ_E_INVALID, name
    off = ctypes.c_void_p(ctypes.addressof(call.buf) + 4)              # not 16-byte aligned
    assert ctypes.addressof(call.buf) % 16 == 0
    assert call(cfg, ws=off) == L.MUZ_E_INVALID


# ---- the Python entry points ---------------------------------------------------------------------------------------
def test_python_entry_points_accept_the_seat_for_classic_only():
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import stochastic as ST
    assert EV.STOCHASTIC_MCTS_AGENT == "stochastic_mcts_agent"
    assert EV._seat(EV._Classic, "stochastic_mcts_agent", 0, 0, "cpu") == EV.STOCHASTIC_MCTS_AGENT
    assert EV._Classic.ENV_SEAT == EV.STOCHASTIC_MCTS_AGENT and EV._Det.ENV_SEAT == EV.MCTS_AGENT
    assert EV._Dog.ENV_SEAT is None
    for game in (EV._Det, EV._Dog):
        with pytest.raises(ValueError, match="chance nodes"):
            EV._seat(game, "stochastic_mcts_agent", 0, 0, "cpu")
    with pytest.raises(ValueError, match="no environment-model search kernel"):
        EV._seat(EV._Classic, "mcts_agent", 0, 0, "cpu")                  # the det seat stays refused for classic
    assert EV._mcts_workspace(EV._Classic, ["random_agent"] * 4, 4, 8, "cpu") is None
    assert EV._mcts_workspace(EV._Dog, ["random_agent"] * 4, 4, 8, "cpu") is None
    with pytest.raises(TypeError, match="classic-MADN"):
        ST.env_stochastic_muzero_policy(object(), 8, 4, seed=0, turn=0)
    with pytest.raises(TypeError):
        ST.env_stochastic_muzero_policy(None, 8, 4)      # seed and turn are required: the rollouts are keyed by them
