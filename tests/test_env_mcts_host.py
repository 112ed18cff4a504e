"""The network-free MCTS agent for det-MADN (csrc/env_mcts.hip, mcts.env_muzero_policy, the 'mcts_agent' seat),
everything that needs no GPU: the restatement's pieces (tests/_env_mcts.py) on oracle/detmadn.py states, the fixture
of root states, muz_detmadn_mcts's refusals (argument checks come before any launch, so they run on a host without a
GPU) and the refusals of the Python entry points."""
import ctypes

import numpy as np
import pytest

from oracle import detmadn as dm
from tests import _env_mcts as EM

RULE_SETS = list(EM.RULE_SETS)


def _lib():
    from exploring_muzero_on_dog_amd import lib as L
    return L


def random_game_states(rule_set, seed, max_plies=3000):
    """Every state of one seeded game under the rollout policy (it ends games: a winning action when there is one)."""
    rng = np.random.default_rng(seed)
    env = dm.env_reset(**EM.RULE_SETS[rule_set])
    for _ in range(max_plies):
        yield env
        if env.done:
            return
        lm = EM.legal_bits(env)
        if lm == 0:
            env = dm.no_step(env)[0]
            continue
        wm = EM.wins_trial(env, lm) if (env.pins >= env.board_size).sum(1).max() >= 3 else 0
        env = dm.env_step(env, dm.map_action(int(rng.choice(np.flatnonzero(EM.bits_to_bool(wm if wm else lm))))))[0]


# ---- wins: the kernel's formulation against the trial steps --------------------------------------------------------
@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_fast_wins_equal_trial_steps_on_every_state_of_random_games(rule_set):
    states = with_win = finished = 0
    for seed in range(4):
        for env in random_game_states(rule_set, 1000 + seed):
            lm = EM.legal_bits(env)
            trial = EM.wins_trial(env, lm)
            assert EM.wins_fast(env, lm) == trial, (rule_set, seed, env.pins.tolist())
            states += 1
            with_win += trial != 0 and not env.done
            finished += env.done
    assert finished == 4 and with_win >= 4 and states > 400, (states, with_win, finished)


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_fixture_holds_the_kinds_of_root_the_tests_need(rule_set):
    envs, tags = EM.load_roots(rule_set)
    assert 20 <= len(envs) <= 28
    kinds = {t for ts in tags for t in ts}
    assert {"wins", "done", "stuck", "pass", "bonus"} <= kinds
    for env, ts in zip(envs, tags):
        lm = EM.legal_bits(env)
        assert ("done" in ts) == bool(env.done)
        assert ("stuck" in ts) == (not env.done and lm == 0)
        assert ("wins" in ts) == (not env.done and EM.wins_trial(env, lm) != 0)
        assert EM.wins_fast(env, lm) == EM.wins_trial(env, lm)
        if "pass" in ts:
            assert any((lm >> a) & 1 and EM.transition(env, a)[3] > 0 for a in range(EM.A))


# ---- transition: the discount and pass rules on hand-checked fixture states ----------------------------------------
def _tagged(rule_set, tag):
    envs, tags = EM.load_roots(rule_set)
    return [e for e, ts in zip(envs, tags) if tag in ts]


def test_discount_is_plus_one_when_the_same_side_moves_again():
    """2 players, bonus turn on 6: a legal move of 6 that does not end the game keeps the mover, discount +1; any other
    legal move that leaves the opponent a legal action hands the turn over, discount -1."""
    seen = {1.0: 0, -1.0: 0}
    for env in EM.load_roots("default_2p")[0]:
        lm = EM.node_mask(env)
        for a in range(EM.A):
            if not (lm >> a) & 1:
                continue
            nxt, reward, disc, passes = EM.transition(env, a)
            if nxt.done:
                assert disc == 0.0 and reward == 1
                continue
            assert reward == 0
            same = nxt.current_player == env.current_player
            assert disc == (1.0 if same else -1.0)
            if passes == 0:
                assert same == (a % 6 == 5)
            seen[disc] += 1
    assert seen[1.0] > 5 and seen[-1.0] > 20


def test_discount_follows_the_team_not_the_seat():
    """4 players in teams: side(p) = p % 2, so a turn that passes over an opponent without a legal action to the
    partner keeps the side (+1), and one that goes to the next seat changes it (-1)."""
    for env in EM.load_roots("selfplay_4p_teams")[0]:
        lm = EM.node_mask(env)
        for a in range(EM.A):
            if (lm >> a) & 1:
                nxt, _, disc, _ = EM.transition(env, a)
                if not nxt.done:
                    assert disc == (1.0 if nxt.current_player % 2 == env.current_player % 2 else -1.0)


@pytest.mark.parametrize("rule_set", RULE_SETS)
def test_transition_passes_over_no_move_turns(rule_set):
    for env in _tagged(rule_set, "pass"):
        lm = EM.legal_bits(env)
        hits = 0
        for a in range(EM.A):
            if not (lm >> a) & 1:
                continue
            stepped = dm.env_step(env, dm.map_action(a))[0]
            nxt, _, _, passes = EM.transition(env, a)
            assert 0 <= passes <= EM.MAX_PASSES
            if passes:
                hits += 1
                assert not stepped.done and EM.legal_bits(stepped) == 0
                skipped = stepped
                for _ in range(passes):
                    skipped = dm.no_step(skipped)[0]
                assert np.array_equal(skipped.action_set, nxt.action_set)
                assert skipped.current_player == nxt.current_player and np.array_equal(stepped.pins, nxt.pins)
                assert EM.legal_bits(nxt) != 0 or passes == EM.MAX_PASSES
            else:
                assert stepped.done or EM.legal_bits(stepped) != 0
        assert hits


def test_a_finished_game_stays_as_it_is():
    for rule_set in RULE_SETS:
        for env in _tagged(rule_set, "done"):
            assert EM.node_mask(env) == 0
            nxt, reward, disc, passes = EM.transition(env, 7)
            assert nxt is env and (reward, disc, passes) == (0, 0.0, 0)
            assert (EM.prior_logits(0, 0) == 0).all()


def test_prior_logits_mask_illegal_actions():
    lg = EM.prior_logits(0b1011, 0b0010)
    assert lg[:4].tolist() == [100.0, 300.0, EM.PZ.FMIN, 100.0] and (lg[4:] == EM.PZ.FMIN).all()


# ---- the rollout ---------------------------------------------------------------------------------------------------
def test_rollout_is_deterministic_in_its_keys():
    env = EM.load_roots("default_2p")[0][-1]
    assert not env.done
    base = EM.rollout(env, 11, 3, 5, 2, 60)
    assert base == EM.rollout(env, 11, 3, 5, 2, 60)
    assert base[1] <= 60 and base[0] in (-1.0, 0.0, 1.0)
    assert EM.rollout(env, 11, 3, 5, 2, 0) == (0.0, 0)
    keys = [(11, 3, 5, 2), (12, 3, 5, 2), (11, 4, 5, 2), (11, 3, 6, 2), (11, 3, 5, 3)]
    draws = [[EM.rollout_uniform(*k, i) for i in range(8)] for k in keys]
    assert all(0.0 <= u < 1.0 for d in draws for u in d)
    assert len({tuple(d) for d in draws}) == len(keys)            # every key component selects another stream
    assert draws[0] == [EM.rollout_uniform(*keys[0], i) for i in range(8)]
    # the pick: the k-th set bit, k = min(floor(u count), count - 1)
    assert [EM.kth_set_bit(0b101100, u) for u in (0.0, 0.33, 0.34, 0.67, 0.999)] == [2, 2, 3, 5, 5]


def test_rollout_with_trial_wins_is_the_same_rollout():
    for rule_set in RULE_SETS:
        env = _tagged(rule_set, "bonus")[0]
        assert EM.rollout(env, 5, 1, 2, 3, 200) == EM.rollout(env, 5, 1, 2, 3, 200, wins_fn=EM.wins_trial)


def test_rollout_value_is_seen_from_the_side_to_move():
    """To the end from a state with a winning action: the mover wins at once, +1; the same final position seen from
    the other side's rollout is -1."""
    env = _tagged("default_2p", "wins")[0]
    assert EM.rollout(env, 1, 0, 0, 0, 300) == (1.0, 1)
    other = env.replace(current_player=1 - env.current_player)
    v, turns = EM.rollout(other, 1, 0, 0, 0, 2000)
    assert v in (-1.0, 1.0) and turns >= 1


def test_restated_search_on_a_winning_root():
    env = _tagged("default_2p", "wins")[0]
    r = EM.search_one(env, 8, 4, 0.0, 20, 3, 0, 0, np.zeros(EM.A, np.float32), np.zeros(EM.A, np.float32))
    wm = EM.wins_trial(env)
    assert (wm >> r["action"]) & 1 and r["visits"].sum() == 8 and r["qvalues"][r["action"]] == 1.0
    done = _tagged("default_2p", "done")[0]
    r = EM.search_one(done, 8, 4, 0.0, 20, 3, 0, 0, np.zeros(EM.A, np.float32), np.zeros(EM.A, np.float32))
    assert r["action"] == -1 and r["tree"] is None and not r["weights"].any() and r["value"] == 0


# ---- the C entry point's refusals (no launch) ----------------------------------------------------------------------
class _Call:
    """muz_detmadn_mcts with never-dereferenced dummy pointers: every case here must return before any launch."""

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

    def __call__(self, cfg, rollout_steps=300, n=1, ws_bytes=1 << 40, rules="det", mcfg="cfg", null=None, soa=None,
                 ws=None):
        P = [self.p] * 9   # dirichlet, gumbel, game_id, workspace, action, weights, value, visits, qvalues
        if null is not None:
            P[null] = None
        if ws is not None:
            P[3] = ws
        m = self.L.MuzEnvMctsCfg(rollout_steps)
        return self.so.muz_detmadn_mcts(self.rules if rules == "det" else rules,
                                        ctypes.byref(cfg) if cfg is not None else None,
                                        ctypes.byref(m) if mcfg == "cfg" else None, self.soa(n) if soa is None else soa,
                                        P[0], P[1], P[2], n, P[3], ws_bytes, P[4], P[5], P[6], P[7], P[8], None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_env_mcts_cfg_layout():
    L = _lib()
    assert ctypes.sizeof(L.MuzEnvMctsCfg) == 4 and L.MuzEnvMctsCfg.rollout_steps.offset == 0


def test_mcts_workspace_is_the_trees_own_carve(call):
    """Per game an int32 turn counter (the block rounded up to 256 bytes), per node six 32-wide children arrays and a
    64-byte state row -- no 1 KB latent slot; one byte less is MUZ_E_INVALID, n = 0 with nothing MUZ_OK."""
    L, M = call.L, call.M
    for n in (1, 17, 4096):
        for S in (1, 50, 100):
            cfg = M.make_puct_cfg(S, min(S, 64))
            need = call.so.muz_detmadn_mcts_tree_bytes(n, ctypes.byref(cfg))
            assert need == (n * 4 + 255) // 256 * 256 + n * (S + 1) * (6 * 32 * 4 + 64)
            assert call(cfg, n=n, ws_bytes=need - 1) == L.MUZ_E_INVALID, (n, S)
            assert call(cfg, n=0, ws_bytes=0) == L.MUZ_OK
    assert call.so.muz_detmadn_mcts_tree_bytes(4, None) == -1
    assert call.so.muz_detmadn_mcts_tree_bytes(-1, ctypes.byref(M.make_puct_cfg(8, 8))) == -1
    assert call.so.muz_detmadn_mcts_tree_bytes(4, ctypes.byref(M.make_puct_cfg(101, 8))) == -1


@pytest.mark.parametrize("change", [
    dict(num_simulations=0), dict(num_simulations=101), dict(max_depth=0), dict(max_depth=65), dict(qtransform=2),
    dict(max_value=-1.0), dict(dirichlet_fraction=1.01), dict(dirichlet_alpha=0.0), dict(pb_c_base=0.0),
    dict(temperature=-0.5), dict(temperature=float("nan")), dict(rollout_steps=-1), dict(rollout_steps=1001)])
def test_mcts_refuses_unsupported_configurations(call, change):
    cfg = call.M.make_puct_cfg(50, 25)
    change = dict(change)
    steps = change.pop("rollout_steps", 300)
    for k, v in change.items():
        setattr(cfg, k, v)
    assert call(cfg, rollout_steps=steps) == call.L.MUZ_E_UNSUPPORTED
    assert call(cfg, rollout_steps=steps, null=4) == call.L.MUZ_E_UNSUPPORTED   # even with a null pointer beside it


def test_mcts_accepts_the_rollout_limits_and_refuses_rules(call):
    L, E = call.L, call.E
    cfg = call.M.make_puct_cfg(50, 25)
    for steps in (0, 1000):                    # accepted: the next check (a short workspace) answers
        assert call(cfg, rollout_steps=steps, ws_bytes=0) == L.MUZ_E_INVALID
    assert call(cfg, rules=E.make_rules(num_players=2, starting_player=-1, **dm.DEFAULT_RULES)) == L.MUZ_E_UNSUPPORTED
    assert call(cfg, rules=E.make_rules(num_players=2, distance=12, **dm.DEFAULT_RULES)) == L.MUZ_E_UNSUPPORTED


def test_mcts_refuses_null_pointers_and_bad_workspaces(call):
    L = call.L
    cfg = call.M.make_puct_cfg(50, 25)
    assert call(None) == L.MUZ_E_INVALID
    assert call(cfg, mcfg=None) == L.MUZ_E_INVALID
    assert call(cfg, rules=None) == L.MUZ_E_INVALID
    assert call(cfg, n=-1) == L.MUZ_E_INVALID
    assert call(cfg, n=2, soa=call.soa(1)) == L.MUZ_E_INVALID          # fewer games in the state than searched
    for i in (3, 4, 5, 6):        # dirichlet, gumbel, game_id (0-2) and visit_counts, qvalues (7, 8) may be null
        assert call(cfg, null=i) == L.MUZ_E_INVALID, i
    for name in ("board", "pins", "action_set", "current_player", "done", "reward"):
        assert call(cfg, soa=call.soa(1, null=name)) == L.MUZ_E_INVALID, name
    off = ctypes.c_void_p(ctypes.addressof(call.buf) + 4)              # not 16-byte aligned
    assert ctypes.addressof(call.buf) % 16 == 0
    assert call(cfg, ws=off) == L.MUZ_E_INVALID


# ---- the Python entry points ---------------------------------------------------------------------------------------
def test_python_entry_points_refuse_where_no_environment_model_exists():
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    assert EV._seat(EV._Det, "mcts_agent", 0, 0, "cpu") == "mcts_agent" == EV.MCTS_AGENT
    for game in (EV._Classic, EV._Dog):
        with pytest.raises(ValueError, match="no environment-model search kernel"):
            EV._seat(game, "mcts_agent", 0, 0, "cpu")
    assert "rule_based_agent" in EV._Dog.REFUSED and "rule_based_agent" not in EV._Classic.REFUSED
    with pytest.raises(ValueError, match="unknown agent"):
        EV._seat(EV._Det, "mcts", 0, 0, "cpu")
    with pytest.raises(ValueError):
        EV.play_vs_random("random_agent", 4, device="cpu")
    with pytest.raises(ValueError):
        EV._search_kwargs("mcts_agent")          # a seat, not a search of a network
    with pytest.raises(TypeError, match="det-MADN"):
        M.env_muzero_policy(object(), 8, 4, seed=0, turn=0)
    with pytest.raises(TypeError):
        M.env_muzero_policy(None, 8, 4)          # seed and turn are required: the rollouts are keyed by them
