"""The DOG greedy agent restated in NumPy on oracle/dog.py (TEST INFRASTRUCTURE; not a test module).

This file is the DEFINITION of muz_dog_greedy_action (csrc/dog_greedy.hip, dog.greedy_policy, dog.afterstate_features,
the 'greedy_agent' seat): the reference has no DOG agent that runs, so parity with the reference is UNPINNED and the
kernel must equal this restatement -- bit for bit in the features, the scores and the temperature-0 action; the
sampled action also goes through the device's logf (``near_tie``).

For one root game with ``game_id``, ``turn`` and ``seed``:

  m = the current player; the SIDE of seat p is p & 1 with enable_teams, else p (_dog_rollout.side_of); ME = the seats
  on m's side, OP = the other seats below num_players; C = the legal actions (valid_actions), ascending, empty for a
  finished game.

  For a in C: after = env_step(root, a) WITHOUT the deal the step may ask for.  Only the board and the pins of
  ``after`` are used, and a deal changes neither.  Swap-phase actions (792..805: the card to hand over) leave the
  board alone, so their features are all 0.

  prog(s, p) = int(oracle.evaluate.calculate_progress(s, p)): the measure the DOG result tables print (sorted rotated
  pins matched greedily to the four goal cells); an exact integer.

  Six int32 features per action, b = root, a = after; 0 for an action outside C:
    0 advance  sum over ME of prog(b, p) - prog(a, p)
    1 setback  sum over OP of prog(a, p) - prog(b, p)
    2 goal     sum over ME of (pins >= board_size after - before)
    3 out      sum over ME of (pins < 0 before - after)      (negative when a 7 sends an own pin home)
    4 hit      sum over OP of (pins < 0 after - before)
    5 win      +1 if get_winner(after) is non-empty and holds a seat of ME, -1 if non-empty and not, else 0

  score[a] = sum_i w[i] F[a][i] as int32 for a in C, INT32_MIN elsewhere; every weight an int32 in [-32768, 32767]
  (the features are bounded by a few hundred, so the sum cannot overflow).

  Choice: C empty -> -1.  temperature == 0 -> the smallest a with the greatest score.  Otherwise
  v(a) = float32(score[a]) / float32(temperature) + policy_gumbel(key, a) (one IEEE division, one IEEE add), key =
  game_key(seed ^ POLICY_STREAM, game_id, turn): the det and classic scripted agents' stream and draw
  (oracle/evaluate.py policy_gumbel), extended to a < 806; the action is the first a of C whose v is strictly
  greatest.  Nothing is keyed by the game's position in a batch.
"""
import functools
import json
import math
import os

import numpy as np

from oracle import dog as dg
from oracle import evaluate as oe
from oracle.dog import M64, _game_key, _mix64, _u24
from tests import _dog_rollout as DR

A = 806
NF = 6
F32 = np.float32
INT32_MIN = int(np.iinfo(np.int32).min)
FEATURES = ("advance", "setback", "goal", "out", "hit", "win")
GREEDY_DEFAULTS = dict(advance=1, setback=1, goal=20, out=15, hit=10, win=1000, temperature=0.25)
RULE_SETS = DR.RULE_SETS
ROOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dog_greedy_roots.json")


def weights_of(cfg=None):
    """-> (int weights [6], float32 temperature) of a dict over GREEDY_DEFAULTS' keys (missing keys: the defaults)."""
    v = dict(GREEDY_DEFAULTS)
    v.update(cfg or {})
    w = [int(v[k]) for k in FEATURES]
    assert all(-32768 <= x <= 32767 for x in w)
    return w, F32(v["temperature"])


# ---- the pieces -----------------------------------------------------------------------------------------------------
def sides(env):
    """-> (ME, OP): the seats on the current player's side, the other seats."""
    teams = env.rules["enable_teams"]
    m = int(env.current_player)
    side = (lambda p: p & 1) if teams else (lambda p: p)
    me = [p for p in range(env.num_players) if side(p) == side(m)]
    return me, [p for p in range(env.num_players) if p not in me]


def prog(env, p):
    return int(oe.calculate_progress(env, p))


def afterstate(env, a):
    """env_step without the deal it may ask for: the board and pins after the action (a deal changes neither)."""
    keys = dg.engine_shuffle_keys(0, 0)       # the keys of a deal that is never looked at
    return dg.env_step(env, int(a), shuffle_keys=keys)[0]


def features_of(env, a):
    """The six features of the legal action ``a`` -> int list [6]."""
    after = afterstate(env, a)
    me, op = sides(env)
    bs = env.board_size
    b, x = env.pins.astype(np.int64), after.pins.astype(np.int64)
    w = np.asarray(dg.get_winner(after, after.board), bool)
    return [sum(prog(env, p) - prog(after, p) for p in me),
            sum(prog(after, p) - prog(env, p) for p in op),
            sum(int((x[p] >= bs).sum()) - int((b[p] >= bs).sum()) for p in me),
            sum(int((b[p] < 0).sum()) - int((x[p] < 0).sum()) for p in me),
            sum(int((x[p] < 0).sum()) - int((b[p] < 0).sum()) for p in op),
            0 if not w.any() else (1 if any(w[p] for p in me) else -1)]


def policy_gumbel(key, a):
    u = max(F32(_u24(_mix64(key ^ (((a + 1) * 0xD6E8FEB86659FD93) & M64)))), F32(oe.TINY))
    return F32(-np.log(-np.log(F32(u))))


def policy_key(seed, game_id, turn):
    return _game_key((seed & M64) ^ oe.POLICY_STREAM, game_id, turn)


def evaluate_root(env):
    """-> (C, features int32 [806, 6]) of one root; independent of weights, temperature and keys."""
    C = DR.candidates(env)
    F = np.zeros((A, NF), np.int32)
    for a in C:
        F[a] = features_of(env, a)
    return C, F


def scores_of(C, F, w):
    sc = np.full(A, INT32_MIN, np.int64)
    for a in C:
        sc[a] = sum(int(w[i]) * int(F[a, i]) for i in range(NF))
    assert all(abs(int(sc[a])) < 2 ** 31 - 1 for a in C)
    return sc.astype(np.int32)


def values_of(C, sc, temperature, seed, turn, game_id):
    """v(a) float32 for a in C (in C's order)."""
    key = policy_key(seed, game_id, turn)
    return [F32(F32(F32(sc[a]) / F32(temperature)) + policy_gumbel(key, a)) for a in C]


def choose(C, sc, temperature, seed, turn, game_id):
    if not C:
        return -1
    if F32(temperature) == 0:
        best = max(int(sc[a]) for a in C)
        return next(a for a in C if int(sc[a]) == best)
    v = values_of(C, sc, temperature, seed, turn, game_id)
    return C[int(np.argmax(np.array(v, F32)))]          # argmax: the first of the greatest


def near_tie(C, sc, temperature, seed, turn, game_id, ulps=4):
    """True when the two largest v of a sampled choice differ by at most ``ulps`` ulp of the larger magnitude: the
    margin within which the device's logf may order them differently from NumPy's."""
    if len(C) < 2 or F32(temperature) == 0:
        return False
    v = np.sort(np.array(values_of(C, sc, temperature, seed, turn, game_id), F32))
    hi, lo = v[-1], v[-2]
    if not (np.isfinite(hi) and np.isfinite(lo)):
        return bool(hi == lo)
    mag = max(abs(hi), abs(lo))
    return bool(F32(hi - lo) <= F32(ulps) * np.spacing(F32(mag)))


def greedy_one(env, cfg, seed, turn, game_id, root=None):
    """-> dict(action, scores int32 [806], features int32 [806, 6], C); ``root``: evaluate_root(env), if at hand."""
    w, temperature = weights_of(cfg)
    C, F = evaluate_root(env) if root is None else root
    sc = scores_of(C, F, w)
    return dict(action=choose(C, sc, temperature, seed, turn, game_id), scores=sc, features=F, C=C)


# ---- the fixture ----------------------------------------------------------------------------------------------------
def load_roots(rule_set, path=ROOTS):
    """-> (oracle states, their tag lists) of one rule set of tests/golden/dog_greedy_roots.json."""
    with open(path) as fh:
        recs = json.load(fh)[rule_set]
    return [DR.state_from_record(rule_set, r) for r in recs], [r["tags"] for r in recs]


@functools.lru_cache(maxsize=None)
def batch_roots(rule_set):
    """The batch the host census and the GPU tests share: the rule set's roots of dog_greedy_roots.json, then its roots
    of dog_rollout_roots.json; a root's game id is its position.  -> (states, tag lists, evaluate_root of each)."""
    envs, tags = load_roots(rule_set)
    more, mtags = DR.load_roots(rule_set)
    envs, tags = envs + more, tags + mtags
    roots = [evaluate_root(e) for e in envs]
    for _, F in roots:
        F.setflags(write=False)
    return envs, tags, roots


# the (seed, turn) pairs of the sampled-action checks (host census and GPU comparison)
SAMPLE_KEYS = ((11, 3), (12, 0), (2025, 77), (0xDEADBEEF, 500))
NEAR_TIE_CAP = 0.01      # at most this share of the compared cases may be excused as near ties


def sampled_cases(rule_set, cfg=None):
    """Every (root b, seed, turn) of the shared batch with its restated action and whether it is a near tie."""
    w, temperature = weights_of(cfg)
    envs, _, roots = batch_roots(rule_set)
    out = []
    for b, (C, F) in enumerate(roots):
        sc = scores_of(C, F, w)
        for seed, turn in SAMPLE_KEYS:
            out.append((b, seed, turn, choose(C, sc, temperature, seed, turn, b),
                        near_tie(C, sc, temperature, seed, turn, b)))
    return out


def binomial_bar(n, p=1e-3):
    """The smallest k with P(Bin(n, 1/2) >= k) < p (the bar of tests/test_gpu_dog_rollout_seat.py)."""
    tail, total = 0, 2 ** n
    for k in range(n, -1, -1):
        tail += math.comb(n, k)
        if tail >= p * total:
            return k + 1
    return 0
