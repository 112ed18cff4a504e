"""The DOG rollout agent with greedy-guided playouts restated in NumPy on oracle/dog.py (TEST INFRASTRUCTURE; not a
test module).

This file is the DEFINITION of muz_dog_guided_rollout_search (csrc/dog_guided.hip, dog.guided_rollout_policy, the
'guided_rollout_agent' seat): the reference has no DOG agent that runs, so parity with the reference is UNPINNED and the
kernel must equal this restatement bit for bit (every result is an integer sum; the value is one float32 division).

The guided search is tests/_dog_rollout.py's search with ONE change, the policy of the playout turns t >= 0.  The
candidates, the phases and the halving schedule, the ranking and the value, the determinization and the deals, the root
action as turn -1, the outcome, ``turns`` and the rollout seed ``rseed`` are that file's.  The new inputs are the six
weights ``w`` (the greedy agent's: tests/_dog_greedy.py, each in [-32768, 32767]) and ``epsilon``, a float32 in [0, 1].

Playout turn t on the playout's current state e with mover m:

  C = the legal actions of e, ascending.  C empty: no_step, as in the random playout.
  scores[a], a in C = the greedy agent's score of e (``_dog_greedy.features_of`` and ``scores_of`` on e): the features
  of the afterstate without the deal, ME and OP taken from m's side, a finished team player moving its partner's pins;
  swap-phase actions (792..805) have features 0, so every score of a swap-phase turn is 0.
  The turn EXPLORES iff u_e < epsilon (one float32 compare), u_e = U24(mix64(game_key(rseed ^ EXPLORE_STREAM, game_id,
  t))): epsilon 1 always explores, epsilon 0 never does.
  M = C when the turn explores, else the actions of C whose score is the greatest (in the swap phase: all of C).
  The action is the k-th member of M in ascending order, k = min(floor(u_t |M|), |M| - 1) in float32, u_t the uniform
  random turn t already draws: ``engine_random_action(mask of M, rseed, game_id, t)``.

Ties are broken uniformly, never by the smallest action (the greedy agent's first-argmax rule would always play the
joker copy of a move and hand over card 0).  With epsilon 1 the guided search is the rollout agent, output for output.
``decided`` counts the rollouts of a search whose outcome is not 0.
"""
import numpy as np

from oracle import dog as dg
from oracle.dog import M64, _game_key, _mix64, _u24
from tests import _dog_greedy as DGR
from tests import _dog_rollout as DR

A = 806
F32 = np.float32
EXPLORE_STREAM = 0xE9B10AE0D6
DEFAULT_EPSILON = 0.125                      # exact in float32
DEFAULT_WEIGHTS = tuple(DGR.GREEDY_DEFAULTS[k] for k in DGR.FEATURES)


def weights_of(weights=None):
    """-> the six int weights of a dict over _dog_greedy.FEATURES (missing keys: the greedy defaults)."""
    v = {k: DGR.GREEDY_DEFAULTS[k] for k in DGR.FEATURES}
    assert set(weights or {}) <= set(DGR.FEATURES)
    v.update(weights or {})
    w = [int(v[k]) for k in DGR.FEATURES]
    assert all(-32768 <= x <= 32767 for x in w)
    return w


def explore_uniform(rseed, game_id, t):
    return _u24(_mix64(_game_key((rseed & M64) ^ EXPLORE_STREAM, game_id, t)))


def explores(rseed, game_id, t, epsilon):
    return bool(F32(explore_uniform(rseed, game_id, t)) < F32(epsilon))


def turn_scores(e, C, w):
    """scores[a] for a in C (int32 [806], INT32_MIN elsewhere) of the playout state ``e``."""
    F = np.zeros((A, DGR.NF), np.int32)
    if e.phase == 0:
        for a in C:
            F[a] = DGR.features_of(e, a)
    return DGR.scores_of(C, F, w)


def choice_set(e, C, w, epsilon, rseed, game_id, t, census=None):
    """M of playout turn t: C when the turn explores, else the argmax set of the scores."""
    if explores(rseed, game_id, t, epsilon):
        if census is not None:
            census["explore"] += 1
        return list(C)
    if len(C) < 2 or e.phase != 0:           # one candidate, or the swap phase's all-zero scores: M = C
        if census is not None:
            census["swap" if e.phase != 0 else "single"] += 1
        return list(C)
    sc = turn_scores(e, C, w)
    best = max(int(sc[a]) for a in C)
    M = [a for a in C if int(sc[a]) == best]
    if census is not None:
        census["greedy"] += 1
        census["ties"] += len(M) > 1
    return M


def pick(M, rseed, game_id, t):
    """The floor(u_t |M|)-th member of M (ascending), u_t random turn t's own uniform."""
    mask = np.zeros(A, bool)
    mask[list(M)] = True
    return dg.engine_random_action(mask, rseed, game_id, t)


def guided_turn(e, w, epsilon, rseed, game_id, t, keys, census=None):
    C = DR.candidates(e)
    if not C:
        return dg.no_step(e, shuffle_keys=keys)[0]
    M = choice_set(e, C, w, epsilon, rseed, game_id, t, census)
    return dg.env_step(e, pick(M, rseed, game_id, t), shuffle_keys=keys)[0]


def rollout(env, a, seed, game_id, turn, j, rollout_steps, det, w=DEFAULT_WEIGHTS, epsilon=DEFAULT_EPSILON,
            census=None):
    """-> (outcome for the root mover's side, playout turns played); _dog_rollout.rollout with the guided turn."""
    side = DR.side_of(env)
    rseed = DR.rollout_seed(seed, game_id, turn, j)
    keys = dg.engine_shuffle_keys(rseed, game_id)
    e = DR.determinize(env, rseed) if det else env
    e = dg.env_step(e, a, shuffle_keys=keys)[0]
    t = 0
    while not e.done and t < rollout_steps:
        e = guided_turn(e, w, epsilon, rseed, game_id, t, keys, census)
        t += 1
    return DR.outcome(e, side), t


def new_census():
    return dict(explore=0, greedy=0, ties=0, swap=0, single=0)


def search_one(env, R, max_phases, rollout_steps, det, seed, turn, game_id, weights=None, epsilon=DEFAULT_EPSILON,
               census=None):
    """_dog_rollout.search_one with the guided rollout plugged in; the result also holds ``decided``, the number of
    rollouts whose outcome was not 0."""
    w = weights_of(weights)
    decided = [0]

    def fn(env_, a, seed_, game_id_, turn_, j, steps, det_):
        z, t = rollout(env_, a, seed_, game_id_, turn_, j, steps, det_, w, epsilon, census)
        decided[0] += z != 0
        return z, t

    out = DR.search_one(env, R, max_phases, rollout_steps, det, seed, turn, game_id, rollout_fn=fn)
    out["decided"] = decided[0]
    return out
