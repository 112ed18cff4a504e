"""The DOG rollout agent restated in NumPy on oracle/dog.py (TEST INFRASTRUCTURE; not a test module).

This file is the DEFINITION of muz_dog_rollout_search (csrc/dog_rollout.hip, dog.rollout_policy, the 'rollout_agent'
seat): the reference has no DOG agent that runs, so parity with the reference is UNPINNED and the kernels must equal
this restatement bit for bit (every result is an integer sum; the value is one float32 division).

For one root game with ``game_id``, ``turn`` and ``seed``:

  m = the current player, m' = sub_player(m) (the partner whose hand a finished team player plays from); the
  OBSERVERS are {m, m'}; the SIDE is m & 1 with enable_teams, else the seat m; C0 = the legal actions
  (valid_actions), ascending.

  A game that is done, or whose C0 is empty: action -1, all visits 0, value 0.  |C0| == 1: that action, no rollout,
  visits 0, value 0.

  Phases p = 0, 1, .. until ``max_phases`` have run or one candidate is left.  In phase p every candidate a of Cp gets
  R rollouts j = p R .. p R + R - 1, so all of Cp have the same visit count afterwards.  The candidates are ranked by
  wins[a] (int32 sum of outcomes) descending, ties by the smaller action; C(p+1) = the best ceil(|Cp| / 2).  The
  action is the best candidate of the last ranked set, value = float32(wins) / float32(visits) of it.

  Rollout (a, j): copy the root; with ``determinize`` re-draw the hidden cards (``determinize``); apply a with
  env_step (and the deal it asks for); if that ends the game the outcome is decided, else play random turns
  (engine_random_action over valid_actions, no_step when nothing is legal) t = 0, 1, .. until the game is done or
  ``rollout_steps`` turns are played.  Outcome: +1 when get_winner of the final board holds the side, -1 when it is
  non-empty and does not, 0 otherwise (the cap).  ``turns`` counts the random turns (the root action is not one).

  Random numbers: rollout j has the seed ``rollout_seed(seed, game_id, turn, j)`` and draws the engine's own streams
  under it -- engine_shuffle_keys(rseed, game_id) for its deals, engine_random_action(mask, rseed, game_id, t) for
  random turn t -- and ``det_uniform(rseed, i)`` for the i-th draw of its determinization.  Nothing is keyed by the
  action a (the candidates of a phase share their random numbers) or by the game's position in a batch.

  Determinization: the hidden multiset H (counts over the 14 cards) = deck + the hands of every seat that is not an
  observer + one card for every such seat q with 0 <= swap_choices[q] < 14 (in the swap phase a chosen card has left
  the hand; the exchange comes later).  For those seats q ascending: draw as many cards as q's hand holds, then q's swap
  choice if it had one; each draw takes the floor(u |H|)-th card of H in card order, without replacement.  What is left
  of H becomes the deck.  Nothing else changes.  The mover also knows the card it gave away in the swap phase; that
  knowledge is ignored (the partner's hand is re-drawn like any hidden hand).
"""
import json
import os

import numpy as np

from oracle import dog as dg
from oracle.dog import M64, _game_key, _mix64, _u24

A = 806
ROLLOUT_STREAM = 0xD06B0110A7
ROLLOUT_MUL = 0xC2B2AE3D27D4EB4F
DET_STREAM = 0xD06DE7E5
DET_MUL = 0x9FB21C651E98DF25

ROOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dog_rollout_roots.json")
RULE_SETS = {
    "selfplay_4p_teams": dict(num_players=4, **dg.SELFPLAY_RULES),                             # the default teams set
    "selfplay_4p_noteams": dict(num_players=4, **{**dg.SELFPLAY_RULES, "enable_teams": False}),
    "exotic_3p": dict(num_players=3, enable_teams=False, enable_initial_free_pin=True, enable_circular_board=False,
                      enable_start_blocking=True, enable_jump_in_goal_area=False, enable_friendly_fire=False,
                      must_traverse_start=False),                                               # tests/dog_states.py
}


# ---- streams --------------------------------------------------------------------------------------------------------
def rollout_seed(seed, game_id, turn, j):
    return _mix64(_game_key((seed & M64) ^ ROLLOUT_STREAM, game_id, turn) ^ (((j + 1) * ROLLOUT_MUL) & M64))


def det_uniform(rseed, i):
    return _u24(_mix64(rseed ^ DET_STREAM ^ (((i + 1) * DET_MUL) & M64)))


# ---- the pieces -----------------------------------------------------------------------------------------------------
def observers(env):
    return {int(env.current_player), int(dg.sub_player(env))}


def side_of(env):
    return (env.current_player & 1) if env.rules["enable_teams"] else int(env.current_player)


def candidates(env):
    if env.done:
        return []
    return [int(a) for a in np.flatnonzero(np.asarray(dg.valid_actions(env), bool))]


def hidden_seats(env):
    obs = observers(env)
    return [q for q in range(env.num_players) if q not in obs]


def hidden_multiset(env):
    H = env.deck.astype(np.int64).copy()
    for q in hidden_seats(env):
        H += env.hands[q].astype(np.int64)
        sc = int(env.swap_choices[q])
        if 0 <= sc < env.num_cards:
            H[sc] += 1
    return H


def determinize(env, rseed):
    H = hidden_multiset(env)
    hands = env.hands.copy()
    choices = env.swap_choices.copy()
    i = 0

    def draw():
        nonlocal i
        tot = int(H.sum())
        k = min(int(np.float32(det_uniform(rseed, i)) * np.float32(tot)), tot - 1)
        i += 1
        card = int(np.searchsorted(np.cumsum(H), k, side="right"))
        H[card] -= 1
        return card

    for q in hidden_seats(env):
        n = int(env.hands[q].astype(np.int64).sum())
        hands[q] = 0
        for _ in range(n):
            hands[q, draw()] += 1
        if 0 <= int(env.swap_choices[q]) < env.num_cards:
            choices[q] = draw()
    return env.replace(hands=hands.astype(np.int8), swap_choices=choices.astype(np.int8), deck=H.astype(np.int8))


def outcome(env, side):
    w = np.asarray(dg.get_winner(env, env.board), bool)
    if not w.any():
        return 0
    return 1 if w[side] else -1


def rollout(env, a, seed, game_id, turn, j, rollout_steps, det):
    """-> (outcome for the root mover's side, random turns played)."""
    side = side_of(env)
    rseed = rollout_seed(seed, game_id, turn, j)
    keys = dg.engine_shuffle_keys(rseed, game_id)
    e = determinize(env, rseed) if det else env
    e = dg.env_step(e, a, shuffle_keys=keys)[0]
    t = 0
    while not e.done and t < rollout_steps:
        act = dg.engine_random_action(dg.valid_actions(e), rseed, game_id, t)
        e = dg.no_step(e, shuffle_keys=keys)[0] if act < 0 else dg.env_step(e, act, shuffle_keys=keys)[0]
        t += 1
    return outcome(e, side), t


def rank(cands, wins):
    """The candidates by (wins descending, action ascending)."""
    return sorted(cands, key=lambda a: (-int(wins[a]), a))


def search_one(env, R, max_phases, rollout_steps, det, seed, turn, game_id, rollout_fn=rollout):
    """-> dict(action, value float32, visits int32[806], wins int32[806], turns, sets = [C0, C1, ..])."""
    visits, wins = np.zeros(A, np.int32), np.zeros(A, np.int32)
    out = dict(action=-1, value=np.float32(0), visits=visits, wins=wins, turns=0, sets=[])
    C = candidates(env)
    out["sets"].append(list(C))
    if len(C) < 2:
        out["action"] = C[0] if C else -1
        return out
    for p in range(max_phases):
        for a in C:
            for j in range(p * R, p * R + R):
                z, t = rollout_fn(env, a, seed, game_id, turn, j, rollout_steps, det)
                wins[a] += z
                visits[a] += 1
                out["turns"] += t
        order = rank(C, wins)
        out["action"] = order[0]
        out["value"] = np.float32(wins[order[0]]) / np.float32(visits[order[0]])
        C = order[:(len(C) + 1) // 2]
        out["sets"].append(list(C))
        if len(C) == 1:
            break
    return out


# ---- the fixture ----------------------------------------------------------------------------------------------------
def record_of(env, tags):
    return dict(tags=sorted(tags), board=env.board.tolist(), pins=env.pins.tolist(), deck=env.deck.tolist(),
                hands=env.hands.tolist(), swap_choices=env.swap_choices.tolist(),
                current_player=int(env.current_player), round_starter=int(env.round_starter), phase=int(env.phase),
                hand_size=int(env.hand_size), reward=int(env.reward), done=bool(env.done), deal=int(env.deal))


def state_from_record(rule_set, r):
    base = dg.env_reset(shuffle_keys=dg.engine_shuffle_keys(0, 0), **RULE_SETS[rule_set])
    return base.replace(board=np.array(r["board"], np.int8), pins=np.array(r["pins"], np.int32),
                        deck=np.array(r["deck"], np.int8), hands=np.array(r["hands"], np.int8),
                        swap_choices=np.array(r["swap_choices"], np.int8), current_player=r["current_player"],
                        round_starter=r["round_starter"], phase=r["phase"], hand_size=r["hand_size"],
                        reward=r["reward"], done=r["done"], deal=r["deal"])


def load_roots(rule_set):
    """-> (oracle states, their tag lists) of one rule set of tests/golden/dog_rollout_roots.json."""
    with open(ROOTS) as fh:
        recs = json.load(fh)[rule_set]
    return [state_from_record(rule_set, r) for r in recs], [r["tags"] for r in recs]
