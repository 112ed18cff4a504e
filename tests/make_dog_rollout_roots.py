"""Writes tests/golden/dog_rollout_roots.json: the root states of the DOG rollout agent's tests, generated on the CPU
from the oracle (python -m tests.make_dog_rollout_roots).  Not a test module.

The roots are late in the game (most pins in the goals, small hands), so that rollouts end in wins and losses within
a short cap.  Every rule set of tests/_dog_rollout.py gets one root per kind it can have (``wanted_tags``):

  swap_partial  the swap phase with some players' cards already chosen (teams only)
  joker         a joker in the mover's hand: many candidates, several halvings
  forced        exactly one legal action
  stuck         no legal action
  wins          some action ends the game at once for the mover's side
  deal          so few cards left that random play crosses a deal within 24 turns
  partner       a finished team player who plays from the partner's hand (teams only)

Each root is the first draw of a seeded generator of late states that has the wanted kind (rejection sampling)."""
import json

import numpy as np

from oracle import dog as dg
from tests import _dog_rollout as DR

KINDS = ("swap_partial", "joker", "forced", "stuck", "wins", "deal", "partner")


def wanted_tags(rule_set):
    teams = DR.RULE_SETS[rule_set]["enable_teams"]
    return {k for k in KINDS if teams or k not in ("swap_partial", "partner")}


def late_state(rng, rule_set, kind):
    kw = DR.RULE_SETS[rule_set]
    env = dg.env_reset(shuffle_keys=dg.engine_shuffle_keys(7, 0), **kw)
    P = env.num_players
    teams = env.rules["enable_teams"]
    cp = int(rng.integers(0, P))
    # three pins of every player in its goal, and with teams one finished player per team: a game from here ends
    # within a few dozen random turns
    in_goal = [3] * P
    if teams:
        in_goal[int(rng.integers(0, 2)) * 2] = 4
        in_goal[int(rng.integers(0, 2)) * 2 + 1] = 4
        cp = int(rng.choice([p for p in range(P) if in_goal[p] == 3]))
    if kind == "partner":
        in_goal[cp] = 4
        in_goal[(cp + 2) % 4] = 3
    if kind == "wins" and teams:
        in_goal[(cp + 2) % 4] = 4
    pins = -np.ones((P, 4), np.int32)
    used = set()
    for p in range(P):
        for k in range(4):
            if k < in_goal[p]:
                pins[p, k] = env.goal[p][3 - k]                         # the deepest goal cells first
            elif rng.random() < 0.75:
                free = [c for c in range(40) if c not in used]
                if kind == "wins" and p == cp:                          # close before the goal entry
                    near = [(env.target[p] - d) % 40 for d in range(0, 8)]
                    free = [c for c in near if c not in used] or free
                pins[p, k] = int(free[int(rng.integers(0, len(free)))])
                used.add(int(pins[p, k]))
    board = dg.set_pins_on_board(-np.ones(56, np.int8), pins)
    # hands dealt from a full deck, the rest partly discarded
    full = np.repeat(np.arange(14), [6] + [8] * 13)
    rng.shuffle(full)
    h = 1 if kind in ("forced", "stuck") else (int(rng.integers(1, 3)) if kind == "deal" else int(rng.integers(2, 4)))
    hands = np.zeros((P, 14), np.int8)
    for p in range(P):
        for c in full[p * h:(p + 1) * h]:
            hands[p, c] += 1
    rest = full[P * h:]
    deck = np.bincount(rest[:int(rng.integers(P * 6, len(rest)))], minlength=14).astype(np.int8)
    mover = (cp + 2) % 4 if kind == "partner" else cp
    if kind == "joker" and hands[mover, 0] == 0:                         # swap one of the mover's cards for a joker
        c = int(np.flatnonzero(hands[mover])[0])
        if deck[0] > 0:
            hands[mover, c] -= 1
            hands[mover, 0] += 1
            deck[0] -= 1
            deck[c] += 1
    env = env.replace(pins=pins, board=board, hands=hands, deck=deck, current_player=cp,
                      round_starter=int(rng.integers(0, P)), phase=0, hand_size=int(rng.integers(2, 7)),
                      deal=int(rng.integers(3, 10)), swap_choices=np.full(4, -1, np.int8), reward=0, done=False)
    if kind == "swap_partial":                                           # round starter and the next seat have chosen
        rs = int(rng.integers(0, 4))
        env = env.replace(phase=1, round_starter=rs, current_player=rs)
        for _ in range(int(rng.integers(1, 4))):
            card = int(rng.choice(np.flatnonzero(env.hands[env.current_player] > 0)))
            env = dg.env_step(env, 792 + card)[0]
    return env


def crosses_a_deal(env, steps=24):
    """Rollout 0 of the first candidate under the test's keys deals within ``steps`` random turns."""
    C = DR.candidates(env)
    if not C:
        return False
    rseed = DR.rollout_seed(11, 0, 3, 0)
    keys = dg.engine_shuffle_keys(rseed, 0)
    e = dg.env_step(env, C[0], shuffle_keys=keys)[0]
    t = 0
    while not e.done and t < steps and e.deal == env.deal:
        a = dg.engine_random_action(dg.valid_actions(e), rseed, 0, t)
        e = dg.no_step(e, shuffle_keys=keys)[0] if a < 0 else dg.env_step(e, a, shuffle_keys=keys)[0]
        t += 1
    return e.deal > env.deal


def winning_actions(env):
    side = DR.side_of(env)
    out = []
    for a in DR.candidates(env):
        e = dg.env_step(env, a, shuffle_keys=dg.engine_shuffle_keys(0, 0))[0]
        if e.done and DR.outcome(e, side) == 1:
            out.append(a)
    return out


def tags_of(env, only=None):
    """Every kind the root has (a root made for one kind often has others too); ``only``: just that kind."""
    if only is not None:
        return {only} & _cheap_tags(env) if only in ("swap_partial", "joker", "forced", "stuck", "partner") else \
            ({"wins"} if env.phase == 0 and winning_actions(env) else set()) if only == "wins" else \
            ({"deal"} if crosses_a_deal(env) else set())
    return _cheap_tags(env) | tags_of(env, "wins") | tags_of(env, "deal")


def _cheap_tags(env):
    C = DR.candidates(env)
    tags = set()
    if env.phase == 1 and (env.swap_choices >= 0).any():
        tags.add("swap_partial")
    if env.phase == 0 and env.hands[dg.sub_player(env), 0] > 0 and len(C) >= 6:
        tags.add("joker")
    if len(C) == 1:
        tags.add("forced")
    if not env.done and not C:
        tags.add("stuck")
    if dg.sub_player(env) != env.current_player:
        tags.add("partner")
    return tags


def roots_of(rule_set, max_candidates=8):
    rng = np.random.default_rng(sorted(DR.RULE_SETS).index(rule_set) + 2024)
    recs = []
    for kind in KINDS:
        if kind not in wanted_tags(rule_set):
            continue
        for _ in range(4000):
            env = late_state(rng, rule_set, kind)
            if len(DR.candidates(env)) > max_candidates:               # keeps the Python restatement quick
                continue
            if kind not in ("forced", "stuck") and len(DR.candidates(env)) < 2:   # a root that is searched
                continue
            if kind in tags_of(env, kind):
                recs.append(DR.record_of(env, tags_of(env)))
                break
        else:
            raise RuntimeError(f"no {kind} root for {rule_set}")
    return recs


if __name__ == "__main__":
    data = {rs: roots_of(rs) for rs in DR.RULE_SETS}
    with open(DR.ROOTS, "w") as fh:
        json.dump(data, fh, separators=(",", ":"))
        fh.write("\n")
    for rs, recs in data.items():
        print(rs, [(r["tags"], len(DR.candidates(DR.state_from_record(rs, r)))) for r in recs])
