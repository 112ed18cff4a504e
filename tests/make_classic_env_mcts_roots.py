"""Generator of tests/golden/classic_env_mcts_roots.json: the root states of the classic network-free MCTS agent's
tests.

    python -m tests.make_classic_env_mcts_roots

Per rule set of tests/_classic_env_mcts.py RULE_SETS seeded games of oracle/classic_madn.py under the rollout policy
(the die thrown every turn from its dice_probabilities; a winning pin if there is one, else a uniformly random legal
one, no_step without a legal pin), from which 24 states are kept, each with its die thrown: the tagged ones the tests
ask for, then evenly spaced states of the games.  Tags:
  wins      a state with a winning pin (wins != 0)
  done      a finished game
  stuck     an unfinished game without a legal pin for its die
  bonus     a legal pin under a die of 6 that does not end the game and keeps the mover
  softlock  a legal pin whose afterstate's dice_probabilities are not uniform (the next player is soft-locked and the
            rules rethrow): a chance node with the 76/216 or 91/216 table
  partner   with teams: a finished player moving its partner's pins
A record is (pins [P][4], current_player, die, done, reward, tags); the board follows from the pins."""
import json

import numpy as np

from oracle import classic_madn as cm
from tests import _classic_env_mcts as CM

PER_SET = 24
GAMES = 3
TAGS = ("wins", "done", "stuck", "bonus", "softlock", "partner")


def tags_of(env):
    if env.done:
        return ["done"]
    lm = CM.legal_bits(env)
    if lm == 0:
        return ["stuck"]
    tags = []
    if CM.wins_trial(env, lm):
        tags.append("wins")
    afters = [cm.env_step(env, a)[0] for a in range(CM.A) if (lm >> a) & 1]
    if env.die == 6 and any(not s.done and s.current_player == env.current_player for s in afters):
        tags.append("bonus")
    if any(not np.array_equal(cm.dice_probabilities(s), cm.NORMAL_DICE_DISTRIBUTION) for s in afters):
        tags.append("softlock")
    if cm._sub_player(env) != env.current_player:
        tags.append("partner")
    return tags


def wanted_tags(rule_set):
    """The tags the rule set allows: softlock needs the rethrow rule, partner teams."""
    R = CM.RULE_SETS[rule_set]
    return {t for t in TAGS if (t != "softlock" or R["enable_dice_rethrow"]) and
            (t != "partner" or (R["enable_teams"] and R["num_players"] == 4))}


def play(rule_set, seed, max_plies=6000):
    """One seeded game -> [(state with its die thrown, tags)] of every turn, the final state included."""
    rng = np.random.default_rng(seed)
    env = cm.env_reset(**CM.RULE_SETS[rule_set])
    out = []
    for _ in range(max_plies):
        if env.done:
            out.append((env, tags_of(env)))
            break
        env = cm.throw_die(env, float(np.float32(rng.random())))
        out.append((env, tags_of(env)))
        lm = CM.legal_bits(env)
        if lm == 0:
            env = cm.no_step(env)[0]
            continue
        wm = CM.wins_trial(env, lm)
        cand = [a for a in range(CM.A) if ((wm if wm else lm) >> a) & 1]
        env = cm.env_step(env, int(rng.choice(cand)))[0]
    return out


def record(env, tags):
    return dict(pins=env.pins.astype(int).tolist(), current_player=int(env.current_player), die=int(env.die),
                done=bool(env.done), reward=int(env.reward), tags=tags)


def roots(rule_set, seed):
    states = [s for g in range(GAMES) for s in play(rule_set, seed + g)]
    keep, seen = [], set()

    def take(i):
        if i not in seen:
            seen.add(i)
            keep.append(states[i])

    for tag in TAGS:                                                 # the first two of each kind
        for i in [i for i, (_, t) in enumerate(states) if tag in t][:2]:
            take(i)
    for i in np.linspace(5, len(states) - 2, 64).astype(int):       # mid-game states
        if len(keep) >= PER_SET:
            break
        take(int(i))
    tags = {t for _, ts in keep for t in ts}
    assert wanted_tags(rule_set) <= tags, (rule_set, tags)
    return [record(e, t) for e, t in keep[:PER_SET]]


def main():
    out = {name: roots(name, 20270 + 100 * k) for k, name in enumerate(CM.RULE_SETS)}
    with open(CM.ROOTS, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    for name, recs in out.items():
        print(name, len(recs), "states;", {t: sum(t in r["tags"] for r in recs) for t in TAGS})


if __name__ == "__main__":
    main()
