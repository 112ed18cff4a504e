"""Generator of tests/golden/env_mcts_roots.json: the root states of the network-free MCTS agent's tests.

    python -m tests.make_env_mcts_roots

Per rule set (2 players with oracle/detmadn.py's default rules; 4 players in teams with the self-play rules) seeded
games of oracle/detmadn.py under the rollout policy of tests/_env_mcts.py (a winning action if there is one, else a
uniformly random legal one, no_step without a legal action), from which 24 states are kept: the tagged ones the tests
ask for, then evenly spaced states of the games.  Tags:
  wins      a state with a winning action (wins != 0)
  done      a finished game
  stuck     an unfinished game without a legal action
  pass      a state with a legal action whose transition passes through a no-move turn
  bonus     a state right after a move of 6 (the same player moves again)
A record is (pins [P][4], action_set [P][6], current_player, done, reward, tags); the board follows from the pins."""
import json

import numpy as np

from oracle import detmadn as dm
from tests import _env_mcts as EM

PER_SET = 24
GAMES = 3


def play(rule_set, seed, max_plies=4000):
    """One seeded game -> [(state, tags)] of every state met, the final one included."""
    rng = np.random.default_rng(seed)
    env = dm.env_reset(**EM.RULE_SETS[rule_set])
    out, after6 = [], False
    for _ in range(max_plies):
        lm = EM.legal_bits(env)
        tags = []
        if env.done:
            out.append((env, ["done"]))
            break
        if after6:
            tags.append("bonus")
        if lm == 0:
            out.append((env, tags + ["stuck"]))
            env, after6 = dm.no_step(env)[0], False
            continue
        wm = EM.wins_trial(env, lm)
        if wm:
            tags.append("wins")
        out.append((env, tags))
        cand = np.flatnonzero(EM.bits_to_bool(wm if wm else lm))
        a = int(rng.choice(cand))
        player = env.current_player
        env = dm.env_step(env, dm.map_action(a))[0]
        after6 = a % 6 == 5 and not env.done and env.current_player == player
    return out


def has_pass(env):
    lm = EM.legal_bits(env)
    return any((lm >> a) & 1 and EM.transition(env, a)[3] > 0 for a in range(EM.A))


def record(env, tags):
    return dict(pins=env.pins.astype(int).tolist(), action_set=env.action_set.astype(int).tolist(),
                current_player=int(env.current_player), done=bool(env.done), reward=int(env.reward), tags=tags)


def roots(rule_set, seed):
    states = [s for g in range(GAMES) for s in play(rule_set, seed + g)]
    keep, seen = [], set()

    def take(i, extra=()):
        if i not in seen:
            seen.add(i)
            keep.append((states[i][0], sorted(set(states[i][1]) | set(extra))))

    for tag in ("wins", "done", "stuck", "bonus"):                 # the first two of each kind
        for i in [i for i, (_, t) in enumerate(states) if tag in t][:2]:
            take(i)
    found = 0
    for i, (env, t) in enumerate(states):                            # trial transitions: stop at the first two
        if not env.done and "stuck" not in t and has_pass(env):
            take(i, ["pass"])
            found += 1
            if found == 2:
                break
    for i in np.linspace(5, len(states) - 2, 64).astype(int):       # mid-game states
        if len(keep) >= PER_SET:
            break
        take(int(i))
    tags = {t for _, ts in keep for t in ts}
    assert {"wins", "done", "stuck", "pass", "bonus"} <= tags, (rule_set, tags)
    return [record(e, t) for e, t in keep[:PER_SET]]


def main():
    out = {name: roots(name, 20260 + 100 * k) for k, name in enumerate(EM.RULE_SETS)}
    with open(EM.ROOTS, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    for name, recs in out.items():
        print(name, len(recs), "states;", {t: sum(t in r["tags"] for r in recs) for t in
                                           ("wins", "done", "stuck", "pass", "bonus")})


if __name__ == "__main__":
    main()
