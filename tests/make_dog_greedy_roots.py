"""Writes tests/golden/dog_greedy_roots.json: the root states of the DOG greedy agent's tests, taken from oracle play
on the CPU (python -m tests.make_dog_greedy_roots).  Not a test module.

Every rule set of tests/_dog_rollout.py plays a few seeded games in which greedy seats (tests/_dog_greedy.py, sampled
at the default temperature) and random seats (engine_random_action) are mixed -- seat p of game k is greedy when k + p
is even -- so that opening, mid-game and late positions all occur.  Every position of those games (and each game's
final state) is tagged with the kinds of root and candidate the tests need:

  many        at least 60 candidates
  hot7_hit    a hot-7 candidate with hit > 0
  swap_both   a pin-swap candidate that changes both advance and setback
  joker       a joker copy among the candidates (an action below 396)
  neg4        a -4 move among the candidates
  swap_phase  a root in the swap phase (teams only)
  finished    a finished game
  stuck       an unfinished game with nothing legal
  win         a candidate with win = +1
  partner     a team player who has finished and plays the partner's pins (teams only)
  self_hit    a candidate with out < 0: a 7 that sends a pin of the mover's own side home

A rule set's roots are, in the order of play, the first position that shows each kind not shown before, then every
STRIDE-th position until the set holds PER_SET roots.  self_hit turned up in every rule set within the three games
played here (the whole script takes about 17 s): a 7 whose path crosses a pin of the mover's own sends it home with
or without enable_friendly_fire.  So it is part of the coverage the script and tests/test_dog_greedy_host.py
assert."""
import json

import numpy as np

from oracle import dog as dg
from tests import _dog_greedy as G
from tests import _dog_rollout as DR

KINDS = ("many", "hot7_hit", "swap_both", "joker", "neg4", "swap_phase", "finished", "stuck", "win", "partner",
         "self_hit")
GAMES, PER_SET, STRIDE, SEED = 3, 12, 97, 2025
MAX_BYTES = 64 * 1024


def kind_of(a):
    """'card' (swap phase), else 'swap' / 'hot7' / 'normal' / 'neg' of the play action."""
    if a >= 792:
        return "card"
    i = a % 396
    return "swap" if i < 224 else ("hot7" if i < 344 else ("normal" if i < 392 else "neg"))


def tags_of(env, root=None):
    C, F = G.evaluate_root(env) if root is None else root
    tags = set()
    if len(C) >= 60:
        tags.add("many")
    if any(kind_of(a) == "hot7" and F[a, 4] > 0 for a in C):
        tags.add("hot7_hit")
    if any(kind_of(a) == "swap" and F[a, 0] != 0 and F[a, 1] != 0 for a in C):
        tags.add("swap_both")
    if any(a < 396 for a in C):
        tags.add("joker")
    if any(kind_of(a) == "neg" for a in C):
        tags.add("neg4")
    if env.phase == 1 and not env.done:
        tags.add("swap_phase")
    if env.done:
        tags.add("finished")
    if not env.done and not C:
        tags.add("stuck")
    if any(F[a, 5] == 1 for a in C):
        tags.add("win")
    if C and env.phase == 0 and dg.sub_player(env) != env.current_player:
        tags.add("partner")
    if any(F[a, 3] < 0 for a in C):
        tags.add("self_hit")
    return tags


def wanted_tags():
    return set(KINDS)


def positions(rule_set, game):
    """Every position of one game in the order of play, the final state last: (state, evaluate_root(state))."""
    seed = SEED + sorted(DR.RULE_SETS).index(rule_set)
    keys = dg.engine_shuffle_keys(seed, game)
    kw = DR.RULE_SETS[rule_set]
    env = dg.env_reset(starting_player=game % kw["num_players"], shuffle_keys=keys, **kw)
    for t in range(2000):
        root = G.evaluate_root(env)
        yield env, root
        if env.done:
            return
        if (game + env.current_player) % 2 == 0:
            a = G.greedy_one(env, None, seed, t, game, root=root)["action"]
        else:
            a = dg.engine_random_action(dg.valid_actions(env), seed, game, t)
        env = dg.no_step(env, shuffle_keys=keys)[0] if a < 0 else dg.env_step(env, a, shuffle_keys=keys)[0]


def roots_of(rule_set):
    recs, seen, filler = [], set(), []
    n = 0
    for game in range(GAMES):
        for env, root in positions(rule_set, game):
            tags = tags_of(env, root)
            n += 1
            if tags - seen:
                seen |= tags
                recs.append(DR.record_of(env, tags))
            elif n % STRIDE == 0:
                filler.append(DR.record_of(env, tags))
    return recs + filler[:max(0, PER_SET - len(recs))]


if __name__ == "__main__":
    data = {rs: roots_of(rs) for rs in DR.RULE_SETS}
    with open(G.ROOTS, "w") as fh:
        json.dump(data, fh, separators=(",", ":"))
        fh.write("\n")
    size = len(json.dumps(data, separators=(",", ":"))) + 1
    for rs, recs in data.items():
        print(rs, len(recs), [(r["tags"], len(DR.candidates(DR.state_from_record(rs, r)))) for r in recs])
    have = {t for recs in data.values() for r in recs for t in r["tags"]}
    assert all(len(recs) >= 8 for recs in data.values()), {rs: len(recs) for rs, recs in data.items()}
    assert wanted_tags() <= have, wanted_tags() - have
    assert size < MAX_BYTES, size
    print("bytes", size)
