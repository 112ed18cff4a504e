"""The 'rollout_agent' seat of evaluate_agent_parallel_dog on the GPU: the same evaluation twice gives the same tables,
and the agent's team beats random play.  GPU only, no oracle.

Strength: seats 0 + 2 play 'rollout_agent', seats 1 + 3 'random_agent', GAMES games in total over the four starting
blocks under evaluate.DOG_RULES (teams).  The bar is derived, not measured: the team's wins must reach the smallest k
with P(Bin(GAMES, 1/2) >= k) < 1e-3, computed here with math.comb; an unfinished game counts as not won.  At 256 games
that k is 154 (P(X >= 154) = 0.00069; P(X >= 153) = 0.00107 is not below 1e-3), above the 152 = 128 + 3 sigma of the
project's other strength tests (P(X >= 152) = 0.0016): the formula sets the bar, the stricter one.

Measured on MI355X with the defaults (4 rollouts per action and phase, rollouts of at most 300 turns, determinized),
seed 42: 241 of 256 wins (94.1 %), 256 finished in 1018 turns; the test takes 10.7 s, under the 15 s at which the
game count would be halved (64 games: 61 wins in 8.6 s -- the time is the serial chain of the games' turns, not the
batch; rollout_steps = 100: 230 of 256 in 5.1 s)."""
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES = 256
ROLLOUTS, ROLLOUT_STEPS = 4, 300
SEATS = ["rollout_agent", "random_agent"] * 2


def bar(n: int, p: float = 1e-3) -> int:
    """The smallest k with P(Bin(n, 1/2) >= k) < p."""
    tail, total = 0, 2 ** n
    for k in range(n, -1, -1):
        tail += math.comb(n, k)
        if tail >= p * total:
            return k + 1
    return 0


def test_the_bar_is_the_binomial_tail():
    assert bar(256) == 154 and bar(128) == 82 and bar(64) == 45
    for n in (64, 128, 256):
        k = bar(n)
        tail = lambda j: sum(math.comb(n, i) for i in range(j, n + 1)) / 2 ** n   # noqa: E731
        assert tail(k) < 1e-3 <= tail(k - 1)


def test_evaluation_is_deterministic(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    runs = [EV.evaluate_agent_parallel_dog(SEATS, batch_size=4, seed=3, max_turns=40, rollouts=2, rollout_steps=24)
            for _ in range(2)]
    a, b = runs
    for k in ("winners", "average_progress", "wins_per_player", "progress_per_player", "finished", "turns"):
        assert a[k] == b[k], k
    sa, sb = a["final_state"], b["final_state"]
    for k in ("board", "pins", "hands", "deck", "current_player", "deal"):
        assert torch.equal(getattr(sa, k), getattr(sb, k)), k
    assert a["turns"] == 40 and bool((sa.pins >= 0).any())


def test_rollout_agent_beats_random(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    t0 = time.perf_counter()
    r = EV.evaluate_agent_parallel_dog(SEATS, batch_size=GAMES // 4, seed=42, rollouts=ROLLOUTS,
                                       rollout_steps=ROLLOUT_STEPS)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    wins, need = r["wins_per_player"][0], bar(GAMES)
    print(f"rollout_agent (seats 0 + 2) vs random, teams: {wins} of {GAMES} wins ({100.0 * wins / GAMES:.1f} %), "
          f"{r['finished']} finished in {r['turns']} turns, bar {need}, rollouts {ROLLOUTS}, rollout_steps "
          f"{ROLLOUT_STEPS}, {dt:.1f} s")
    assert r["wins_per_player"][0] == r["wins_per_player"][2]          # a team wins together
    assert wins >= need
