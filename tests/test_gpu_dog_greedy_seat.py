"""The 'greedy_agent' seat of evaluate_agent_parallel_dog on the GPU: the same evaluation twice gives the same tables,
the agent's team beats random play, and the seat is DOG's alone.  GPU only, no oracle.

Strength: seats 0 + 2 play 'greedy_agent' with its defaults (dog.GREEDY_DEFAULTS), seats 1 + 3 'random_agent', GAMES
games in total over the four starting blocks under evaluate.DOG_RULES (teams).  The bar is derived, not measured: the
team's wins must reach the smallest k with P(Bin(GAMES, 1/2) >= k) < 1e-3 (tests/_dog_greedy.py binomial_bar, the
formula of tests/test_gpu_dog_rollout_seat.py), 154 at 256 games; an unfinished game counts as not won.  The game
count would be halved if the test took over 15 s, as the rollout seat's test documents; the docstring of
test_greedy_agent_beats_random records what was measured."""
import time

import pytest
import torch

from tests._dog_greedy import binomial_bar

pytestmark = pytest.mark.gpu

GAMES = 256
SEATS = ["greedy_agent", "random_agent"] * 2


def test_evaluation_is_deterministic(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    runs = [EV.evaluate_agent_parallel_dog(SEATS, batch_size=4, seed=3, max_turns=60) for _ in range(2)]
    a, b = runs
    for k in ("winners", "average_progress", "wins_per_player", "progress_per_player", "finished", "turns"):
        assert a[k] == b[k], k
    sa, sb = a["final_state"], b["final_state"]
    for k in ("board", "pins", "hands", "deck", "current_player", "deal"):
        assert torch.equal(getattr(sa, k), getattr(sb, k)), k
    assert a["turns"] == 60 and bool((sa.pins >= 0).any())
    # the seat's parameters reach the kernel: other weights, another game
    c = EV.evaluate_agent_parallel_dog(SEATS, batch_size=4, seed=3, max_turns=60,
                                       greedy=dict(advance=-1, setback=-1, goal=-20, out=-15, hit=-10, temperature=0.0))
    assert not torch.equal(c["final_state"].pins, sa.pins)


def test_greedy_agent_beats_random(cuda):
    """Measured on MI355X with the defaults, seed 42: 256 of 256 wins, 256 finished in 773 turns; the test takes
    0.2 s, far under the 15 s at which the game count would be halved."""
    from exploring_muzero_on_dog_amd import evaluate as EV
    t0 = time.perf_counter()
    r = EV.evaluate_agent_parallel_dog(SEATS, batch_size=GAMES // 4, seed=42)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    wins, need = r["wins_per_player"][0], binomial_bar(GAMES)
    print(f"greedy_agent (seats 0 + 2) vs random, teams: {wins} of {GAMES} wins ({100.0 * wins / GAMES:.1f} %), "
          f"{r['finished']} finished in {r['turns']} turns, bar {need}, {dt:.1f} s")
    assert need == 154
    assert r["wins_per_player"][0] == r["wins_per_player"][2]          # a team wins together
    assert wins >= need


def test_the_seat_is_dogs_alone(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    with pytest.raises(ValueError, match="greedy agent") as e:
        EV.evaluate_agent_parallel(["greedy_agent", "random_agent"] * 2, batch_size=1)
    assert "'rule_based_agent'" in str(e.value) and "det-MADN" in str(e.value)
    with pytest.raises(ValueError, match="greedy agent") as e:
        EV.evaluate_agent_parallel_classic(["greedy_agent", "random_agent"] * 2, batch_size=1)
    assert "'rule_based_agent'" in str(e.value) and "classic MADN" in str(e.value)
    with pytest.raises(ValueError) as e:
        EV.evaluate_agent_parallel_dog(["rule_based_agent", "random_agent"] * 2, batch_size=1)
    assert str(e.value) == ("MuZero_DOG/evaluate_agent.py's rule-based agent reshapes the 806-action mask to (4, 6) and "
                            "cannot run; use 'random_agent' or a MuZero agent")
