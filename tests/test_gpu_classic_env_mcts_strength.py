"""Playing strength of the classic network-free MCTS agent (the 'stochastic_mcts_agent' seat of evaluate.py): the
check of the decision / chance tree, its value signs and its team discounts by how it plays rather than by
restatement.  GPU only, no oracle.

4 players in teams under evaluate.CLASSIC_RULES, 256 games of play_vs_random_classic, the agent at seats 0 + 2, S = 16,
D = 16, seed 42.  The bar is derived, not measured: against random opponents a coin flip wins 128 of 256 with sigma =
sqrt(256) / 2 = 8, so an agent that plays better than random with z >= 3 wins at least 128 + 3 * 8 = 152; an
unfinished game counts as not won.

Measured on MI355X with rollouts of at most 300 turns (the reference's cap): 158 of 256 wins (61.7 %), 256 finished,
+0.8 sigma above the bar (3.75 sigma above a coin flip); the test takes 65.5 s.

ROLLOUT_STEPS stays 300 although the test is far above 10 s.  Lowering the cap was measured on the same games and it
takes the agent under the bar, because a rollout that stops at the cap is worth 0 and dice games rarely end within a
few dozen turns:
    rollout_steps   30    40    50    60    80    300
    wins           139   131   143   141   143    158
    seconds       12.1  14.3  17.1  19.5  25.8   65.5
Even at 30 the test is above 10 s: about 4 s is the turn loop, the rest the searches, whose time is each game's serial
chain of rollout turns (14.65 us per turn with the environment in one lane; each turn of the loop
launches one search per agent seat over at most 128 games, so the GPU is nearly empty and only that latency counts).
The bar and the game count are not lowered; what brings the time down is a faster rollout turn."""
import time

import pytest

pytestmark = pytest.mark.gpu

GAMES, BAR = 256, 152
ROLLOUT_STEPS = 300


def test_stochastic_mcts_agent_beats_random(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    t0 = time.perf_counter()
    r = EV.play_vs_random_classic("stochastic_mcts_agent", GAMES, num_simulations=16, max_depth=16, seed=42,
                                  rollout_steps=ROLLOUT_STEPS)
    dt = time.perf_counter() - t0
    sigma = (GAMES ** 0.5) / 2
    print(f"stochastic_mcts_agent vs random, 4 players in teams: {r['wins']} of {GAMES} wins "
          f"({100.0 * r['wins'] / GAMES:.1f} %), {r['finished']} finished, {(r['wins'] - BAR) / sigma:+.1f} sigma from "
          f"the bar of {BAR}, {dt:.1f} s")
    assert r["wins"] >= BAR
