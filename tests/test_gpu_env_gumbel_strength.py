"""Playing strength of the Gumbel network-free MCTS agent (the 'gumbel_mcts_agent' seat of evaluate.py): the Gumbel
tree arithmetic -- sequential halving at the root, completed Q-values, softmax - visit share inside -- judged on real
game values by how it plays rather than by restatement.  GPU only, no oracle.

2 players, 256 games of play_vs_random, S = 16, rollouts of at most 300 turns: tests/test_gpu_env_mcts_strength.py's
call with the other seat.  The bar is derived, not measured: against a random opponent a coin flip wins 128 of 256 with
sigma = sqrt(256) / 2 = 8, so an agent that plays better than random with z >= 3 wins at least 128 + 3 * 8 = 152.

Measured on MI355X: 236 of 256 wins (92.2 %), 10.5 sigma above the bar, in 1.3 s; in the same session the 'mcts_agent'
seat won 227 of the same games in 1.2 s, so rollout_steps stays 300 (profiles/env_gumbel_bench.log, which also has
qtransform="min_max": 233)."""
import pytest

pytestmark = pytest.mark.gpu

GAMES, BAR = 256, 152


def test_gumbel_mcts_agent_beats_random(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    r = EV.play_vs_random("gumbel_mcts_agent", GAMES, num_players=2, num_simulations=16, max_depth=16, seed=42,
                          rollout_steps=300)
    sigma = (GAMES ** 0.5) / 2
    print(f"gumbel_mcts_agent vs random, 2 players: {r['wins']} of {GAMES} wins ({100.0 * r['wins'] / GAMES:.1f} %), "
          f"{r['finished']} finished, {(r['wins'] - BAR) / sigma:+.1f} sigma from the bar of {BAR}")
    assert r["finished"] == GAMES
    assert r["wins"] >= BAR
