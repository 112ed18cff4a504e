"""Playing strength of the network-free MCTS agent (the 'mcts_agent' seat of evaluate.py): the first check of the tree
machinery by how it plays rather than by restatement.  GPU only, no oracle.

2 players, 256 games of play_vs_random, S = 16, rollouts of at most 300 turns.  The bar is derived, not measured:
against a random opponent a coin flip wins 128 of 256 with sigma = sqrt(256) / 2 = 8, so an agent that plays better
than random with z >= 3 wins at least 128 + 3 * 8 = 152.

Measured on MI355X: 227 of 256 wins (88.7 %), 9.4 sigma above the bar; a random agent at seat 0 of the same games
wins 127."""
import pytest

pytestmark = pytest.mark.gpu

GAMES, BAR = 256, 152


def test_mcts_agent_beats_random(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    r = EV.play_vs_random("mcts_agent", GAMES, num_players=2, num_simulations=16, max_depth=16, seed=42,
                          rollout_steps=300)
    sigma = (GAMES ** 0.5) / 2
    print(f"mcts_agent vs random, 2 players: {r['wins']} of {GAMES} wins ({100.0 * r['wins'] / GAMES:.1f} %), "
          f"{r['finished']} finished, {(r['wins'] - BAR) / sigma:+.1f} sigma from the bar of {BAR}")
    assert r["finished"] == GAMES
    assert r["wins"] >= BAR
