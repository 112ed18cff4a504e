"""The 'guided_rollout_agent' seat of evaluate_agent_parallel_dog on the GPU: the same evaluation twice gives the same
tables, other ``guided`` parameters give another game, the seat is DOG's alone, and the agent's team beats random play.
GPU only, no oracle.

Strength: seats 0 + 2 play 'guided_rollout_agent', seats 1 + 3 'random_agent', 64 games in total over the four starting
blocks under evaluate.DOG_RULES (teams), rollouts of at most 100 turns, seed 42.  The bar is derived, not measured: the
team's wins must reach binomial_bar(64) = 45, the smallest k with P(Bin(64, 1/2) >= k) < 1e-3 (tests/_dog_greedy.py);
an unfinished game counts as not won.

Measured on MI355X with the defaults otherwise (4 rollouts per action and phase, epsilon 0.125, the greedy agent's
default weights, determinized): 61 of 64 wins (95.3 %), 64 finished in 1110 turns; the test takes 7.7 s, under the 15 s at
which rollout_steps would be halved."""
import time

import pytest
import torch

from tests._dog_greedy import binomial_bar

pytestmark = pytest.mark.gpu

GAMES = 64
ROLLOUTS, ROLLOUT_STEPS = 4, 100
SEATS = ["guided_rollout_agent", "random_agent"] * 2
TABLES = ("winners", "average_progress", "wins_per_player", "progress_per_player", "finished", "turns")
STATE = ("board", "pins", "hands", "deck", "current_player", "deal")


def _run(**kw):
    from exploring_muzero_on_dog_amd import evaluate as EV
    kw = dict(dict(batch_size=4, seed=3, max_turns=40, rollouts=2, rollout_steps=24), **kw)
    return EV.evaluate_agent_parallel_dog(SEATS, **kw)


def test_evaluation_is_deterministic(cuda):
    a, b = _run(), _run()
    for k in TABLES:
        assert a[k] == b[k], k
    sa, sb = a["final_state"], b["final_state"]
    for k in STATE:
        assert torch.equal(getattr(sa, k), getattr(sb, k)), k
    assert a["turns"] == 40 and bool((sa.pins >= 0).any())
    # the defaults spelled out are the defaults
    c = _run(guided=dict(epsilon=0.125, weights=dict(advance=1, setback=1, goal=20, out=15, hit=10, win=1000)))
    for k in STATE:
        assert torch.equal(getattr(sa, k), getattr(c["final_state"], k)), k


def test_other_guided_parameters_play_another_game(cuda):
    """160 turns with playouts of at most 100 turns: long enough for playouts to decide and so for the playout policy
    to reach the action (in the opening no short playout decides, every candidate has 0 wins and the first one is
    played whatever the policy)."""
    kw = dict(max_turns=160, rollout_steps=100)
    sa = _run(**kw)["final_state"]
    for other in (dict(epsilon=1.0), dict(weights=dict(advance=-5, goal=-20, out=-15))):
        sd = _run(guided=other, **kw)["final_state"]
        assert any(not torch.equal(getattr(sa, k), getattr(sd, k)) for k in STATE), other


def test_epsilon_one_seat_plays_the_rollout_seats_game(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    a = _run(guided=dict(epsilon=1.0))
    b = EV.evaluate_agent_parallel_dog(["rollout_agent", "random_agent"] * 2, batch_size=4, seed=3, max_turns=40,
                                       rollouts=2, rollout_steps=24)
    for k in STATE:
        assert torch.equal(getattr(a["final_state"], k), getattr(b["final_state"], k)), k


def test_the_seat_is_dogs_alone(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    with pytest.raises(ValueError, match="'mcts_agent'"):
        EV.evaluate_agent_parallel(SEATS, batch_size=1, num_simulations=2, max_depth=2, max_turns=2)
    with pytest.raises(ValueError, match="'stochastic_mcts_agent'"):
        EV.evaluate_agent_parallel_classic(SEATS, batch_size=1, num_simulations=2, max_depth=2, max_turns=2)
    with pytest.raises(ValueError, match="'epsilon' and 'weights'"):
        _run(guided=dict(temperature=0.25))
    with pytest.raises(ValueError, match="no temperature"):
        _run(guided=dict(weights=dict(temperature=0.25)))


def test_guided_rollout_agent_beats_random(cuda):
    from exploring_muzero_on_dog_amd import evaluate as EV
    t0 = time.perf_counter()
    r = EV.evaluate_agent_parallel_dog(SEATS, batch_size=GAMES // 4, seed=42, rollouts=ROLLOUTS,
                                       rollout_steps=ROLLOUT_STEPS)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    wins, need = r["wins_per_player"][0], binomial_bar(GAMES)
    print(f"guided_rollout_agent (seats 0 + 2) vs random, teams: {wins} of {GAMES} wins ({100.0 * wins / GAMES:.1f} %), "
          f"{r['finished']} finished in {r['turns']} turns, bar {need}, rollouts {ROLLOUTS}, rollout_steps "
          f"{ROLLOUT_STEPS}, {dt:.1f} s")
    assert need == 45
    assert r["wins_per_player"][0] == r["wins_per_player"][2]          # a team wins together
    assert wins >= need
