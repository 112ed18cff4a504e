"""The four-seat evaluation loop with scripted seats only, against tables recorded before det, classic and DOG shared
one loop (tests/golden/evaluate_scripted_seats.json, written by profiles/evaluate_refactor.py).  No network runs, so
the games depend on the environment kernels, the agents' kernels and the counter RNG alone: the tables are exact."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "evaluate_scripted_seats.json")) as f:
    GOLDEN = json.load(f)
RULE_VS_RANDOM = ["rule_based_agent", "random_agent"] * 2
CALLS = {"det_scripted": ("evaluate_agent_parallel", RULE_VS_RANDOM, 7),
         "classic_scripted": ("evaluate_agent_parallel_classic", RULE_VS_RANDOM, 7),
         "dog_scripted": ("evaluate_agent_parallel_dog", ["random_agent"] * 4, 3)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_scripted_seats_play_the_recorded_games(cuda, name):
    from exploring_muzero_on_dog_amd import evaluate as EV
    fn, seats, seed = CALLS[name]
    r = getattr(EV, fn)(seats, batch_size=4, seed=seed)
    want = GOLDEN[name]
    assert set(want) == {"winners", "average_progress", "finished"} | ({"turns"} if name == "dog_scripted" else set())
    assert {k: r[k] for k in want} == want
    assert r["games"] == 16 and r["final_state"].batch == 16
