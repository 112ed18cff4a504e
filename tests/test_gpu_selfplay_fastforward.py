"""The det streaming driver's fast-forward (csrc/selfplay.hip, k_sp_head<STREAM>): a game without a legal move plays
its no_step turn inside the turn head instead of sitting out a launched turn.  Records are keyed by game number
and the game's own step count, so every buffer must stay bit for bit what the batch driver (one reference turn per
launch, no fast-forward) writes.

Where no-move turns fall (looked up before fixing the shapes):
 * oracle/detmadn.py under uniformly random legal play, SELFPLAY_RULES: 2 players, 30 games to the end (100-153
   steps): 15 no-move turns, none before step 50, no run longer than 1.  4 players, 20 games (273-573 steps): 93
   no-move turns, the first after step 50, 3 runs of two consecutive ones (teams: a finished player's partner
   substitutes), none longer.
 * the searched play of these tests (init_muzero_params(3), S = 4, D = 3, seed 99), from a batch's own records:
   2 players, 256 games (97-178 steps): 233 no-move turns, 40 of them in steps 20-39, 7 runs of two, none longer;
   4 players, 128 games (243-563 steps): 1016 no-move turns, 31 runs of two, none longer.  So two consecutive
   no-move turns occur under both rule sets, and a run never reaches the cap of 4.
   The first 48 2-player games cut at T = 92 hold 35 live no-move turns, 3 games whose turn T - 1 is one, and a
   run of two; the first 40 4-player games cut at T = 94 hold 50, 4 and a run of two.  Of the first 40 games
   played to the end, the longest has 141 turns of which 139 search (2 players), 493 of which 480 search (4
   players) -- so the turn counts with and without fast-forward differ.  Game 1 of the 4-player games cut at
   T = 94 is one of those that fill on a no-move turn (the single-lane case).
Each case re-derives its coverage from the batch's records and fails, not skips, if it is gone.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, D, SEED = 4, 3, 99
CAP = 4   # kSpFfCap (csrc/selfplay.hip)


def _mods():
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import game_agent as GA
    from exploring_muzero_on_dog_amd import nets as N
    return E, GA, N


_NETS, _BATCH = {}, {}


def _net(P):
    E, GA, N = _mods()
    if P not in _NETS:
        C = E.num_channels(P)
        _NETS[P] = N.DeviceNet(N.init_muzero_params(3, C), C)
    return _NETS[P]


def _batch(P, games, T):
    """The reference: one batch of `games` games (computed once per shape, never modified)."""
    key = (P, games, T)
    if key not in _BATCH:
        _, GA, _ = _mods()
        eng = GA.SelfPlayEngine(_net(P), games, num_players=P, max_steps=T, num_simulations=S, max_depth=D)
        buf = {k: v.clone() for k, v in eng.play(SEED, 1.0).items()}
        _BATCH[key] = (buf, dict(eng.last_stats))
    return _BATCH[key]


def _stream(P, games, lanes, T):
    _, GA, _ = _mods()
    eng = GA.SelfPlayEngine(_net(P), lanes, num_players=P, max_steps=T, num_simulations=S, max_depth=D)
    got = eng.play_stream(games, SEED, 1.0)
    return got, dict(eng.last_stats)


def _coverage(buf, T):
    """From the records: live no-move turns, the longest run of consecutive ones per game, games whose last
    recorded turn is a no-move turn at idx == T, searched turns per game."""
    idx = buf["idx"].cpu().numpy()
    mask = buf["mask"].cpu().numpy()
    live = np.arange(T)[None, :] < idx[:, None]
    nm = live & (mask == 0)
    longest = np.zeros(len(idx), int)
    for g in range(len(idx)):
        r = 0
        for t in range(int(idx[g])):
            r = r + 1 if nm[g, t] else 0
            longest[g] = max(longest[g], r)
    full_nomove = int(((idx == T) & nm[:, T - 1]).sum())
    searched = (live & (mask == 1)).sum(1)
    return dict(idx=idx, no_move=int(nm.sum()), longest=longest, full_nomove=full_nomove, searched=searched)


def _assert_equal(got, want):
    for k in want:
        assert torch.equal(got[k], want[k]), k


# P, games, lanes, T, two consecutive no-move turns expected
CASES = [(2, 48, 16, 92, True), (4, 40, 8, 94, True)]


@pytest.mark.parametrize("P,games,lanes,T,runs2", CASES)
def test_records_unchanged(cuda, P, games, lanes, T, runs2):
    """play_stream (fast-forward) == play (none) in every buffer, on games with enough no-move turns."""
    want, bst = _batch(P, games, T)
    cov = _coverage(want, T)
    print(f"P={P}: {cov['no_move']} live no-move turns, longest run {cov['longest'].max()}, "
          f"{cov['full_nomove']} games end on a no-move turn at idx == T")
    if cov["no_move"] < 20:
        pytest.fail(f"coverage: only {cov['no_move']} live no-move turns")
    if cov["full_nomove"] < 1:
        pytest.fail("coverage: no game whose last recorded turn is a no-move turn at idx == T")
    if runs2 and cov["longest"].max() < 2:
        pytest.fail("coverage: no game with two consecutive no-move turns")
    got, st = _stream(P, games, lanes, T)
    _assert_equal(got, want)
    assert st["searches"] == bst["searches"] == int(cov["searched"].sum())


@pytest.mark.parametrize("P,n,T", [(2, 40, 200), (4, 40, 500)])
def test_every_lane_turn_searches(cuda, monkeypatch, P, n, T):
    """num_games == lanes, nothing refilled: with fast-forward a game is launched once per searched turn, without
    it once per recorded turn."""
    want, bst = _batch(P, n, T)
    cov = _coverage(want, T)
    print(f"P={P}: longest game {cov['idx'].max()} turns, most searched turns {cov['searched'].max()}, "
          f"longest no-move run {cov['longest'].max()}")
    assert cov["longest"].max() < CAP, "a run of no-move turns as long as the cap: turns would count its rest"
    if cov["searched"].max() >= cov["idx"].max():
        pytest.fail("coverage: the longest game has no no-move turn, both drivers would launch the same turns")
    got, st = _stream(P, n, n, T)
    _assert_equal(got, want)
    assert st["turns"] == cov["searched"].max()
    assert st["searches"] == int(cov["searched"].sum())
    monkeypatch.setenv("MUZ_SP_FASTFORWARD", "0")   # (read by every call of the driver)
    got, st = _stream(P, n, n, T)
    _assert_equal(got, want)
    assert st["turns"] == cov["idx"].max() == bst["turns"]
    assert st["searches"] == int(cov["searched"].sum())


@pytest.mark.parametrize("P,games,lanes,T,runs2", CASES)
def test_cap_path(cuda, monkeypatch, P, games, lanes, T, runs2):
    """MUZ_SP_FASTFORWARD=1: one no-move turn per game and launch, so the second turn of a run of two meets the
    cap, keeps flag 2 and is applied by the next head.  Same records."""
    want, bst = _batch(P, games, T)
    cov = _coverage(want, T)
    if cov["longest"].max() < 2:
        pytest.fail("coverage: no run of no-move turns longer than the cap of 1")
    monkeypatch.setenv("MUZ_SP_FASTFORWARD", "1")
    got, st = _stream(P, games, lanes, T)
    _assert_equal(got, want)
    assert st["searches"] == bst["searches"]


def test_single_lane_record_fills_in_fast_forward(cuda):
    """One lane: when the only active game fills its record inside the fast-forward (a no-move turn at step T - 1)
    the turn has no game to search, yet the driver must go on to the games that are left."""
    P, games, T = 4, 4, 94
    want, bst = _batch(P, games, T)
    idx = want["idx"].cpu().numpy()
    mask = want["mask"].cpu().numpy()
    if not ((idx[:-1] == T) & (mask[:-1, T - 1] == 0)).any():
        pytest.fail("coverage: no game before the last whose record fills on a no-move turn")
    got, st = _stream(P, games, 1, T)
    _assert_equal(got, want)
    assert st["searches"] == bst["searches"]
