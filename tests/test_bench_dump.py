"""bench.py --dump-outputs on the CPU: dump_selfplay_outputs on record buffers of the engines' layout writes float32
.npy files -- idx of every game, a fixed sample of the games for the other fields, rows past a game's idx as the
reference initialises them -- and the same call writes the same files."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _buffers(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    return {"obs": torch.randint(0, 5, (n, T, 18, 56), dtype=torch.int8, generator=g),
            "act": torch.randint(0, 24, (n, T), dtype=torch.int32, generator=g),
            "val": torch.rand((n, T), generator=g),
            "pol": torch.rand((n, T, 24), generator=g),
            "team": torch.randint(0, 2, (n, T), dtype=torch.int32, generator=g),
            "idx": torch.randint(1, T, (n,), dtype=torch.int32, generator=g)}


def test_dump_selfplay_outputs(tmp_path):
    n, T = 300, 12          # more games than the sample holds
    buf = _buffers(n, T, 0)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_selfplay_outputs(a, buf)
    bench.dump_selfplay_outputs(b, {k: v.clone() for k, v in buf.items()})
    assert sorted(os.listdir(a)) == sorted(f"{k}.npy" for k in buf)
    got = {k: np.load(os.path.join(a, f"{k}.npy")) for k in buf}
    assert all(v.dtype == np.float32 for v in got.values())
    assert all(np.array_equal(got[k], np.load(os.path.join(b, f"{k}.npy"))) for k in buf)
    assert np.array_equal(got["idx"], buf["idx"].numpy().astype(np.float32))
    pick = np.sort(np.random.RandomState(0).permutation(n)[:bench.DUMP_GAMES])
    assert got["act"].shape == (bench.DUMP_GAMES, T) and got["obs"].shape == (bench.DUMP_OBS_GAMES, T, 18, 56)
    for k in ("obs", "act", "val", "pol", "team"):
        for j in range(got[k].shape[0]):
            i = int(buf["idx"][pick[j]])
            assert np.array_equal(got[k][j, :i], buf[k][pick[j], :i].numpy().astype(np.float32)), (k, j)
            assert (got[k][j, i:] == (-1 if k == "team" else 0)).all(), (k, j)


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    args = bench.parse()
    assert not args.full and args.dump_outputs is None and args.steps == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"


def test_dump_fewer_games_than_the_sample(tmp_path):
    buf = _buffers(5, 7, 1)
    bench.dump_selfplay_outputs(str(tmp_path), buf)
    assert np.load(tmp_path / "act.npy").shape == (5, 7) and np.load(tmp_path / "obs.npy").shape == (5, 7, 18, 56)
