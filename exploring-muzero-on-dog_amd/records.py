"""The self-play record buffers, defined once: the reference's buffer dict (MuZero_det_MADN/game_agent.py:158-169,
MuZero_Classic_MADN/game_agent_stochastic.py:191-204) as device tensors, its view as the C ABI's muz_traj /
muz_traj_chance, and what the det, classic and DOG engines share around them (game_agent.py, game_agent_stochastic.py,
game_agent_dog.py; replay.py and transfer.py take the same dicts).  A new record field or a dtype change is made here.
"""
from __future__ import annotations

import ctypes

import torch

from . import lib as _L

CELLS = 56
# the fields of muz_traj, in its order
RECORD_KEYS = ("obs", "act", "rew", "val", "pol", "mask", "player", "team", "discount", "idx")
# the dtypes the reference's play_n_games_v3 returns (the engines store obs as int8: its values are 0..4)
REFERENCE_DTYPES = {"obs": torch.float32, "act": torch.int32, "rew": torch.int32, "val": torch.float32,
                    "pol": torch.float32, "mask": torch.float32, "player": torch.int32, "team": torch.int32,
                    "discount": torch.int32, "idx": torch.int32}


def alloc_records(games: int, T: int, C: int, A: int, device, chance: int | None = None) -> dict:
    """Uninitialised records of ``games`` games of at most ``T`` steps: C observation channels, A actions and, with
    ``chance`` outcomes per step (classic MADN: 6), the die and the next state's dice distribution."""
    n, T = int(games), int(T)
    spec = [("obs", torch.int8, (T, C, CELLS)), ("act", torch.int32, (T,)), ("rew", torch.int32, (T,)),
            ("val", torch.float32, (T,)), ("pol", torch.float32, (T, A)), ("mask", torch.float32, (T,))]
    if chance:
        spec += [("dice", torch.int32, (T,)), ("dice_dist", torch.float32, (T, chance))]
    spec += [("player", torch.int32, (T,)), ("team", torch.int32, (T,)), ("discount", torch.int32, (T,)),
             ("idx", torch.int32, ())]
    return {k: torch.empty((n,) + shape, dtype=dt, device=device) for k, dt, shape in spec}


def _address(t: torch.Tensor) -> int:
    return t.data_ptr() if t.numel() else 0


def as_traj(buf: dict, T: int = 0) -> _L.MuzTraj:
    """``buf`` as muz_traj with ``max_steps`` = T (0: packed rows, transfer.pack); a missing field is a KeyError."""
    t = _L.MuzTraj()
    for k in RECORD_KEYS:
        setattr(t, k, _address(buf[k]))
    t.max_steps = int(T)
    return t


def as_traj_chance(buf: dict) -> _L.MuzTrajChance:
    ch = _L.MuzTrajChance()
    ch.dice, ch.dice_dist = _address(buf["dice"]), _address(buf["dice_dist"])
    return ch


def stats_dict(st: _L.MuzSpStats, timing: bool) -> dict | None:
    """An engine's ``last_stats`` after a call that was (or was not) given ``st`` to fill."""
    if not timing:
        return None
    return {"turns": st.turns, "searches": st.searches, "search_ms": st.search_ms, "total_ms": st.total_ms}


def reference_buffers(buf: dict, dtypes: dict) -> dict:
    """Fresh copies of the engine's (reused) record buffers in the reference dtypes, with every row at or past a
    game's ``idx`` as the reference's initial buffers hold it: zeros, ``team`` -1 (game_agent.py:158-169,
    game_agent_stochastic.py:191-204).  The native loops write only rows below ``idx``."""
    idx = buf["idx"].long()
    past = torch.arange(buf["act"].shape[1], device=idx.device)[None, :] >= idx[:, None]
    out = {}
    for k, v in buf.items():
        x = v.to(dtypes[k], copy=True)
        if k != "idx":
            x.masked_fill_(past.view(past.shape + (1,) * (x.dim() - 2)), -1 if k == "team" else 0)
        out[k] = x
    return out


def cached(cache: dict, key, net, make):
    """The one live engine of a play_n_games_v3: ``cache``'s entry when it is for ``key`` and the same weight set
    (``hit.net is net``), else the cache is emptied and ``make()`` builds the engine.  A test_training-style loop calls
    play_n_games_v3 once per iteration, and a fresh engine would reallocate its state, workspace and [num_envs,
    max_steps] buffers (GBs at config (e)) every time."""
    hit = cache.get(key)
    if hit is None or hit.net is not net:
        cache.clear()
        hit = cache[key] = make()
    return hit


class NativeSelfPlay:
    """What the det and the classic engine share: the record buffers of a batch (``buffers``) and of a stream of
    ``num_games`` games, the workspace, and the call into the native driver with its stats bookkeeping.  A subclass
    sets n, P, T, S, D, C, net, rules and state before ``_alloc``."""

    def _alloc(self, A: int, workspace_bytes: int, device, chance: int | None = None):
        self.buffers = alloc_records(self.n, self.T, self.C, A, device, chance)
        self.workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=device)
        self._sbuf, self._sbuf_n = None, None
        self.last_turns = 0
        self.last_stats = None

    def traj(self) -> _L.MuzTraj:
        return as_traj(self.buffers, self.T)

    def _stream_buffers(self, num_games: int) -> dict:
        """Buffers shaped [num_games, max_steps, ...], reused across calls of the same size."""
        if self._sbuf_n != num_games:
            self._sbuf = {k: torch.empty((num_games,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
                          for k, v in self.buffers.items()}
            self._sbuf_n = num_games
        return self._sbuf

    def _call(self, name: str, cfg, traj, chance, games: tuple, stream, timing: bool):
        """Entry point ``name`` on this engine's state and workspace; ``games``: (n,) or (num_games, lanes).  The
        native loop synchronises its stream before returning."""
        st = _L.MuzSpStats()
        records = (traj,) if chance is None else (traj, chance)
        _L.check(getattr(_L.load(), name)(self.rules, self.net.w, ctypes.byref(cfg), self.state.soa(), *records, *games,
                                          _L.ptr(self.workspace), _L.nbytes(self.workspace),
                                          ctypes.byref(st) if timing else None, _L.stream_ptr(stream)), name)
        self.last_stats = stats_dict(st, timing)
        self.last_turns = st.turns if timing else -1
