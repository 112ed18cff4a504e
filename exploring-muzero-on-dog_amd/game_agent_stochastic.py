"""Batched Stochastic-MuZero self-play for classic MADN on the GPU (host mirror of
MuZero_Classic_MADN/game_agent_stochastic.py).

``StochasticSelfPlayEngine.play`` = ``play_n_games_v3`` (234-257) + ``play_batch_of_games_jitted``
(52-218): the whole loop runs natively (muz_classic_selfplay).  Buffers: the det keys with
``pol`` [n, T, 4], plus ``dice`` [n, T] and ``dice_dist`` [n, T, 6]; ``obs`` is int8.
"""
from __future__ import annotations

import torch

from . import classic as E
from . import lib as _L
from . import stochastic as ST
from .nets import rng_key_to_seed
from .records import REFERENCE_DTYPES, NativeSelfPlay, as_traj, as_traj_chance, cached, reference_buffers

# MuZero_Classic_MADN/game_agent_stochastic.py:13-24
RULES = dict(E.SELFPLAY_RULES)


class StochasticSelfPlayEngine(NativeSelfPlay):
    def __init__(self, net: ST.DeviceClassicNet, num_envs: int, num_players: int = 4, max_steps: int = 550,
                 num_simulations: int = 50, max_depth: int = 25, rules: dict | None = None, starting_player=0,
                 device="cuda"):
        self.net = net
        self.n, self.P, self.T = int(num_envs), int(num_players), int(max_steps)
        self.S, self.D = int(num_simulations), int(max_depth)
        self.C = E.num_channels(self.P)
        if net.C != self.C:
            raise ValueError(f"network expects {net.C} observation channels, {self.P} players give {self.C}")
        self.rules = E.make_rules(self.P, starting_player=starting_player, **dict(RULES if rules is None else rules))
        self.state = E.ClassicMADNState.alloc(self.n, self.P, self.rules, device)
        nbytes = _L.load().muz_classic_selfplay_workspace_bytes(self.n, self.C, ST.make_cfg(self.S, self.D))
        self._alloc(ST.A_CLASSIC, nbytes, device, chance=ST.CHANCE)

    def _cfg(self, seed, temperature, dirichlet_fraction):
        return ST.make_cfg(self.S, self.D, temperature=temperature, seed=seed, dirichlet_fraction=dirichlet_fraction)

    def play(self, seed: int, temperature: float = 1.0, dirichlet_fraction: float = 0.25, stream=None,
             timing: bool = True) -> dict:
        self._call("muz_classic_selfplay", self._cfg(seed, temperature, dirichlet_fraction), self.traj(),
                   as_traj_chance(self.buffers), (self.n,), stream, timing)
        return self.buffers

    def play_stream(self, num_games: int, seed: int, temperature: float = 1.0, dirichlet_fraction: float = 0.25,
                    stream=None, timing: bool = True) -> dict:
        """``num_games`` games through this engine's lanes (muz_classic_selfplay_stream); game k's record
        equals game k of ``play`` on a batch of ``num_games``."""
        buf = self._stream_buffers(int(num_games))
        self._call("muz_classic_selfplay_stream", self._cfg(seed, temperature, dirichlet_fraction),
                   as_traj(buf, self.T), as_traj_chance(buf), (int(num_games), self.n), stream, timing)
        return buf


_ENGINE_CACHE = {}


def play_n_games_v3(params, rng_key, input_shape, num_envs, num_simulation, max_depth, max_steps, temp,
                    obs_dtype=torch.float32) -> dict:
    """play_n_games_v3 (MuZero_Classic_MADN/game_agent_stochastic.py:220-244), reference signature: Flax
    params dict (or flat dict / DeviceClassicNet), int / uint32[2] key (the engine's counter RNG), input_shape
    (2P + 3, 56).  Returns the reference's buffers (obs fp32 unless ``obs_dtype``; dice int32, dice_dist fp32)
    as device tensors.  The reference's reset seeds only feed jax's unused random start."""
    C = int(input_shape[0])
    if (C - 3) % 2 or int(input_shape[-1]) != E.CELLS:
        raise ValueError(f"input_shape {tuple(input_shape)} is not (2P + 3, 56)")
    net = ST.as_device_classic_net(params, C)
    key = (id(net), int(num_envs), (C - 3) // 2, int(max_steps), int(num_simulation), int(max_depth))
    eng = cached(_ENGINE_CACHE, key, net, lambda: StochasticSelfPlayEngine(
        net, num_envs, num_players=(C - 3) // 2, max_steps=max_steps, num_simulations=num_simulation,
        max_depth=max_depth))
    buf = eng.play(rng_key_to_seed(rng_key), temp)
    dt = dict(REFERENCE_DTYPES, obs=obs_dtype, dice=torch.int32, dice_dist=torch.float32)
    return reference_buffers(buf, dt)
