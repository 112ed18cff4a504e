"""Batched MuZero self-play on the GPU (host mirror of MuZero_det_MADN/game_agent.py).

``play_n_games_v3`` keeps the reference signature's meaning (game_agent.py:185-192): reset
``num_envs`` games, play them to completion (or ``max_steps`` batched turns) with a Gumbel-MuZero
search per move (``policy="puct"``: the reference's commented mctx.muzero_policy call instead), and return the trajectory buffers as a dict of device tensors
(obs, act, rew, val, pol, mask, player, team, discount, idx) shaped [num_envs, max_steps, ...].
The whole loop runs natively in libmuz.so (muz_detmadn_selfplay): no per-turn Python, no
host<->device copy inside a turn.  ``obs`` is int8 (values 0..4); the reference stores fp32.
"""
from __future__ import annotations

import torch

from . import detmadn as E
from . import lib as _L
from . import mcts as M
from . import nets as N
from .records import REFERENCE_DTYPES, NativeSelfPlay, as_traj, cached, reference_buffers  # noqa: F401 (re-exported)

# MuZero_det_MADN/game_agent.py:12-22
RULES = dict(E.SELFPLAY_RULES)
POLICIES = ("gumbel", "puct")
PUCT_KWARGS = ("qtransform", "min_value", "max_value", "dirichlet_fraction", "dirichlet_alpha", "pb_c_init", "pb_c_base")


def check_policy(policy, policy_kwargs) -> dict:
    """The rule of mcts.muzero_mcts: an unknown policy is a ValueError, PUCT keywords on the Gumbel path (or unknown
    ones on the PUCT path) a TypeError.  -> the keywords as a dict."""
    kw = dict(policy_kwargs or {})
    if policy not in POLICIES:
        raise ValueError(f"unknown policy {policy!r} ('gumbel' or 'puct')")
    if policy == "gumbel" and kw:
        raise TypeError(f"policy='gumbel' takes no {sorted(kw)}")
    if set(kw) - set(PUCT_KWARGS):
        raise TypeError(f"policy='puct' takes no {sorted(set(kw) - set(PUCT_KWARGS))}")
    return kw


class SelfPlayEngine(NativeSelfPlay):
    """Owns the device state, trajectory buffers and workspace for repeated self-play calls."""

    def __init__(self, net: N.DeviceNet, num_envs: int, num_players: int = 4, max_steps: int = 550,
                 num_simulations: int = 50, max_depth: int = 25, rules: dict | None = None, starting_player=0,
                 device="cuda", policy: str = "gumbel", policy_kwargs: dict | None = None):
        """``policy="puct"`` plays with mctx.muzero_policy (mcts.muzero_policy; ``policy_kwargs``: qtransform,
        min_value, max_value, dirichlet_fraction, dirichlet_alpha, pb_c_init, pb_c_base); the records' ``pol`` are then
        the root visit fractions.  The workspace is the same for both policies."""
        self.policy, self.policy_kwargs = policy, check_policy(policy, policy_kwargs)   # (before any allocation)
        self.net = net
        self.n, self.P, self.T = int(num_envs), int(num_players), int(max_steps)
        self.S, self.D = int(num_simulations), int(max_depth)
        self.C = E.num_channels(self.P)
        if net.C != self.C:
            raise ValueError(f"network expects {net.C} observation channels, {self.P} players give {self.C}")
        r = dict(RULES if rules is None else rules)
        self.rules = E.make_rules(self.P, starting_player=starting_player, **r)
        self.state = E.DetMADNState.alloc(self.n, self.P, self.rules, device)
        self._alloc(net.A, _L.load().muz_selfplay_workspace_bytes(self.n, self.C, M.make_cfg(self.S, self.D)), device)

    def _search(self, seed, temperature):
        """-> (the call's search configuration, the batch entry point's name, the streaming one's)."""
        if self.policy == "puct":
            return (M.make_puct_cfg(self.S, self.D, temperature, seed=seed, **self.policy_kwargs),
                    "muz_detmadn_selfplay_puct", "muz_detmadn_selfplay_puct_stream")
        return (M.make_cfg(self.S, self.D, temperature=temperature, seed=seed), "muz_detmadn_selfplay",
                "muz_detmadn_selfplay_stream")

    def play(self, seed: int, temperature: float = 1.0, stream=None, timing: bool = True) -> dict:
        """One play_n_games_v3 call.  The native loop synchronises its stream before returning.
        With ``timing`` the search launches are bracketed by HIP events (see ``last_stats``)."""
        cfg, name, _ = self._search(seed, temperature)
        self._call(name, cfg, self.traj(), None, (self.n,), stream, timing)
        return self.buffers

    def play_stream(self, num_games: int, seed: int, temperature: float = 1.0, stream=None,
                    timing: bool = True) -> dict:
        """``num_games`` games through this engine's ``num_envs`` lanes (muz_detmadn_selfplay_stream): a
        lane whose game ends starts the next one, so every search runs on a full batch until the last
        games.  Game k's trajectory equals game k of ``play`` on a batch of ``num_games``.  Returns
        buffers shaped [num_games, max_steps, ...] (reused across calls of the same size)."""
        buf = self._stream_buffers(int(num_games))
        cfg, _, name = self._search(seed, temperature)
        self._call(name, cfg, as_traj(buf, self.T), None, (int(num_games), self.n), stream, timing)
        return buf


_ENGINE_CACHE = {}


def cached_engine(net: N.DeviceNet, num_envs, num_players, max_steps, num_simulation, max_depth, rules,
                  policy="gumbel", policy_kwargs=None) -> SelfPlayEngine:
    """The engine of the last reference-signature call, reused when the call's shape, rules, search policy (and its
    keywords) and weight set are the same (records.cached)."""
    kw = check_policy(policy, policy_kwargs)
    key = (id(net), int(num_envs), int(num_players), int(max_steps), int(num_simulation), int(max_depth),
           tuple(sorted((dict(RULES if rules is None else rules)).items())), policy, tuple(sorted(kw.items())))
    return cached(_ENGINE_CACHE, key, net, lambda: SelfPlayEngine(net, num_envs, num_players, max_steps, num_simulation,
                                                                  max_depth, rules, policy=policy, policy_kwargs=kw))


def play_n_games_v3(params, rng_key, input_shape, num_envs, num_simulation, max_depth, max_steps, temp,
                    rules: dict | None = None, obs_dtype=torch.float32, policy="gumbel", policy_kwargs=None) -> dict:
    """play_n_games_v3 (MuZero_det_MADN/game_agent.py:185-192), reference signature.

    ``params``: init_muzero_params' nested Flax dict (or a flat dict / DeviceNet, nets.as_device_net);
    ``rng_key``: int or uint32[2] key (nets.rng_key_to_seed; the engine's counter RNG, not threefry);
    ``input_shape``: (C, 56) with C = 8P + 2, which fixes the player count (the reference's game_agent
    plays P = 4, C = 34).  Returns the reference's buffer dict (game_agent.py:158-169): obs fp32
    [num_envs, max_steps, C, 56] (``obs_dtype=torch.int8`` keeps the engine's exact int8 copy), act / rew /
    player / team / discount int32, val / mask fp32, pol fp32 [.., 24], idx int32 -- fresh device tensors, rows past
    ``idx`` zero (``team`` -1) as the reference initialises them.

    ``policy="puct"`` (with ``policy_kwargs``, see SelfPlayEngine) plays what the reference plays once run_muzero_mcts'
    commented mctx.muzero_policy call (muzero_deterministic_madn.py:685-697) is the live one: ``pol`` holds the root
    visit fractions."""
    check_policy(policy, policy_kwargs)
    C = int(input_shape[0])
    if (C - 2) % 8 or int(input_shape[-1]) != E.CELLS:
        raise ValueError(f"input_shape {tuple(input_shape)} is not (8P + 2, 56)")
    net = N.as_device_net(params, C)
    eng = cached_engine(net, num_envs, (C - 2) // 8, max_steps, num_simulation, max_depth, rules, policy, policy_kwargs)
    buf = eng.play(N.rng_key_to_seed(rng_key), temp)
    return reference_buffers(buf, dict(REFERENCE_DTYPES, obs=obs_dtype))
