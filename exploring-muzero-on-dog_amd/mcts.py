"""MuZero search on the GPU: run_muzero_mcts (MuZero_det_MADN/muzero_deterministic_madn.py:663-704).

The whole ``mctx.gumbel_muzero_policy`` call (S simulations of select / expand / backup) is one
persistent HIP kernel (csrc/search.hip); the root inference runs first (csrc/nets.hip).  The reference's
second policy, the ``mctx.muzero_policy`` call it keeps commented (685-697: PUCT, Dirichlet root noise,
visit-count weights), is ``muzero_policy`` here: another persistent kernel (csrc/puct_search.hip) on the same
workspace, chosen with ``policy="puct"``.  ``env_muzero_policy`` is the reference's network-free agent
(MADN/deterministic_madn.py:481-589): the same ``muzero_policy`` with the det-MADN environment as its model and random
rollouts as leaf values (csrc/env_mcts.hip), on a workspace of its own; ``env_gumbel_muzero_policy`` is the same agent
under ``gumbel_muzero_policy`` (csrc/env_gumbel.hip), the call the reference drives
(MADN/simulate_deterministicMADN.py:12-35), on that workspace.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import lib as _L
from . import nets as _N


@dataclass
class PolicyOutput:
    """mctx.PolicyOutput without the tree object (the tree stays in the device workspace)."""
    action: torch.Tensor          # int32 [B]
    action_weights: torch.Tensor  # fp32 [B, A]


class SearchWorkspace:
    """Device workspace for B searches: tree arrays + node embeddings (+ root-inference scratch)."""

    def __init__(self, batch: int, num_simulations: int, device="cuda"):
        lib = _L.load()
        cfg = make_cfg(num_simulations, 1)
        self.batch, self.S = batch, num_simulations
        nbytes = lib.muz_search_workspace_bytes(batch, cfg)
        self.tree = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        self.scratch = torch.empty(lib.muz_nets_root_scratch_bytes(batch) // 4, dtype=torch.float32, device=device)

    def fits(self, batch, S):
        return batch <= self.batch and S <= self.S


def make_cfg(num_simulations, max_depth, temperature=1.0, max_num_considered=16, value_scale=0.5,
             maxvisit_init=50.0, seed=0, turn=0):
    c = _L.MuzSearchCfg()
    c.num_simulations = int(num_simulations)
    c.max_depth = int(max_depth)
    c.max_num_considered = int(max_num_considered)
    c.value_scale = float(value_scale)
    c.maxvisit_init = float(maxvisit_init)
    c.gumbel_scale = float(temperature)
    c.seed = int(seed) & ((1 << 64) - 1)
    c.turn = int(turn)
    return c


def gumbel_muzero_policy(net: _N.DeviceNet, root_logits, root_value, root_embedding, legal_bits,
                         num_simulations, max_depth, temperature=1.0, gumbel=None, seed=0, turn=0,
                         game_id=None, workspace: SearchWorkspace | None = None):
    """mctx.gumbel_muzero_policy with qtransform_completed_by_mix_value(value_scale=0.5),
    max_num_considered_actions=16, gumbel_scale=temperature.  ``gumbel`` = explicit (already scaled)
    noise [B, A] or None to draw it on device from (seed, game_id, turn).
    Returns (PolicyOutput, root_value = search_tree.summary().value)."""
    lib = _L.load()
    B = root_logits.shape[0]
    dev = root_logits.device
    if workspace is None or not workspace.fits(B, num_simulations):
        workspace = SearchWorkspace(B, num_simulations, dev)
    cfg = make_cfg(num_simulations, max_depth, temperature, seed=seed, turn=turn)
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    weights = torch.empty((B, net.A), dtype=torch.float32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    g = None if gumbel is None else gumbel.to(device=dev, dtype=torch.float32).contiguous()
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).contiguous()
    lb = legal_bits.to(device=dev, dtype=torch.int32).contiguous()
    _L.check(lib.muz_gumbel_search(net.w, cfg, _L.ptr(root_logits.contiguous()), _L.ptr(root_value.contiguous()),
                                   _L.ptr(root_embedding.contiguous()), _L.ptr(lb), _L.ptr(g), _L.ptr(gid), B,
                                   _L.ptr(workspace.tree), _L.nbytes(workspace.tree), _L.ptr(action), _L.ptr(weights),
                                   _L.ptr(value),
                                   _L.stream_ptr()), "muz_gumbel_search")
    return PolicyOutput(action, weights), value


QTRANSFORMS = {"min_max": _L.MUZ_QT_MIN_MAX, "parent_and_siblings": _L.MUZ_QT_PARENT_SIBLINGS}


def make_puct_cfg(num_simulations, max_depth, temperature=1.0, qtransform="min_max", min_value=-1.0, max_value=1.0,
                  dirichlet_fraction=0.25, dirichlet_alpha=0.3, pb_c_init=1.25, pb_c_base=19652.0, seed=0, turn=0):
    """muz_puct_cfg with the constants of the reference's commented mctx.muzero_policy call (685-697) and mctx's
    defaults for what that call leaves out (pb_c_init, pb_c_base)."""
    if qtransform not in QTRANSFORMS:
        raise ValueError(f"unknown qtransform {qtransform!r} (one of {sorted(QTRANSFORMS)})")
    c = _L.MuzPuctCfg()
    c.num_simulations = int(num_simulations)
    c.max_depth = int(max_depth)
    c.qtransform = QTRANSFORMS[qtransform]
    c.min_value = float(min_value)
    c.max_value = float(max_value)
    c.dirichlet_fraction = float(dirichlet_fraction)
    c.dirichlet_alpha = float(dirichlet_alpha)
    c.pb_c_init = float(pb_c_init)
    c.pb_c_base = float(pb_c_base)
    c.temperature = float(temperature)
    c.seed = int(seed) & ((1 << 64) - 1)
    c.turn = int(turn)
    return c


def muzero_policy(net: _N.DeviceNet, root_logits, root_value, root_embedding, legal_bits, num_simulations, max_depth,
                  temperature=1.0, *, qtransform="min_max", min_value=-1.0, max_value=1.0, dirichlet_fraction=0.25,
                  dirichlet_alpha=0.3, pb_c_init=1.25, pb_c_base=19652.0, dirichlet=None, gumbel=None, seed=0, turn=0,
                  game_id=None, workspace: SearchWorkspace | None = None):
    """mctx.muzero_policy as the reference's commented call sets it (muzero_deterministic_madn.py:685-697): PUCT
    selection with qtransform_by_min_max(-1, 1) (``qtransform="parent_and_siblings"``: mctx's default), Dirichlet
    root noise 0.25 / 0.3, visit-count action weights, ``temperature`` on the final draw (0: a most-visited action).
    ``dirichlet`` / ``gumbel`` = explicit root noise / final Gumbel draws [B, A], or None to draw them on device from
    (seed, game_id, turn).  Returns (PolicyOutput, root_value = search_tree.summary().value)."""
    lib = _L.load()
    B = root_logits.shape[0]
    dev = root_logits.device
    if workspace is None or not workspace.fits(B, num_simulations):
        workspace = SearchWorkspace(B, num_simulations, dev)
    cfg = make_puct_cfg(num_simulations, max_depth, temperature, qtransform, min_value, max_value, dirichlet_fraction,
                        dirichlet_alpha, pb_c_init, pb_c_base, seed, turn)
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    weights = torch.empty((B, net.A), dtype=torch.float32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    dn = None if dirichlet is None else dirichlet.to(device=dev, dtype=torch.float32).contiguous()
    g = None if gumbel is None else gumbel.to(device=dev, dtype=torch.float32).contiguous()
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).contiguous()
    lb = legal_bits.to(device=dev, dtype=torch.int32).contiguous()
    _L.check(lib.muz_puct_search(net.w, cfg, _L.ptr(root_logits.contiguous()), _L.ptr(root_value.contiguous()),
                                 _L.ptr(root_embedding.contiguous()), _L.ptr(lb), _L.ptr(dn), _L.ptr(g), _L.ptr(gid), B,
                                 _L.ptr(workspace.tree), _L.nbytes(workspace.tree), _L.ptr(action), _L.ptr(weights),
                                 _L.ptr(value), _L.stream_ptr()), "muz_puct_search")
    return PolicyOutput(action, weights), value


class EnvSearchWorkspace:
    """Device workspace of env_muzero_policy for B searches: the tree's own carve (muz_detmadn_mcts_tree_bytes:
    children arrays and a 64-byte state row per node, no latent slots)."""

    def __init__(self, batch: int, num_simulations: int, device="cuda"):
        cfg = make_puct_cfg(num_simulations, 1)
        self.batch, self.S = batch, num_simulations
        nbytes = _L.load().muz_detmadn_mcts_tree_bytes(batch, cfg)
        if nbytes < 0:
            raise _L.MuzError(f"env_muzero_policy: num_simulations {num_simulations} is outside the kernel's limits")
        self.tree = torch.empty((nbytes,), dtype=torch.uint8, device=device)

    def fits(self, batch, S):
        return batch <= self.batch and S <= self.S

    def rollout_turns(self, batch: int) -> torch.Tensor:
        """int32 [batch]: the rollout turns each game of the last search of ``batch`` games played."""
        return self.tree[:4 * batch].view(torch.int32)


def env_muzero_policy(env, num_simulations, max_depth, temperature=0.0, *, rollout_steps=300, seed, turn,
                      game_id=None, workspace: EnvSearchWorkspace | None = None, summary=False, qtransform="min_max",
                      min_value=-1.0, max_value=1.0, dirichlet_fraction=0.0, dirichlet_alpha=0.3, pb_c_init=1.25,
                      pb_c_base=19652.0, dirichlet=None, gumbel=None):
    """The network-free MCTS agent of the reference (MADN/deterministic_madn.py:481-589 with
    MADN/simulate_deterministicMADN.py:12-35): mctx.muzero_policy whose model is the det-MADN environment itself --
    prior logits 100 legal + 200 winning, random-rollout leaf values of at most ``rollout_steps`` turns -- on the
    states of ``env`` (a detmadn.DetMADNState, read only), one persistent kernel (csrc/env_mcts.hip).  The semantics
    the reference leaves open are fixed in include/muz.h (muz_detmadn_mcts); parity with the reference is unpinned.
    The keywords after ``summary`` are muzero_policy's, with no root noise by default (an evaluation agent).  A game
    that is finished or has no legal action is not searched: action -1, weights 0, value 0.
    Returns (PolicyOutput, root_value), with ``summary`` also search_tree.summary()'s visit_counts (int32 [B, 24]) and
    qvalues (fp32 [B, 24]; unvisited children 0)."""
    from . import detmadn as _E
    if not isinstance(env, _E.DetMADNState):
        raise TypeError("env_muzero_policy searches det-MADN states (detmadn.DetMADNState): no environment-model "
                        f"kernel exists for {type(env).__name__}")
    lib = _L.load()
    B = env.batch
    dev = env.board.device
    cfg = make_puct_cfg(num_simulations, max_depth, temperature, qtransform, min_value, max_value, dirichlet_fraction,
                        dirichlet_alpha, pb_c_init, pb_c_base, seed, turn)
    mcfg = _L.MuzEnvMctsCfg(int(rollout_steps))
    if workspace is None or not workspace.fits(B, num_simulations):
        workspace = EnvSearchWorkspace(B, num_simulations, dev)
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    weights = torch.empty((B, _E.ACTIONS), dtype=torch.float32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    visits = torch.empty((B, _E.ACTIONS), dtype=torch.int32, device=dev) if summary else None
    qvalues = torch.empty((B, _E.ACTIONS), dtype=torch.float32, device=dev) if summary else None
    dn = None if dirichlet is None else dirichlet.to(device=dev, dtype=torch.float32).contiguous()
    g = None if gumbel is None else gumbel.to(device=dev, dtype=torch.float32).contiguous()
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).contiguous()
    _L.check(lib.muz_detmadn_mcts(env.rules, cfg, mcfg, env.soa(), _L.ptr(dn), _L.ptr(g), _L.ptr(gid), B,
                                  _L.ptr(workspace.tree), _L.nbytes(workspace.tree), _L.ptr(action), _L.ptr(weights),
                                  _L.ptr(value), _L.ptr(visits), _L.ptr(qvalues), _L.stream_ptr()), "muz_detmadn_mcts")
    out = (PolicyOutput(action, weights), value)
    return out + (visits, qvalues) if summary else out


GUMBEL_QTRANSFORMS = {"completed_by_mix_value": _L.MUZ_QT_COMPLETED_MIX, "min_max": _L.MUZ_QT_MIN_MAX}


def env_gumbel_muzero_policy(env, num_simulations, max_depth, temperature=0.0, *, rollout_steps=300, seed, turn,
                             game_id=None, workspace: EnvSearchWorkspace | None = None, summary=False,
                             qtransform="completed_by_mix_value", max_num_considered=16, value_scale=0.5,
                             maxvisit_init=50.0, min_value=-1.0, max_value=1.0, gumbel=None):
    """The network-free agent under the Gumbel policy, as the reference drives it (MADN/simulate_deterministicMADN.py:
    12-35 run_gumbel: mctx.gumbel_muzero_policy over root_fn / recurrent_fn of MADN/deterministic_madn.py:481-589):
    env_muzero_policy's model -- the det-MADN environment itself, prior logits 100 legal + 200 winning, random-rollout
    leaf values of at most ``rollout_steps`` turns -- searched as gumbel_muzero_policy searches a network (sequential
    halving at the root, completed Q-values, every node masked), one persistent kernel (csrc/env_gumbel.hip) on the
    states of ``env`` (a detmadn.DetMADNState, read only) and env_muzero_policy's workspace.
    ``qtransform``: "completed_by_mix_value" (gumbel_muzero_policy's here, with ``value_scale`` / ``maxvisit_init``) or
    "min_max" (the reference's call, qtransform_by_min_max(``min_value``, ``max_value``)).  ``temperature`` is the
    Gumbel scale as in gumbel_muzero_policy (0: a deterministic agent); ``gumbel`` = explicit, already scaled noise
    [B, 24], or None to draw it on device from (seed, game_id, turn).  The semantics both parents leave open are fixed
    in include/muz.h (muz_detmadn_gumbel_mcts); parity with the reference is unpinned.  A game that is finished or has
    no legal action is not searched: action -1, weights 0, value 0.
    Returns what env_muzero_policy returns: (PolicyOutput, root_value), with ``summary`` also visit_counts (int32
    [B, 24]) and qvalues (fp32 [B, 24]; unvisited children 0)."""
    from . import detmadn as _E
    if not isinstance(env, _E.DetMADNState):
        raise TypeError("env_gumbel_muzero_policy searches det-MADN states (detmadn.DetMADNState): no "
                        f"environment-model kernel exists for {type(env).__name__}")
    if qtransform not in GUMBEL_QTRANSFORMS:
        raise ValueError(f"unknown qtransform {qtransform!r} (one of {sorted(GUMBEL_QTRANSFORMS)})")
    lib = _L.load()
    B = env.batch
    dev = env.board.device
    cfg = make_cfg(num_simulations, max_depth, temperature, max_num_considered, value_scale, maxvisit_init, seed, turn)
    gcfg = _L.MuzEnvGumbelCfg(int(rollout_steps), GUMBEL_QTRANSFORMS[qtransform], float(min_value), float(max_value))
    if workspace is None or not workspace.fits(B, num_simulations):
        workspace = EnvSearchWorkspace(B, num_simulations, dev)
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    weights = torch.empty((B, _E.ACTIONS), dtype=torch.float32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    visits = torch.empty((B, _E.ACTIONS), dtype=torch.int32, device=dev) if summary else None
    qvalues = torch.empty((B, _E.ACTIONS), dtype=torch.float32, device=dev) if summary else None
    g = None if gumbel is None else gumbel.to(device=dev, dtype=torch.float32).contiguous()
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).contiguous()
    _L.check(lib.muz_detmadn_gumbel_mcts(env.rules, cfg, gcfg, env.soa(), _L.ptr(g), _L.ptr(gid), B,
                                         _L.ptr(workspace.tree), _L.nbytes(workspace.tree), _L.ptr(action),
                                         _L.ptr(weights), _L.ptr(value), _L.ptr(visits), _L.ptr(qvalues),
                                         _L.stream_ptr()), "muz_detmadn_gumbel_mcts")
    out = (PolicyOutput(action, weights), value)
    return out + (visits, qvalues) if summary else out


def muzero_mcts(net: _N.DeviceNet, observations, legal_bits, num_simulations, max_depth, temperature,
                gumbel=None, seed=0, turn=0, workspace: SearchWorkspace | None = None, *, policy="gumbel",
                **policy_kwargs):
    """Device-native form of run_muzero_mcts: a DeviceNet, device observations and the 24-bit legal mask
    per game (what the self-play / evaluation loops hold); root inference + Gumbel search, or with
    ``policy="puct"`` root inference + muzero_policy (``policy_kwargs``: its keyword arguments)."""
    if policy not in ("gumbel", "puct"):
        raise ValueError(f"unknown policy {policy!r} ('gumbel' or 'puct')")
    if policy == "gumbel" and policy_kwargs:
        raise TypeError(f"policy='gumbel' takes no {sorted(policy_kwargs)}")
    scratch = workspace.scratch if workspace is not None else None
    logits, value, emb = _N.root_inference_fn(net, observations, scratch)
    if policy == "puct":
        return muzero_policy(net, logits, value, emb, legal_bits, num_simulations, max_depth, temperature,
                             gumbel=gumbel, seed=seed, turn=turn, workspace=workspace, **policy_kwargs)
    return gumbel_muzero_policy(net, logits, value, emb, legal_bits, num_simulations, max_depth, temperature,
                                gumbel=gumbel, seed=seed, turn=turn, workspace=workspace)


def invalid_to_bits(invalid_actions) -> torch.Tensor:
    """bool [B, A] invalid mask (True = illegal, the reference's ``~valid_action``) -> int32 legal bits [B]."""
    inv = invalid_actions if isinstance(invalid_actions, torch.Tensor) else torch.from_numpy(
        np.asarray(invalid_actions, dtype=bool))
    inv = inv.reshape(inv.shape[0], -1).to(torch.bool)
    sh = torch.arange(inv.shape[1], device=inv.device, dtype=torch.int64)
    return ((~inv).to(torch.int64) << sh).sum(1).to(torch.int32)


def run_muzero_mcts(params, rng_key, observations, invalid_actions, num_simulations, max_depth, temperature, *,
                    policy="gumbel", **policy_kwargs):
    """run_muzero_mcts (MuZero_det_MADN/muzero_deterministic_madn.py:663-704), reference signature.

    ``params``: init_muzero_params' nested Flax dict (or a flat dict / DeviceNet, see nets.as_device_net);
    ``rng_key``: int or uint32[2] key (selects the engine's Gumbel stream, nets.rng_key_to_seed);
    ``observations``: [B, C, 56] (NumPy or torch, any device); ``invalid_actions``: bool [B, 24].
    Returns (PolicyOutput(action, action_weights), root_value = search_tree.summary().value) as device
    tensors on cuda.

    Kernel limits (k_gumbel_search; every reference call site is inside them: S = 50 / 100, D = 25 / 50):
    num_simulations 1..100, max_depth 1..64, 24 actions (det-MADN), max_num_considered_actions 16 (mctx's
    default); outside them muz_gumbel_search returns MUZ_E_UNSUPPORTED and this raises MuzError.

    ``policy="puct"`` runs the reference's other policy instead, the mctx.muzero_policy call it keeps commented
    (685-697), with that call's constants: PUCT selection, qtransform_by_min_max(-1, 1), Dirichlet root noise
    0.25 / 0.3, visit-count action_weights, ``temperature`` on the final draw (muzero_policy above; ``policy_kwargs``
    override its keyword arguments, e.g. ``dirichlet_fraction=0`` or ``qtransform="parent_and_siblings"``).  Its limits
    (k_puct_search): num_simulations 1..100, max_depth 1..64, 24 actions, max_value > min_value, dirichlet_fraction in
    [0, 1], dirichlet_alpha > 0, pb_c_base > 0, temperature >= 0; outside them muz_puct_search returns
    MUZ_E_UNSUPPORTED and this raises MuzError."""
    dev = torch.device("cuda")
    net = _N.as_device_net(params, device=dev)
    obs = observations if isinstance(observations, torch.Tensor) else torch.from_numpy(np.asarray(observations))
    obs = obs.to(device=dev, dtype=torch.float32)
    bits = invalid_to_bits(invalid_actions).to(dev)
    return muzero_mcts(net, obs, bits, num_simulations, max_depth, temperature, seed=_N.rng_key_to_seed(rng_key),
                       policy=policy, **policy_kwargs)
