"""Persistent PUCT search kernel (csrc/puct_search.hip, mcts.muzero_policy) vs the NumPy restatement of mctx 0.0.6
muzero_policy (tests/_mctx_muzero.py) on the GPU.

Search logic only: the restatement is driven by the GPU's own recurrent_inference kernel, so both sides see identical
network outputs and the tree arithmetic is compared (it is written to agree bit for bit).  The action weights are
visit fractions, so the 1e-5 bound of tests/_parity.py means identical visit counts.  There is no end-to-end case
against the NumPy networks: a 1e-6 network deviation can move one visit, 1 / S in the weights, and the networks are
pinned by tests/test_gpu_nets*.py.  Parity vs mctx itself is unpinned (mctx is not vendored in the reference)."""
import functools

import numpy as np
import pytest
import torch

from oracle import detmadn as dm
from oracle import nets as ON
from tests import _mctx_muzero as PZ
from tests._parity import log, search_parity
from tests.test_gpu_nets import random_obs
from tests.test_gpu_search import gpu_recurrent_fn

pytestmark = pytest.mark.gpu

B = 37   # two full 16-game tiles and a ragged one of 5
RULE_SET = {2: "selfplay_2p", 4: "selfplay_4p_teams"}


def _mods():
    from exploring_muzero_on_dog_amd import mcts as M
    from exploring_muzero_on_dog_amd import nets as N
    return N, M


@functools.lru_cache(maxsize=None)
def setup(P):
    """Network, B observations with a legal move each and their root inference, shared by the cases of P players."""
    N, M = _mods()
    C = dm.num_channels(P)
    params = ON.init_params(C, seed=7, randomize_affine=True)
    net = N.DeviceNet(params, C)
    obs, envs = random_obs(RULE_SET[P], 64, 12)
    valid = np.stack([dm.valid_action(e).flatten() for e in envs])
    keep = np.flatnonzero(valid.any(1))[:B]
    assert keep.size == B
    obs, valid = obs[keep], valid[keep]
    bits = torch.from_numpy((valid.astype(np.int64) << np.arange(24)).sum(1).astype(np.int32))
    root = N.root_inference_fn(net, torch.from_numpy(obs).cuda())
    return params, net, obs, valid, bits, root


# (P, S, D): the Gumbel search's shapes and the smallest search; qtransform x temperature x dirichlet_fraction spread
# over them so that each value meets each other value and every shape sees both qtransforms
CASES = [
    (2, 50, 25, "min_max", 1.0, 0.25),
    (2, 50, 25, "parent_and_siblings", 0.0, 0.0),
    (2, 50, 25, "min_max", 0.0, 0.25),
    (4, 16, 4, "min_max", 0.0, 0.0),
    (4, 16, 4, "parent_and_siblings", 1.0, 0.25),
    (4, 16, 4, "parent_and_siblings", 0.0, 0.25),
    (2, 8, 50, "min_max", 1.0, 0.0),
    (2, 8, 50, "parent_and_siblings", 0.0, 0.25),
    (4, 100, 50, "min_max", 1.0, 0.25),          # config (e)'s search shape
    (4, 100, 50, "parent_and_siblings", 1.0, 0.0),
    (2, 1, 1, "min_max", 1.0, 0.25),
    (2, 1, 1, "parent_and_siblings", 0.0, 0.0),
]


@pytest.mark.parametrize("P,S,D,qt,temp,frac", CASES)
def test_puct_search_logic_matches_mctx_restatement(cuda, P, S, D, qt, temp, frac):
    N, M = _mods()
    params, net, obs, valid, bits, (lg, v, e) = setup(P)
    rng = np.random.default_rng(3)
    dirichlet = rng.dirichlet(np.full(24, 0.3), B).astype(np.float32)
    gum = rng.gumbel(size=(B, 24)).astype(np.float32)
    gids = (7 * np.arange(B) + 3).astype(np.int32)
    seed, turn = 4321, 9
    pol, rv = M.muzero_policy(net, lg, v, e, bits, S, D, temp, qtransform=qt, dirichlet_fraction=frac,
                              dirichlet=torch.from_numpy(dirichlet), gumbel=torch.from_numpy(gum), seed=seed, turn=turn,
                              game_id=torch.from_numpy(gids))
    trace = {}
    a, w, orv, _ = PZ.muzero_policy(params, lg.cpu().numpy(), v.cpu().numpy(), e.cpu().numpy(),
                                    gpu_recurrent_fn(N, net), S, ~valid, dirichlet, gum, max_depth=D,
                                    temperature=temp, qtransform=qt, dirichlet_fraction=frac, seed=seed, turn=turn,
                                    gids=gids, trace=trace)
    torch.cuda.synchronize()
    ga, gw, grv = pol.action.cpu().numpy(), pol.action_weights.cpu().numpy(), rv.cpu().numpy()
    search_parity(f"puct search logic P{P} S{S} D{D} {qt} T{temp} f{frac}", ga, gw, grv, a, w, orv, trace["margin"],
                  gain=None)
    assert valid[np.arange(B), ga].all(), "search picked an invalid root action"
    excused = int((ga != a).sum())
    log(f"puct search logic P{P} S{S} D{D} {qt} T{temp} f{frac}: {excused} of {B} games excused as near-ties "
        f"(at most 2 allowed); identical visit counts in {int((np.rint(gw * S) == np.rint(w * S)).all(-1).sum())}")
    assert excused <= 2


@pytest.mark.parametrize("qt,frac,with_gids", [("min_max", 0.25, True), ("min_max", 1.0, False),
                                               ("parent_and_siblings", 0.25, False),
                                               ("parent_and_siblings", 1.0, True)])
def test_puct_search_device_noise(cuda, qt, frac, with_gids):
    """The root noise drawn inside k_puct_search (dirichlet=None): the restatement is fed the float32 restatement of
    the device stream (oracle/root_noise.py) for the same (seed, game ids, turn), which pins the kernel's keying, its
    row normalisation and the mixing; at dirichlet_fraction 1 the prior is the noise alone.  Excuses: the oracle's own
    near-ties and the games with a Gamma draw whose float64 acceptance margin is below the threshold of
    tests/_root_noise.py (left out)."""
    from oracle import root_noise as RN
    from tests import _root_noise as H
    N, M = _mods()
    P, S, D, temp = 2, 16, 8, 1.0
    params, net, obs, valid, bits, (lg, v, e) = setup(P)
    gum = np.random.default_rng(3).gumbel(size=(B, 24)).astype(np.float32)
    gids = (7 * np.arange(B) + 3).astype(np.int32)[::-1].copy() if with_gids else np.arange(B, dtype=np.int32)
    seed, turn = 4321, 9
    pol, rv = M.muzero_policy(net, lg, v, e, bits, S, D, temp, qtransform=qt, dirichlet_fraction=frac, dirichlet=None,
                              gumbel=torch.from_numpy(gum), seed=seed, turn=turn,
                              game_id=torch.from_numpy(gids) if with_gids else None)
    r32 = RN.root_noise(seed, gids, turn, 0.3, 24, np.float32)
    r64 = RN.root_noise(seed, gids, turn, 0.3, 24, np.float64)
    ok = ~(r64["margin"] < H.threshold([(r32, r64)])).any(1)
    assert (~ok).sum() <= H.MAX_EXCUSED * B
    trace = {}
    a, w, orv, _ = PZ.muzero_policy(params, lg.cpu().numpy(), v.cpu().numpy(), e.cpu().numpy(),
                                    gpu_recurrent_fn(N, net), S, ~valid, r32["noise"], gum, max_depth=D,
                                    temperature=temp, qtransform=qt, dirichlet_fraction=frac, seed=seed, turn=turn,
                                    gids=gids, trace=trace)
    torch.cuda.synchronize()
    ga, gw, grv = pol.action.cpu().numpy(), pol.action_weights.cpu().numpy(), rv.cpu().numpy()
    label = f"puct search device noise P{P} S{S} D{D} {qt} f{frac} game_id {'given' if with_gids else 'none'}"
    search_parity(label, ga[ok], gw[ok], grv[ok], a[ok], w[ok], orv[ok], trace["margin"][ok], gain=None)
    assert valid[np.arange(B), ga].all(), "search picked an invalid root action"
    excused = int((ga[ok] != a[ok]).sum())
    log(f"{label}: games excused by the noise's acceptance margin {int((~ok).sum())} of {B}, by an oracle near-tie "
        f"{excused} (at most 2 allowed)")
    assert excused <= 2


def test_puct_device_rng_is_deterministic_and_valid(cuda):
    N, M = _mods()
    params, net, obs, valid, bits, (lg, v, e) = setup(2)
    S = 16
    gid = torch.arange(B, dtype=torch.int32) + 100
    kw = dict(turn=7, game_id=gid)
    p1, v1 = M.muzero_policy(net, lg, v, e, bits, S, 8, 1.0, seed=123, **kw)
    p2, v2 = M.muzero_policy(net, lg, v, e, bits, S, 8, 1.0, seed=123, **kw)
    p3, _ = M.muzero_policy(net, lg, v, e, bits, S, 8, 1.0, seed=124, **kw)
    torch.cuda.synchronize()
    assert torch.equal(p1.action, p2.action) and torch.equal(p1.action_weights, p2.action_weights)
    assert torch.equal(v1, v2)
    assert not torch.equal(p1.action_weights, p3.action_weights)
    ga, w = p1.action.cpu().numpy(), p1.action_weights.cpu().numpy()
    assert valid[np.arange(B), ga].all()
    assert np.abs(w.sum(1) - 1.0).max() <= 1e-6 and (w[~valid] == 0).all()
    assert np.abs(w * S - np.rint(w * S)).max() <= 1e-5 and (np.rint(w * S).sum(1) == S).all()
    assert np.isfinite(v1.cpu().numpy()).all()


def test_run_muzero_mcts_routes_both_policies(cuda):
    from exploring_muzero_on_dog_amd import checkpoint as CK
    N, M = _mods()
    C = dm.num_channels(2)
    flat = N.init_muzero_params(4, C)
    tree = CK.flat_to_muzero_tree(flat)
    _, _, obs, valid, bits, _ = setup(2)
    net = N.DeviceNet(flat, C)
    lg, v, e = N.root_inference_fn(net, torch.from_numpy(obs).cuda())
    pol, rv = M.run_muzero_mcts(tree, 1234, obs, ~valid, 16, 8, 1.0, policy="puct")
    pol2, rv2 = M.muzero_policy(net, lg, v, e, bits, 16, 8, 1.0, seed=1234)
    assert torch.equal(pol.action, pol2.action) and torch.equal(pol.action_weights, pol2.action_weights)
    assert torch.equal(rv, rv2)
    w = pol.action_weights.cpu().numpy()
    assert np.abs(w * 16 - np.rint(w * 16)).max() <= 1e-5      # visit fractions, not the Gumbel policy's softmax
    # further keywords reach muzero_policy
    pol3, _ = M.run_muzero_mcts(tree, 1234, obs, ~valid, 16, 8, 1.0, policy="puct", dirichlet_fraction=0.0,
                                qtransform="parent_and_siblings")
    pol4, _ = M.muzero_policy(net, lg, v, e, bits, 16, 8, 1.0, seed=1234, dirichlet_fraction=0.0,
                              qtransform="parent_and_siblings")
    assert torch.equal(pol3.action_weights, pol4.action_weights)
    assert not torch.equal(pol3.action_weights, pol.action_weights)
    # the default path is today's call
    g0, gv0 = M.run_muzero_mcts(tree, 1234, obs, ~valid, 16, 8, 1.0)
    g1, gv1 = M.run_muzero_mcts(tree, 1234, obs, ~valid, 16, 8, 1.0, policy="gumbel")
    g2, gv2 = M.gumbel_muzero_policy(net, lg, v, e, bits, 16, 8, 1.0, seed=1234)
    for g, gv in ((g1, gv1), (g2, gv2)):
        assert torch.equal(g0.action, g.action) and torch.equal(g0.action_weights, g.action_weights)
        assert torch.equal(gv0, gv)


def test_evaluation_seats_search_with_puct(cuda):
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    N, M = _mods()
    C = E.num_channels(4)
    net = N.DeviceNet(ON.init_params(C, seed=3), C)
    agents = [net, "random_agent", None, "rule_based_agent"]
    r = EV.evaluate_agent_parallel(agents, batch_size=4, num_simulations=8, max_depth=4, seed=4, search="puct")
    assert r["games"] == 16 and r["finished"] == 16
    assert sum(r["wins_per_player"]) == 2 * 16                  # teams: both partners of the winning team
    # the default reproduces today's results
    kw = dict(batch_size=4, num_simulations=8, max_depth=4, seed=4, max_turns=40)
    a = EV.evaluate_agent_parallel(agents, **kw)
    b = EV.evaluate_agent_parallel(agents, search="gumbel", **kw)
    c = EV.evaluate_agent_parallel(agents, search="puct", **kw)
    assert a["average_progress"] == b["average_progress"] and a["winners"] == b["winners"]
    assert a["average_progress"] != c["average_progress"]
    wins, prog = EV.test_agent_vs_random(net, 8, batch_size=8, num_players=4, num_simulations=8, max_depth=4,
                                         max_turns=40, search="puct")
    assert 0 <= wins <= 8 and len(prog) == 4
