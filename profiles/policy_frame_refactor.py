"""The PUCT policy frame (csrc/tree.hpp) and the environment toolkit (csrc/env_model.hpp) against the parent commit's
library: the same bits from muz_puct_search, muz_detmadn_mcts, muz_classic_mcts and muz_detmadn_gumbel_mcts at a shape
the tests do not reach, and muz_puct_search's time (the line profiles/search_body_refactor.log measured).

    python profiles/policy_frame_refactor.py --parent-lib PATH [--no-time]

Bits: B = 250 (a ragged last workgroup), S = 50, D = 25, rollouts of at most 300 turns, every qtransform of each entry
point, Dirichlet noise at fraction 0.25 once supplied and once drawn on the device, temperature 1 with the final
Gumbel drawn on the device, seed 4321, turn 9.  Each library dumps its arrays from a process of its own (MUZ_LIB);
this process compares them with np.array_equal and never opens the GPU.
Time: 2p B = 4096 S = 50 D = 25 min_max, one warm-up launch then the median of 20 launches, a fresh process per
measurement, parent and new alternating, three pairs.

The other three kernels' times come from profiles/env_mcts_bench.py, classic_env_mcts_bench.py and env_gumbel_bench.py
(--parent-lib)."""
import os
import sys
import tempfile

import _parent_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, D, ROLLOUT, SEED, TURN, FRAC = 250, 50, 25, 300, 4321, 9, 0.25
TB, LAUNCHES, PAIRS = 4096, 20, 3


def _modules():
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import classic as CL
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    from exploring_muzero_on_dog_amd import nets as N
    from exploring_muzero_on_dog_amd import stochastic as ST
    return torch, CL, E, EV, M, N, ST


def _det_roots(torch, E, EV, batch, plies, dev):
    """(states, legal bits): `plies` plies of random play, then the games that have a legal move (repeated to fill)"""
    env = E.env_reset(batch, num_players=2, device=dev, **EV.RULES)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for _ in range(plies):
        bits = E.legal_bits(env)
        live = env.done == 0
        EV._Det.advance(env, EV.random_legal(bits, gen), live, live & (bits != 0))
    bits = E.legal_bits(env)
    ok = ((env.done == 0) & (bits != 0)).nonzero().flatten()
    pick = ok[torch.arange(batch, device=dev) % ok.numel()]
    return env.take(pick), bits[pick].contiguous()


def _classic_roots(torch, CL, EV, batch, turns, dev):
    env = CL.env_reset(batch, num_players=4, device=dev, **CL.SELFPLAY_RULES)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for turn in range(turns + 1):
        CL.throw_die(env, torch.rand((batch,), generator=gen, device=dev))
        bits = CL.legal_bits(env)
        if turn == turns:
            break
        live = env.done == 0
        EV._Classic.advance(env, EV.classic_policy_action(env, bits, "random_agent", 3, turn), live,
                            live & ((bits & 15) != 0))
    ok = ((env.done == 0) & ((bits & 15) != 0)).nonzero().flatten()
    return env.take(ok[torch.arange(batch, device=dev) % ok.numel()])


def dump(path):
    import numpy as np
    torch, CL, E, EV, M, N, ST = _modules()
    dev = torch.device("cuda")
    out = {}

    def keep(name, *arrays):
        for i, t in enumerate(arrays):
            out[f"{name}/{i}"] = t.cpu().numpy()

    rng = np.random.default_rng(1)
    noise = {A: torch.from_numpy(rng.dirichlet([0.3] * A, size=B).astype(np.float32)).to(dev) for A in (24, 4)}
    modes = (("supplied", True), ("drawn", False))

    roots, bits = _det_roots(torch, E, EV, B, 60, dev)
    C = E.num_channels(2)
    net = N.DeviceNet(N.init_muzero_params(1, C), C, device=dev)
    ws = M.SearchWorkspace(B, S, dev)
    lg, v, e = N.root_inference_fn(net, E.encode_board(roots), ws.scratch)
    for qt in ("min_max", "parent_and_siblings"):
        for mode, given in modes:
            pol, rv = M.muzero_policy(net, lg, v, e, bits, S, D, 1.0, qtransform=qt, dirichlet_fraction=FRAC,
                                      dirichlet=noise[24] if given else None, seed=SEED, turn=TURN, workspace=ws)
            keep(f"muz_puct_search {qt} {mode}", pol.action, pol.action_weights, rv)
    # fraction 0, nothing supplied: the parent's k_puct_search drew the noise and multiplied it by 0, this one skips it
    pol, rv = M.muzero_policy(net, lg, v, e, bits, S, D, 1.0, dirichlet_fraction=0.0, seed=SEED, turn=TURN,
                              workspace=ws)
    keep("muz_puct_search min_max fraction 0", pol.action, pol.action_weights, rv)
    ews = M.EnvSearchWorkspace(B, S, dev)
    for qt in ("min_max", "parent_and_siblings"):
        for mode, given in modes:
            pol, rv, vc, q = M.env_muzero_policy(roots, S, D, 1.0, rollout_steps=ROLLOUT, seed=SEED, turn=TURN,
                                                 workspace=ews, summary=True, qtransform=qt, dirichlet_fraction=FRAC,
                                                 dirichlet=noise[24] if given else None)
            keep(f"muz_detmadn_mcts {qt} {mode}", pol.action, pol.action_weights, rv, vc, q, ews.rollout_turns(B))
    for qt in M.GUMBEL_QTRANSFORMS:
        pol, rv, vc, q = M.env_gumbel_muzero_policy(roots, S, D, 1.0, rollout_steps=ROLLOUT, seed=SEED, turn=TURN,
                                                    workspace=ews, summary=True, qtransform=qt)
        keep(f"muz_detmadn_gumbel_mcts {qt}", pol.action, pol.action_weights, rv, vc, q, ews.rollout_turns(B))
    croots = _classic_roots(torch, CL, EV, B, 120, dev)
    cws = ST.ClassicEnvSearchWorkspace(B, S, dev)
    for mode, given in modes:
        pol, rv, vc, q = ST.env_stochastic_muzero_policy(croots, S, D, 1.0, rollout_steps=ROLLOUT, seed=SEED,
                                                         turn=TURN, workspace=cws, summary=True,
                                                         dirichlet_fraction=FRAC,
                                                         dirichlet=noise[4] if given else None)
        keep(f"muz_classic_mcts parent_and_siblings {mode}", pol.action, pol.action_weights, rv, vc, q,
             cws.rollout_turns(B))
    torch.cuda.synchronize()
    np.savez(path, **out)


def time_puct():
    torch, CL, E, EV, M, N, ST = _modules()
    dev = torch.device("cuda")
    roots, bits = _det_roots(torch, E, EV, TB, 40, dev)
    C = E.num_channels(2)
    net = N.DeviceNet(N.init_muzero_params(1, C), C, device=dev)
    ws = M.SearchWorkspace(TB, S, dev)
    lg, v, e = N.root_inference_fn(net, E.encode_board(roots), ws.scratch)
    M.muzero_policy(net, lg, v, e, bits, S, D, 1.0, seed=5, turn=0, workspace=ws)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(LAUNCHES + 1)]
    ev[0].record()
    for i in range(LAUNCHES):
        M.muzero_policy(net, lg, v, e, bits, S, D, 1.0, seed=5, turn=1 + i, workspace=ws)
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(LAUNCHES))
    print(f"{per[LAUNCHES // 2]:.4f}")


def _child(flag, arg, lib, limit=300):
    r = _parent_lib.run_child(__file__, [flag, *arg], lib, limit)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"{flag} ({'parent' if lib else 'new'} library) ended with status {r.returncode}")
    return r.stdout


def main():
    import numpy as np
    parent = _parent_lib.parent_lib(sys.argv)
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for tag, lib in (("parent", parent), ("new", None)):
            files[tag] = os.path.join(tmp, tag + ".npz")
            _child("--dump", [files[tag]], lib)
        a, b = np.load(files["parent"]), np.load(files["new"])
        names = ("action", "weights", "root value", "visit counts", "q-values", "rollout turns")
        print(f"# bits: B={B} S={S} D={D} rollout_steps={ROLLOUT} dirichlet_fraction={FRAC} temperature=1 seed={SEED} "
              f"turn={TURN}; np.array_equal(parent, new) per array")
        bad = 0
        for case in sorted({k.rsplit("/", 1)[0] for k in a.files}):
            res = []
            for i, nm in enumerate(names):
                k = f"{case}/{i}"
                if k in a.files:
                    same = bool(np.array_equal(a[k], b[k]))
                    bad += 0 if same else 1
                    res.append(f"{nm} {'equal' if same else 'DIFFERS'}")
            searched = int((a[f"{case}/0"] >= 0).sum())
            print(f"{case}: {', '.join(res)} ({searched} of {B} roots searched)")
        print(f"# {len(a.files)} arrays, {bad} differ")
    if "--no-time" not in sys.argv:
        ms = {"parent": [], "new": []}
        for _ in range(PAIRS):
            for tag, lib in (("parent", parent), ("new", None)):
                ms[tag].append(float(_child("--time-puct", [], lib)))
        print(f"# muz_puct_search, 2p B={TB} S={S} D={D} min_max, median of {LAUNCHES} launches, ms per launch, "
              f"alternating")
        for tag in ("parent", "new"):
            xs = ms[tag]
            print(f"{tag:6s} {' '.join(f'{x:.4f}' for x in xs)}   median {sorted(xs)[len(xs) // 2]:.4f}   "
                  f"min {min(xs):.4f} max {max(xs):.4f}")
    return 1 if bad else 0


if __name__ == "__main__":
    if "--dump" in sys.argv:
        sys.exit(dump(sys.argv[sys.argv.index("--dump") + 1]))
    if "--time-puct" in sys.argv:
        sys.exit(time_puct())
    sys.exit(main())
