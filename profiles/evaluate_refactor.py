"""evaluate.py before and after a change of its Python layer: a fixed set of small evaluation calls, every returned
table and every tensor of the four-seat calls' final states written to an .npz, two packages compared bit for bit, and
the call set timed on both, alternating.

    python profiles/evaluate_refactor.py ab PARENT_PKG [--log F] [--out DIR]  # writes profiles/evaluate_refactor.log
    python profiles/evaluate_refactor.py run --pkg DIR --out F.npz [--golden F.json] [--time]
    python profiles/evaluate_refactor.py compare A.npz B.npz

PARENT_PKG is a directory that holds the parent commit's package (``git archive`` of exploring-muzero-on-dog_amd/,
with the same libmuz.so beside it).  ``ab`` runs every side in a child process of its own under a time limit and stops
at the first one that fails; this process never opens the GPU.  ``--golden`` writes the tables of the scripted-seat
calls (no network, so no float arithmetic of a search) as JSON: tests/golden/evaluate_scripted_seats.json is the
parent's."""
import argparse
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "evaluate_refactor.log")
OUT = os.path.join(ROOT, "profiles", "_exp")     # the .npz files of ``ab`` (kept out of git)
SMALL = dict(num_simulations=4, max_depth=4)
MIX = ("net", None, "rule_based_agent", "random_agent")
GOLDEN_KEYS = ("winners", "average_progress", "finished", "turns")


def calls(pkg_dir):
    """[(name, thunk)]: the fixed call set on the package in ``pkg_dir``."""
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.PKG_DIR = os.path.abspath(pkg_dir)
    muzpkg.load()
    from exploring_muzero_on_dog_amd import classic as CL
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    from exploring_muzero_on_dog_amd import nets as N
    from exploring_muzero_on_dog_amd import stochastic as ST

    C = E.num_channels(4)
    net = N.DeviceNet(N.init_muzero_params(3, C), C)
    cparams = ST.init_classic_params(CL.num_channels(4), seed=3)
    dparams = MD.init_muzero_params(4)
    det = [net if a == "net" else a for a in MIX]
    cla = [cparams if a == "net" else a for a in MIX]
    scripted = ["rule_based_agent", "random_agent"] * 2
    return [
        ("det4_gumbel", lambda: EV.evaluate_agent_parallel(det, batch_size=2, seed=4, max_turns=300, search="gumbel",
                                                           **SMALL)),
        ("det4_puct", lambda: EV.evaluate_agent_parallel(det, batch_size=2, seed=4, max_turns=300, search="puct",
                                                         **SMALL)),
        ("classic4", lambda: EV.evaluate_agent_parallel_classic(cla, batch_size=2, seed=4, max_turns=300, **SMALL)),
        ("dog4", lambda: EV.evaluate_agent_parallel_dog([dparams, "random_agent", None, "random_agent"], batch_size=2,
                                                        seed=6, max_turns=200, **SMALL)),
        ("pvr_net", lambda: EV.play_vs_random(net, 8, seed=5, **SMALL)),
        ("pvr_net_puct", lambda: EV.play_vs_random(net, 8, seed=5, search="puct", **SMALL)),
        ("pvr_none", lambda: EV.play_vs_random(None, 8)),
        ("pvr_classic", lambda: EV.play_vs_random_classic(cparams, 8, seed=9, **SMALL)),
        ("pvr_classic_rule", lambda: EV.play_vs_random_classic("rule_based_agent", 8, seed=9)),
        ("det_scripted", lambda: EV.evaluate_agent_parallel(scripted, batch_size=4, seed=7)),
        ("classic_scripted", lambda: EV.evaluate_agent_parallel_classic(scripted, batch_size=4, seed=7)),
        ("dog_scripted", lambda: EV.evaluate_agent_parallel_dog(["random_agent"] * 4, batch_size=4, seed=3)),
    ]


def run(args):
    import numpy as np
    import torch
    todo = calls(args.pkg)
    arrays, golden = {}, {}
    for name, fn in todo:
        r = fn()
        st = r.pop("final_state", None)
        for k, v in r.items():
            arrays[f"{name}/{k}"] = np.asarray(v)
        if st is not None:
            for k, v in vars(st).items():
                if isinstance(v, torch.Tensor):
                    arrays[f"{name}/final_state/{k}"] = v.cpu().numpy()
        if name.endswith("_scripted"):
            golden[name] = {k: r[k] for k in GOLDEN_KEYS if k in r}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **arrays)
    if args.golden:
        with open(args.golden, "w") as f:
            json.dump(golden, f, indent=1)
            f.write("\n")
    if args.time:      # a second pass over the call set, everything loaded and warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _, fn in todo:
            fn()
        torch.cuda.synchronize()
        print(f"call set: {time.perf_counter() - t0:.3f} s", flush=True)
    return 0


def compare(a_path, b_path, out=sys.stdout):
    import numpy as np
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    print(f"compare {os.path.basename(a_path)} {os.path.basename(b_path)}: {len(a.files)} arrays, "
          f"{'all equal bit for bit' if not bad else 'DIFFERENT: ' + ', '.join(bad)}", file=out, flush=True)
    return 1 if bad else 0


def ab(parent_pkg, log, out):
    sys.path.insert(0, ROOT)
    import muzpkg
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sides = {"parent": parent_pkg, "result": muzpkg.PKG_DIR}
    secs = {k: [] for k in sides}
    npz = {k: [os.path.join(out, f"evaluate_{k}_{rep}.npz") for rep in range(3)] for k in sides}
    for rep in range(3):
        for side, pkg in sides.items():
            cmd = [sys.executable, os.path.abspath(__file__), "run", "--pkg", pkg, "--time", "--out", npz[side][rep]]
            if side == "parent" and rep == 0:
                cmd += ["--golden", os.path.join(out, "evaluate_golden.json")]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
            sys.stderr.write(r.stderr)
            if r.returncode != 0:
                say(f"{side} run {rep}: exit {r.returncode}")
                return r.returncode
            secs[side].append(float(r.stdout.split("call set:")[1].split()[0]))
            say(f"{side} run {rep}: call set {secs[side][-1]:.3f} s")
    rc = 0
    for other in npz["parent"][1:] + npz["result"]:
        buf = io.StringIO()
        rc |= compare(npz["parent"][0], other, buf)
        say(buf.getvalue().strip())
    for side, v in secs.items():
        say(f"{side}: mean {sum(v) / 3:.3f} s, min {min(v):.3f}, max {max(v):.3f}")
    with open(log, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--pkg", required=True)
    r.add_argument("--out", required=True)
    r.add_argument("--golden")
    r.add_argument("--time", action="store_true")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    a = sub.add_parser("ab")
    a.add_argument("parent_pkg")
    a.add_argument("--log", default=LOG)
    a.add_argument("--out", default=OUT, help="directory of the .npz files")
    args = ap.parse_args()
    if args.cmd == "run":
        return run(args)
    if args.cmd == "compare":
        return compare(args.a, args.b)
    return ab(args.parent_pkg, args.log, args.out)


if __name__ == "__main__":
    sys.exit(main())
