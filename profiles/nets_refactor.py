"""The host side of the det, classic and DOG networks before and after it was put on one construction path: what the
public entry points compute, two packages compared bit for bit, and the per-turn wrappers timed on both, alternating.

    python profiles/nets_refactor.py ab PARENT_PKG [--log F] [--out DIR]     # writes profiles/nets_refactor.log
    python profiles/nets_refactor.py run --pkg DIR --out F.npz [--time]
    python profiles/nets_refactor.py compare A.npz B.npz

PARENT_PKG is a directory that holds the parent commit's package (``git archive`` of exploring-muzero-on-dog_amd/,
with the same libmuz.so beside it).  ``ab`` runs every side in a child process of its own under a time limit and stops
at the first one that fails; this process never opens the GPU.

Per game a run records: the packed net's buffer; root inference at B = 1 and B = 17 (one row, and one row past the
packed layers' 16-row tile) on a fixed integer-valued observation; the recurrent outputs on those embeddings (classic:
decision, then chance); every parameter after 3 graph-captured train steps from ``make_optimizer(cfg).init(tree)`` on
one fixed batch in the ring's format (B = 8, unroll 5).  ``--time``: 2,000 back-to-back root_inference_fn calls at
B = 17 and one synchronise, and 200 as_device_* calls on an unchanged tree."""
import argparse
import io
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "nets_refactor.log")
OUT = os.path.join(ROOT, "profiles", "_exp")     # the .npz files of ``ab`` (kept out of git)
CFG = {"unroll_steps": 5, "learning_rate": 0.005, "train_steps_per_iteration": 10}
BATCH, ROOT_CALLS, CACHE_CALLS = 8, 2000, 200


def games(pkg_dir):
    """{game: dict of the package's entry points and fixed parameters}."""
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.PKG_DIR = os.path.abspath(pkg_dir)
    muzpkg.load()
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    from exploring_muzero_on_dog_amd import nets as N
    from exploring_muzero_on_dog_amd import stochastic as ST
    from exploring_muzero_on_dog_amd import train_dog as TD
    from exploring_muzero_on_dog_amd import train_stochastic as TS
    from exploring_muzero_on_dog_amd import train_with_reward as TW
    det, cla, dog = N.init_muzero_params(3, 34), ST.init_classic_params(11, seed=3), MD.init_muzero_params(3)
    return {
        "det": dict(params=det, C=34, A=24, net=lambda: N.DeviceNet(det, 34), as_device=N.as_device_net,
                    root=N.root_inference_fn, rec=[N.recurrent_inference_fn], script=TW),
        "classic": dict(params=cla, C=11, A=4, net=lambda: ST.DeviceClassicNet(cla, 11),
                        as_device=ST.as_device_classic_net, root=ST.root_inference_fn,
                        rec=[ST.decision_recurrent_fn, ST.chance_recurrent_fn], script=TS),
        "dog": dict(params=dog, C=34, A=806, net=lambda: MD.DeviceDogNet(dog), as_device=MD.as_device_net,
                    root=MD.root_inference_fn, rec=[MD.recurrent_inference_fn], script=TD),
    }


def ring_batch(game, C, A, K):
    """One fixed batch with the keys, shapes and dtypes of the device ring's sample_batch."""
    import numpy as np
    import torch
    rng = np.random.default_rng(17)
    B = BATCH
    pol = rng.random((B, K + 1, A)).astype(np.float32)
    b = {"observations": rng.integers(0, 5, (B, C, 56)).astype(np.float32),
         "actions": rng.integers(-1, A, (B, K)).astype(np.int32),
         "rewards": rng.integers(0, 3, (B, K)).astype(np.int32),
         "policies": pol / pol.sum(-1, keepdims=True),
         "values": rng.uniform(-1, 1, (B, K + 1)).astype(np.float32),
         "masks": (rng.random((B, K + 1)) > 0.2).astype(np.float32),
         "target_values": rng.uniform(-1, 1, (B, K + 1)).astype(np.float32),
         "discount_targets": rng.integers(0, 3, (B, K)).astype(np.int32)}
    if game == "classic":
        pr = rng.random((B, K, 6)).astype(np.float32)
        b["dice_outcomes"] = rng.integers(0, 6, (B, K)).astype(np.int32)
        b["dice_probs"] = pr / pr.sum(-1, keepdims=True)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


def run(args):
    import numpy as np
    import torch
    todo = games(args.pkg)
    from exploring_muzero_on_dog_amd import checkpoint as CK
    arrays, timed = {}, []
    for game, g in todo.items():
        net = g["net"]()
        arrays[f"{game}/buffer"] = net.buffer.cpu().numpy()
        rng = np.random.default_rng(5)
        for B in (1, 17):
            obs = torch.from_numpy(rng.integers(0, 5, (B, g["C"], 56)).astype(np.float32)).cuda()
            logits, value, emb = g["root"](net, obs)
            outs = {"root/logits": logits, "root/value": value, "root/embedding": emb}
            idx = torch.from_numpy(rng.integers(0, min(g["A"], 6), (B,)).astype(np.int32)).cuda()
            state = emb
            for n, fn in enumerate(g["rec"]):
                res = fn(net, idx, state)
                outs.update({f"recurrent{n}/{i}": t for i, t in enumerate(res)})
                state = res[2]       # decision_recurrent_fn's afterstate (fed to chance_recurrent_fn)
            arrays.update({f"{game}/B{B}/{k}": t.cpu().numpy() for k, t in outs.items()})
        if args.time:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ROOT_CALLS):
                g["root"](net, obs)
            torch.cuda.synchronize()
            timed.append((f"{game} root_inference_fn", (time.perf_counter() - t0) / ROOT_CALLS * 1e6))
            g["as_device"](g["params"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CACHE_CALLS):
                g["as_device"](g["params"])
            torch.cuda.synchronize()
            timed.append((f"{game} as_device", (time.perf_counter() - t0) / CACHE_CALLS * 1e6))
        del net
        # 3 graph-captured train steps from optimizer.init on the Flax tree, as the reference's loop starts
        S = g["script"]
        tree = CK.flat_to_muzero_tree(g["params"])
        st = S.make_optimizer(CFG).init(tree)
        params, batch = st.tree, ring_batch(game, g["C"], g["A"], CFG["unroll_steps"])
        for _ in range(3):
            params, st, losses = S.train_step(params, st, batch)
        arrays.update({f"{game}/trained/{k}": v.detach().cpu().numpy() for k, v in st.learner.nets.p.items()})
        arrays.update({f"{game}/losses/{k}": v.detach().cpu().numpy() for k, v in losses.items()})
        del st, params
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **arrays)
    for name, us in timed:
        print(f"timed {name}: {us:.2f} us/call", flush=True)
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
          f"{'all equal bit for bit' if not bad else str(len(bad)) + ' DIFFERENT: ' + ', '.join(bad[:20])}",
          file=out, flush=True)
    return 1 if bad else 0


def ab(parent_pkg, log, out):
    sys.path.insert(0, ROOT)
    import muzpkg
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish(rc):
        with open(log, "w") as f:
            f.write("\n".join(lines) + "\n")
        return rc

    sides = {"parent": parent_pkg, "result": muzpkg.PKG_DIR}
    us = {k: {} for k in sides}
    npz = {k: [os.path.join(out, f"nets_{k}_{rep}.npz") for rep in range(3)] for k in sides}
    for rep in range(3):
        for side, pkg in sides.items():
            cmd = [sys.executable, os.path.abspath(__file__), "run", "--pkg", pkg, "--time", "--out", npz[side][rep]]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
            except subprocess.TimeoutExpired:
                say(f"{side} run {rep}: no result within 400 s")
                return finish(124)
            sys.stderr.write(r.stderr)
            if r.returncode != 0:
                say(f"{side} run {rep}: exit {r.returncode}")
                return finish(r.returncode)
            for line in r.stdout.splitlines():
                if line.startswith("timed "):
                    name, val = line[6:].split(": ")
                    us[side].setdefault(name, []).append(float(val.split()[0]))
            say(f"{side} run {rep}: " + ", ".join(f"{n} {v[-1]:.1f}" for n, v in us[side].items()) + " (us/call)")
    rc = 0
    for other in npz["parent"][1:] + npz["result"]:
        buf = io.StringIO()
        rc |= compare(npz["parent"][0], other, buf)
        say(buf.getvalue().strip())
    for name in us["parent"]:
        p, n = us["parent"][name], us["result"][name]
        mean = sum(n) / len(n)
        inside = min(p) <= mean <= max(p)
        say(f"{name}: parent mean {sum(p) / len(p):.2f} us (min {min(p):.2f}, max {max(p):.2f}); result mean {mean:.2f} us "
            f"(min {min(n):.2f}, max {max(n):.2f}): " + ("within the parent's spread" if inside else
                                                      f"{mean - sum(p) / len(p):+.2f} us/call against the parent's mean"))
    return finish(rc)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--pkg", required=True)
    r.add_argument("--out", required=True)
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
