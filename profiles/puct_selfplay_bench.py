"""Self-play with the PUCT muzero_policy search beside the Gumbel one, the yardstick: 2 players, 4096 lanes, S = 50,
D = 25, a randomly initialised net; play_stream of 16,384 games with each policy, the two interleaved over 3
repetitions after one warm-up call each; HIP-event times from the engine's own statistics.

    python profiles/puct_selfplay_bench.py [--parent DIR]     # writes profiles/puct_selfplay_bench.log

--parent DIR: a built checkout of the parent commit.  The script then also runs `bench.py --workload det` (the Gumbel
headline) from this tree and from DIR, alternating, RUNS times each, and logs both sets of values: k_gumbel_search is
not edited by the PUCT self-play, so the new mean has to lie within the parent's own run-to-run spread.

Every measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "puct_selfplay_bench.log")
P, LANES, GAMES, S, D, T, REPS = 2, 4096, 16384, 50, 25, 500, 3
RUNS, HEADLINE_ARGS = 3, ["--gpus", "1", "--steps", "1", "--warmup", "1", "--workload", "det"]


def child():
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import game_agent as GA
    from exploring_muzero_on_dog_amd import nets as N

    C = E.num_channels(P)
    net = N.DeviceNet(N.init_muzero_params(0, C), C)
    kw = dict(num_players=P, max_steps=T, num_simulations=S, max_depth=D)
    eng = {"gumbel": GA.SelfPlayEngine(net, LANES, **kw), "puct": GA.SelfPlayEngine(net, LANES, policy="puct", **kw)}
    print(f"shape: {P}p, {LANES} lanes, {GAMES} games per call streamed, S={S} D={D} max_steps={T}, random-init net, "
          f"temperature 1, {REPS} repetitions, interleaved, one warm-up call each", flush=True)

    def call(name, seed):
        e = eng[name]
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        buf = e.play_stream(GAMES, seed=seed, temperature=1.0)
        t1.record()
        torch.cuda.synchronize()
        st = dict(e.last_stats)
        st["wall_ms"] = t0.elapsed_time(t1)
        st["steps"] = int(buf["idx"].sum().item())
        return st

    for name in eng:
        call(name, 1)
    rows = {"gumbel": [], "puct": []}
    for rep in range(REPS):
        for name in eng:
            st = call(name, 1000 + rep)
            rows[name].append(st)
            print(f"rep {rep} {name:6s}: {st['steps'] / st['wall_ms']:.1f} k env-steps/s, "
                  f"{st['searches'] * S / st['wall_ms'] / 1e3:.2f} M sims/s, search_ms / total_ms "
                  f"{st['search_ms']:.1f} / {st['total_ms']:.1f} = {st['search_ms'] / st['total_ms']:.3f}, "
                  f"{st['turns']} launched turns, {st['searches'] / st['turns']:.1f} searches per launched turn, "
                  f"{st['search_ms'] / st['turns']:.3f} ms search and "
                  f"{(st['total_ms'] - st['search_ms']) / st['turns'] * 1e3:.1f} us rest per turn, "
                  f"{st['steps']} env-steps in {st['wall_ms']:.1f} ms", flush=True)

    def med(name, f):
        return sorted(f(st) for st in rows[name])[REPS // 2]

    out = {}
    for name in eng:
        out[name] = dict(rate=med(name, lambda st: st["steps"] / st["wall_ms"] * 1e3),
                         sims=med(name, lambda st: st["searches"] * S / st["wall_ms"] * 1e3),
                         share=med(name, lambda st: st["search_ms"] / st["total_ms"]),
                         per_turn=med(name, lambda st: st["searches"] / st["turns"]),
                         search_turn=med(name, lambda st: st["search_ms"] / st["turns"]),
                         rest_turn=med(name, lambda st: (st["total_ms"] - st["search_ms"]) / st["turns"]),
                         turns=med(name, lambda st: st["turns"]),
                         length=med(name, lambda st: st["steps"] / GAMES))
        o = out[name]
        print(f"{name:6s} (median of {REPS}): {o['rate'] / 1e3:.1f} k env-steps/s, {o['sims'] / 1e6:.2f} M sims/s, "
              f"search_ms / total_ms {o['share']:.3f}, {o['per_turn']:.1f} searches per launched turn, "
              f"{o['search_turn']:.3f} ms search + {o['rest_turn'] * 1e3:.1f} us rest per launched turn, "
              f"{o['turns']} launched turns, {o['length']:.1f} recorded turns per game")
    g, p = out["gumbel"], out["puct"]
    print(f"ratio puct / gumbel: time per env-step {g['rate'] / p['rate']:.3f}, time per simulation "
          f"{g['sims'] / p['sims']:.3f}, search time per launched turn {p['search_turn'] / g['search_turn']:.3f}, "
          f"rest of the turn {p['rest_turn'] / g['rest_turn']:.3f}, recorded turns per game "
          f"{p['length'] / g['length']:.3f} (the isolated search: 1.075, profiles/puct_search_bench.log)")


def headline(tree):
    """One `bench.py --workload det` run from `tree` -> (env-steps/s or None, its output)."""
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + HEADLINE_ARGS, cwd=tree, capture_output=True,
                       text=True, timeout=240)
    value = None
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            try:
                value = json.loads(line)["value"]
            except (ValueError, KeyError):
                pass
    return (value if r.returncode == 0 else None), r.stdout + r.stderr


def main():
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                       timeout=300)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        return r.returncode
    text = r.stdout
    if parent:
        vals = {"parent": [], "this": []}
        for run in range(RUNS):
            for name, tree in (("parent", os.path.abspath(parent)), ("this", ROOT)):
                v, out = headline(tree)
                if v is None:            # nothing more is started on the GPU after a failed run
                    sys.stderr.write(out)
                    return 1
                vals[name].append(v)
                print(f"headline run {run} {name:6s}: {v:.0f} env-steps/s", flush=True)
        lines = [f"Gumbel headline, bench.py {' '.join(HEADLINE_ARGS)}, parent commit and this one alternating:"]
        for name in ("parent", "this"):
            v = vals[name]
            lines.append(f"  {name:6s}: " + ", ".join(f"{x:.0f}" for x in v)
                         + f" env-steps/s; mean {sum(v) / len(v):.0f}, spread {min(v):.0f} .. {max(v):.0f}")
        m, pv = sum(vals["this"]) / RUNS, vals["parent"]
        lines.append(f"  this commit's mean {m:.0f} is {'within' if min(pv) <= m <= max(pv) else 'OUTSIDE'} the parent's "
                     f"spread ({m / (sum(pv) / RUNS):.4f} of the parent's mean)")
        print("\n".join(lines))
        text += "\n".join(lines) + "\n"
    with open(LOG, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else main())
