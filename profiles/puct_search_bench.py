"""muz_puct_search beside muz_gumbel_search, the yardstick: 2 players, B = 4096, S = 50, D = 25, a randomly initialised
net, root states from random play; the two searches interleaved, 3 repetitions of 20 launches each, HIP events.

    python profiles/puct_search_bench.py            # writes profiles/puct_search_bench.log

The measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "puct_search_bench.log")
B, S, D, REPS, LAUNCHES = 4096, 50, 25, 3, 20
FLOP_PER_SIM = 1_867_648          # Dyn4 + Pred4 per simulation per game
PEAK_TFLOPS = 157.3               # fp32 MFMA, dense


def child():
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    from exploring_muzero_on_dog_amd import nets as N

    dev = torch.device("cuda")
    P = 2
    C = E.num_channels(P)
    net = N.DeviceNet(N.init_muzero_params(1, C), C, device=dev)
    # root states: 40 plies of random play, then the games that have a legal move (repeated to fill the batch)
    env = E.env_reset(B, num_players=P, device=dev, **EV.RULES)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for _ in range(40):
        bits = E.legal_bits(env)
        live = env.done == 0
        mv = (live & (bits != 0)).nonzero().flatten()
        if mv.numel():
            sub = env.take(mv)
            E.env_step(sub, EV.random_legal(bits[mv], gen))
            env.put(mv, sub)
        ns = (live & (bits == 0)).nonzero().flatten()
        if ns.numel():
            sub = env.take(ns)
            E.no_step(sub)
            env.put(ns, sub)
    bits = E.legal_bits(env)
    ok = ((env.done == 0) & (bits != 0)).nonzero().flatten()
    pick = ok[torch.arange(B, device=dev) % ok.numel()]
    obs = E.encode_board(env.take(pick))
    bits = bits[pick].contiguous()
    ws = M.SearchWorkspace(B, S, dev)
    lg, v, e = N.root_inference_fn(net, obs, ws.scratch)
    print(f"shape: {P}p B={B} S={S} D={D}, random-init net, {int(ok.numel())} distinct root states, "
          f"{REPS} repetitions x {LAUNCHES} launches, interleaved", flush=True)

    def gumbel(turn):
        return M.gumbel_muzero_policy(net, lg, v, e, bits, S, D, 1.0, seed=5, turn=turn, workspace=ws)

    def puct(turn):
        return M.muzero_policy(net, lg, v, e, bits, S, D, 1.0, seed=5, turn=turn, workspace=ws)

    for t in range(3):     # warm-up
        gumbel(t)
        puct(t)
    torch.cuda.synchronize()
    ms = {"gumbel": [], "puct": []}
    for rep in range(REPS):
        for name, fn in (("gumbel", gumbel), ("puct", puct)):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(LAUNCHES + 1)]
            ev[0].record()
            for i in range(LAUNCHES):
                fn(100 * rep + i)
                ev[i + 1].record()
            torch.cuda.synchronize()
            per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(LAUNCHES))
            ms[name].append(per[LAUNCHES // 2])
            print(f"rep {rep} {name:6s}: median {per[LAUNCHES // 2]:.3f} ms per launch (min {per[0]:.3f}, "
                  f"max {per[-1]:.3f})", flush=True)
    g = sorted(ms["gumbel"])[REPS // 2]
    p = sorted(ms["puct"])[REPS // 2]
    sims = B * S / (p * 1e-3)
    tf = sims * FLOP_PER_SIM / 1e12
    gsims = B * S / (g * 1e-3)
    print(f"gumbel: {g:.3f} ms per search of the batch, {gsims / 1e6:.1f} M sims/s, "
          f"{gsims * FLOP_PER_SIM / 1e12 / PEAK_TFLOPS:.3f} of the fp32 MFMA peak")
    print(f"puct:   {p:.3f} ms per search of the batch, {sims / 1e6:.1f} M sims/s, {tf:.1f} TFLOP/s = "
          f"{tf / PEAK_TFLOPS:.3f} of the fp32 MFMA peak ({PEAK_TFLOPS} TFLOP/s)")
    print(f"ratio puct / gumbel: {p / g:.3f}")
    # how deep the two policies walk: the root's most visited child's share of the S visits
    pw = puct(0)[0].action_weights
    print(f"puct: mean largest visit share at the root {float(pw.max(1).values.mean()):.3f}, "
          f"mean root children visited {float((pw > 0).sum(1).float().mean()):.2f}")


def main():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                       timeout=300)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    if r.returncode == 0:
        with open(LOG, "w") as f:
            f.write(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else main())
