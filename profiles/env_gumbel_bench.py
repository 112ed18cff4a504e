"""muz_detmadn_gumbel_mcts (k_env_gumbel, the Gumbel network-free MCTS agent) measured beside muz_detmadn_mcts
(k_env_mcts, the PUCT one) in the same process: 2 players, B = 4096 mid-game root states (profiles/env_mcts_bench.py's),
S = 50, D = 25, rollouts of at most 300 turns, both qtransforms; 3 interleaved repetitions, HIP events, medians.  Then
how the agent plays: 256 games against random with each qtransform (tests/test_gpu_env_gumbel_strength.py's call), and
'gumbel_mcts_agent' against 'mcts_agent' head to head through evaluate_agent_parallel, both seatings (reported, not
asserted).

    python profiles/env_gumbel_bench.py [--parent-lib PATH]      # writes profiles/env_gumbel_bench.log

--parent-lib: a libmuz.so built from the parent commit.  k_env_mcts takes its model through a header it now shares
with k_env_gumbel; with the parent's library the same k_env_mcts measurement runs once more in a process of its own, so
the log holds both commits' figures from one session.

Every measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "env_gumbel_bench.log")
B, S, D, ROLLOUT, PLIES, REPS, LAUNCHES = 4096, 50, 25, 300, 60, 3, 5
GAMES, PLAY_S, PLAY_D, H2H_BATCH = 256, 16, 16, 64
QTS = ("completed_by_mix_value", "min_max")


def _modules(parent):
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import lib as L
    if parent:      # the parent's library has no muz_detmadn_gumbel_mcts to bind
        L.SIGNATURES.pop("muz_detmadn_gumbel_mcts")
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    return torch, E, EV, M


def timing(parent=False):
    torch, E, EV, M = _modules(parent)
    dev = torch.device("cuda")
    P = 2
    # root states: PLIES plies of random play (mid-game), then the games that have a legal move (repeated to fill)
    env = E.env_reset(B, num_players=P, device=dev, **EV.RULES)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for _ in range(PLIES):
        bits = E.legal_bits(env)
        live = env.done == 0
        EV._Det.advance(env, EV.random_legal(bits, gen), live, live & (bits != 0))
    bits = E.legal_bits(env)
    ok = ((env.done == 0) & (bits != 0)).nonzero().flatten()
    roots = env.take(ok[torch.arange(B, device=dev) % ok.numel()])
    ws = M.EnvSearchWorkspace(B, S, dev)
    who = "parent commit's library" if parent else "this commit"
    print(f"[{who}] shape: {P}p B={B} S={S} D={D} rollout_steps={ROLLOUT}, {int(ok.numel())} distinct root states "
          f"after {PLIES} plies of random play, {REPS} repetitions of {LAUNCHES} launches, interleaved", flush=True)

    def puct(turn, rollout_steps=ROLLOUT):
        return M.env_muzero_policy(roots, S, D, 0.0, rollout_steps=rollout_steps, seed=5, turn=turn, workspace=ws)

    def gumbel(qt):
        return lambda turn, rollout_steps=ROLLOUT: M.env_gumbel_muzero_policy(
            roots, S, D, 0.0, rollout_steps=rollout_steps, seed=5, turn=turn, workspace=ws, qtransform=qt)

    kinds = {"k_env_mcts": puct}
    if not parent:
        kinds.update({f"k_env_gumbel {qt}": gumbel(qt) for qt in QTS})

    def timed(fn, count):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        ev[0].record()
        for i in range(count):
            fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(count))
        return per[count // 2], per[0], per[-1]

    for fn in kinds.values():          # warm-up
        fn(0)
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    tree = {k: [] for k in kinds}
    turns = {k: [] for k in kinds}
    for rep in range(REPS):
        for name, fn in kinds.items():
            med, lo, hi = timed(lambda i: fn(100 * rep + i), LAUNCHES)
            ms[name].append(med)
            turns[name].append(int(ws.rollout_turns(B).long().sum()))        # of the repetition's last search
            tmed, _, _ = timed(lambda i: fn(100 * rep + i, 0), LAUNCHES)
            tree[name].append(tmed)
            print(f"rep {rep} {name:39s}: median {med:.2f} ms per batched search (min {lo:.2f}, max {hi:.2f}), "
                  f"{turns[name][-1]} rollout turns in the last one; {tmed:.2f} ms with rollout_steps = 0", flush=True)
    mid = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    base = mid(ms["k_env_mcts"])
    for name in kinds:
        s, t = mid(ms[name]), mid(turns[name])
        print(f"[{who}] {name}: {s:.3f} ms per batched search (spread {min(ms[name]):.3f}-{max(ms[name]):.3f} over "
              f"the repetitions), {B / (s * 1e-3) / 1e3:.1f} k searches/s, {B * S / (s * 1e-3) / 1e6:.2f} M "
              f"simulations/s, {t} rollout turns, {t / (s * 1e-3) / 1e6:.1f} M rollout env-steps/s; tree alone "
              f"{mid(tree[name]):.2f} ms; time over k_env_mcts's {s / base:.3f}")
    if not parent:
        for qt in QTS:
            pol, rv = gumbel(qt)(0)
            w = pol.action_weights
            print(f"k_env_gumbel {qt}: mean largest action weight {float(w.max(1).values.mean()):.3f}, mean root value "
                  f"{float(rv.mean()):+.3f}")


def strength():
    torch, E, EV, M = _modules(False)
    import time
    seat = EV._Det.gumbel_env_search

    def under(qt):      # the seat's search with another qtransform (the seat itself runs the default one)
        def search(sub, gid, S_, D_, temperature, seed, turn, mws, rollout_steps=EV.MCTS_ROLLOUT_STEPS):
            out, _ = M.env_gumbel_muzero_policy(sub, S_, D_, temperature, rollout_steps=rollout_steps, seed=seed,
                                                turn=turn, game_id=gid, workspace=mws, qtransform=qt)
            return out.action
        return staticmethod(search)

    def play(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = EV.play_vs_random(name, GAMES, num_players=2, num_simulations=PLAY_S, max_depth=PLAY_D, seed=42,
                              rollout_steps=ROLLOUT)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    print(f"against random: 2 players, {GAMES} games of play_vs_random, S={PLAY_S} D={PLAY_D} rollout_steps={ROLLOUT}, "
          f"seed 42 (the bar of the strength tests: 152)")
    for qt in QTS:
        EV._Det.gumbel_env_search = under(qt)
        r, dt = play("gumbel_mcts_agent")
        print(f"gumbel_mcts_agent {qt}: {r['wins']} of {GAMES} wins ({100.0 * r['wins'] / GAMES:.1f} %), "
              f"{r['finished']} finished, {dt:.1f} s", flush=True)
    EV._Det.gumbel_env_search = seat
    r, dt = play("mcts_agent")
    print(f"mcts_agent: {r['wins']} of {GAMES} wins ({100.0 * r['wins'] / GAMES:.1f} %), {r['finished']} finished, "
          f"{dt:.1f} s", flush=True)
    print(f"head to head: evaluate_agent_parallel, 4 players in teams (evaluate.RULES), {4 * H2H_BATCH} games per "
          f"seating, S={PLAY_S} D={PLAY_D}, temperature 0, rollouts of at most {EV.MCTS_ROLLOUT_STEPS} turns")
    g, m = "gumbel_mcts_agent", "mcts_agent"
    total = {g: 0, m: 0}
    for seats in ([g, m, g, m], [m, g, m, g]):
        r = EV.evaluate_agent_parallel(seats, batch_size=H2H_BATCH, num_simulations=PLAY_S, max_depth=PLAY_D,
                                       temperature=0.0, seed=7)
        wins = r["wins_per_player"]
        total[seats[0]] += wins[0]
        total[seats[1]] += wins[1]
        print(f"seats {seats}: wins per player {wins}, {r['finished']} of {r['games']} finished", flush=True)
    n = total[g] + total[m]
    print(f"head to head: gumbel_mcts_agent's team won {total[g]} of {n} finished games "
          f"({100.0 * total[g] / max(n, 1):.1f} %), mcts_agent's {total[m]}")


def main():
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    steps = [("--timing", {}, 300), ("--strength", {}, 600)]
    if parent:
        steps[1:1] = [("--timing-parent", {"MUZ_LIB": os.path.abspath(parent)}, 300), ("--timing", {}, 300)]
    out = []
    for flag, env, limit in steps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), flag], capture_output=True, text=True,
                           timeout=limit, env={**os.environ, **env})
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        sys.stdout.flush()
        if r.returncode != 0:
            return r.returncode
        out.append(r.stdout)
    with open(LOG, "w") as f:
        f.write("".join(out))
    return 0


if __name__ == "__main__":
    if "--timing" in sys.argv:
        sys.exit(timing())
    if "--timing-parent" in sys.argv:
        sys.exit(timing(parent=True))
    if "--strength" in sys.argv:
        sys.exit(strength())
    sys.exit(main())
