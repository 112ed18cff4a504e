"""muz_dog_guided_rollout_search (the DOG rollout agent with greedy-guided playouts, csrc/dog_guided.hip) measured
against muz_dog_rollout_search in the same process on the same roots: profiles/dog_rollout_bench.py's 1024 mid-game
roots (4 players in teams under the DOG self-play rules, 150 turns of random play), the defaults (4 rollouts per action
and phase, at most 10 phases, rollouts of at most 300 turns, determinized, epsilon 0.125, the greedy agent's default
weights).  3 repetitions of 3 searches, HIP events, medians.  No throughput number is fixed in advance: the base is
rollout_policy here.  The decided share of rollout_policy is read from guided_rollout_policy at epsilon 1, which is
rollout_policy output for output (tests/test_gpu_dog_guided.py).

Then the agents head to head, reported, not judged: evaluate_agent_parallel_dog, 256 games a seating, both seatings,
'guided_rollout_agent' at epsilon 0, 0.125 and 0.5 against 'greedy_agent' and against 'rollout_agent'.

    python profiles/dog_guided_bench.py              # writes profiles/dog_guided_bench.log
    python profiles/dog_guided_bench.py vs_greedy    # writes profiles/dog_guided_vs_greedy.log
    python profiles/dog_guided_bench.py vs_rollout   # writes profiles/dog_guided_vs_rollout.log

Each measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = {"bench": "dog_guided_bench.log", "vs_greedy": "dog_guided_vs_greedy.log",
        "vs_rollout": "dog_guided_vs_rollout.log"}
LIMITS = {"bench": 420, "vs_greedy": 1080, "vs_rollout": 1080}
B, PLIES, REPS, LAUNCHES = 1024, 150, 3, 3
GAMES = 256
EPSILONS = (0.0, 0.125, 0.5)


def _load():
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()


def bench():
    import torch
    _load()
    from exploring_muzero_on_dog_amd import dog as D

    dev = torch.device("cuda")
    rp = D.RandomPlay(B, seed=3)          # profiles/dog_rollout_bench.py's roots
    rp.play(PLIES)
    env = rp.env
    nleg = D.valid_actions(env).sum(dim=1)
    ok = ((env.done == 0) & (nleg >= 2)).nonzero().flatten()
    roots = env.take(ok[torch.arange(B, device=dev) % ok.numel()])
    nleg = D.valid_actions(roots).sum(dim=1).float()
    ws = D.RolloutWorkspace(B, dev)
    print(f"shape: DOG 4p teams (SELFPLAY_RULES) B={B}, defaults (rollouts 4, max_phases 10, rollout_steps 300, "
          f"determinize; guided: epsilon 0.125, GREEDY_DEFAULTS' weights), {int(ok.numel())} distinct roots after "
          f"{PLIES} turns of random play ({float(nleg.mean()):.1f} legal actions per root, max {int(nleg.max())}), "
          f"{REPS} repetitions of {LAUNCHES} searches", flush=True)

    def timed(fn, count):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        ev[0].record()
        out = None
        for i in range(count):
            out = fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(count))
        return per[count // 2], out

    def measure(name, search):
        """-> (ms per search, playout turns per search) as medians over the repetitions."""
        search(0)
        torch.cuda.synchronize()
        rows = []
        for rep in range(REPS):
            med, out = timed(lambda i: search(100 * rep + i), LAUNCHES)
            visits, turns = int(out[2].long().sum()), int(out[4].long().sum())
            decided = int(out[5].long().sum()) if len(out) > 5 else None
            rows.append((med, visits, turns, decided))
        med, visits, turns, decided = sorted(rows)[REPS // 2]
        steps = turns + visits                                     # playout turns + the root action of every rollout
        share = "" if decided is None else f", decided {decided} of {visits} rollouts = {100.0 * decided / visits:.1f} %"
        print(f"{name}: {med:.2f} ms per batched search of {B} roots ({1e3 * med / B:.1f} us per root), {visits} "
              f"rollouts = {visits / (med * 1e-3) / 1e6:.3f} M rollouts/s, {steps / (med * 1e-3) / 1e6:.1f} M rollout "
              f"env-steps/s, {turns / visits:.1f} playout turns per rollout (cap 300){share}", flush=True)
        return med, turns

    def guided(eps):
        return lambda turn: D.guided_rollout_policy(roots, seed=5, turn=turn, workspace=ws, summary=True, epsilon=eps)

    base_ms, base_turns = measure("rollout_policy", lambda turn: D.rollout_policy(roots, seed=5, turn=turn,
                                                                                  workspace=ws, summary=True))
    one_ms, one_turns = measure("guided_rollout_policy epsilon 1 (= rollout_policy, with its decided count)", guided(1.0))
    print(f"ratio: the guided kernel at epsilon 1 / rollout_policy = {one_ms / base_ms:.3f} in ms per search (the same "
          f"playouts: {one_turns} against {base_turns} playout turns)", flush=True)
    for eps in (0.125, 0.0, 0.5):
        ms, turns = measure(f"guided_rollout_policy epsilon {eps:g}" + (" (the default)" if eps == 0.125 else ""),
                            guided(eps))
        print(f"ratio: epsilon {eps:g}: {ms / base_ms:.2f}x rollout_policy's ms per search, "
              f"{(ms / turns) / (base_ms / base_turns):.2f}x its time per playout turn ({1e6 * ms / turns:.2f} ns "
              f"against {1e6 * base_ms / base_turns:.2f} ns per playout turn of the batch)", flush=True)
    cap1, out = timed(lambda i: D.guided_rollout_policy(roots, seed=5, turn=900 + i, workspace=ws, summary=True,
                                                        rollout_steps=1), LAUNCHES)
    print(f"split: {cap1:.2f} ms with rollout_steps = 1 ({int(out[2].long().sum())} rollouts: the 31 launches and the "
          f"memset, item loads, determinizations, root actions and one playout turn)", flush=True)


def head_to_head(opponent):
    import torch
    _load()
    from exploring_muzero_on_dog_amd import evaluate as EV

    print(f"head to head: evaluate_agent_parallel_dog, {GAMES} games a seating under evaluate.DOG_RULES (teams), seed "
          f"42, the defaults otherwise (rollouts 4, rollout_steps 300, determinize; greedy_agent: GREEDY_DEFAULTS); "
          f"reported, not judged", flush=True)
    for eps in EPSILONS:
        for g in (0, 1):
            seats = ["guided_rollout_agent", opponent] * 2 if g == 0 else [opponent, "guided_rollout_agent"] * 2
            t0 = time.perf_counter()
            r = EV.evaluate_agent_parallel_dog(seats, batch_size=GAMES // 4, seed=42, guided=dict(epsilon=eps))
            torch.cuda.synchronize()
            w = r["wins_per_player"]
            print(f"head to head: epsilon {eps:g}, guided_rollout_agent at seats {g} + {g + 2}: guided_rollout_agent "
                  f"{w[g]} wins, {opponent} {w[1 - g]} wins of {GAMES} games ({r['finished']} finished in "
                  f"{r['turns']} turns, {time.perf_counter() - t0:.1f} s)", flush=True)


def main(part):
    """Run ``part`` in a child that is ended at its time limit, echoing its lines as they come; the log is written on
    success."""
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", part], stdout=subprocess.PIPE,
                         text=True)
    late = []
    timer = threading.Timer(LIMITS[part], lambda: (late.append(True), p.kill()))
    timer.start()
    lines = []
    for line in p.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
        lines.append(line)
    rc = p.wait()
    timer.cancel()
    if late:
        print(f"{part}: over its limit of {LIMITS[part]} s, ended", file=sys.stderr)
        return 124
    if rc == 0:
        with open(os.path.join(ROOT, "profiles", LOGS[part]), "w") as f:
            f.writelines(lines)
    return rc


if __name__ == "__main__":
    if "--child" in sys.argv:
        part = sys.argv[-1]
        sys.exit(bench() if part == "bench" else head_to_head({"vs_greedy": "greedy_agent",
                                                               "vs_rollout": "rollout_agent"}[part]))
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "bench"))
