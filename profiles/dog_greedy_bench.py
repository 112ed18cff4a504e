"""muz_dog_greedy_action (the one-ply greedy agent for DOG, csrc/dog_greedy.hip) measured: 4 players in teams under the
DOG self-play rules, B = 1024 mid-game roots (those of profiles/dog_rollout_bench.py), the defaults
(dog.GREEDY_DEFAULTS); beside it, in the same process, a muz_dog_legal launch on the same roots (the floor: the root
load and the legality checks the greedy kernel also runs) and dog.rollout_policy with its defaults.  HIP events,
medians.  The one requirement: a greedy call is cheaper than a rollout search.  Then the two agents head to head:
evaluate_agent_parallel_dog with ["greedy_agent", "rollout_agent"] * 2 and the swapped seating, 256 games each; the
wins are reported, nothing is asserted about them.

    python profiles/dog_greedy_bench.py            # writes profiles/dog_greedy_bench.log

The measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "dog_greedy_bench.log")
B, PLIES, REPS, LAUNCHES, GAMES = 1024, 150, 5, 20, 256


def child():
    import time

    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import dog as D
    from exploring_muzero_on_dog_amd import evaluate as EV

    dev = torch.device("cuda")
    # roots: PLIES turns of random play from the reset, then the unfinished games with at least two legal actions
    # (repeated to fill)
    rp = D.RandomPlay(B, seed=3)
    rp.play(PLIES)
    env = rp.env
    nleg = D.valid_actions(env).sum(dim=1)
    ok = ((env.done == 0) & (nleg >= 2)).nonzero().flatten()
    roots = env.take(ok[torch.arange(B, device=dev) % ok.numel()])
    legal = D.valid_actions(roots)
    nleg = legal.sum(dim=1).float()
    stepped = int(legal[:, :D.PLAY_ACTIONS].sum())          # swap-phase candidates are scored without a step
    print(f"shape: DOG 4p teams (SELFPLAY_RULES) B={B}, defaults {D.GREEDY_DEFAULTS}, {int(ok.numel())} distinct roots "
          f"after {PLIES} turns of random play ({float(nleg.mean()):.1f} legal actions per root, max {int(nleg.max())}; "
          f"{stepped} candidates stepped per call, {int((roots.phase != 0).sum())} roots in the swap phase), "
          f"{REPS} repetitions of {LAUNCHES} calls", flush=True)

    def timed(fn, count):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        ev[0].record()
        for i in range(count):
            fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(count))
        return per[count // 2], per[0], per[-1]

    def median_of(fn, count, what):
        fn(0)
        torch.cuda.synchronize()
        meds = []
        for rep in range(REPS):
            med, lo, hi = timed(lambda i: fn(100 * rep + i), count)
            meds.append(med)
            print(f"rep {rep} {what}: median {1e3 * med:.1f} us per call (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})",
                  flush=True)
        return sorted(meds)[REPS // 2]

    mask = torch.empty((B, D.MASK_WORDS), dtype=torch.int32, device=dev)
    g_ms = median_of(lambda t: D.greedy_policy(roots, seed=5, turn=t), LAUNCHES, "greedy_policy")
    s_ms = median_of(lambda t: D.greedy_policy(roots, seed=5, turn=t, summary=True), LAUNCHES,
                     "greedy_policy(summary)")
    l_ms = median_of(lambda t: D.legal_mask(roots, out=mask), LAUNCHES, "muz_dog_legal")
    ws = D.RolloutWorkspace(B, dev)
    r_ms = median_of(lambda t: D.rollout_policy(roots, seed=5, turn=t, workspace=ws), 3, "rollout_policy")
    print(f"greedy: {1e3 * g_ms:.1f} us per greedy_policy call of {B} roots ({1e3 * g_ms / B:.3f} us per root), "
          f"{stepped} candidates stepped per call, {stepped / (g_ms * 1e-3) / 1e6:.1f} M candidates/s; with the "
          f"scores and features written (summary): {1e3 * s_ms:.1f} us")
    print(f"floor: {1e3 * l_ms:.1f} us per muz_dog_legal launch on the same roots (greedy / legal = {g_ms / l_ms:.2f})")
    print(f"rollout: {r_ms:.2f} ms per rollout_policy call with its defaults (rollout / greedy = {r_ms / g_ms:.0f})")
    assert g_ms < r_ms, "a greedy call must be cheaper than a rollout search"

    # head to head, both seatings; reported, not judged
    for seats in (["greedy_agent", "rollout_agent"] * 2, ["rollout_agent", "greedy_agent"] * 2):
        t0 = time.perf_counter()
        r = EV.evaluate_agent_parallel_dog(seats, batch_size=GAMES // 4, seed=42)
        torch.cuda.synchronize()
        w = r["wins_per_player"]
        g = seats.index("greedy_agent")
        print(f"head to head: seats {seats}: greedy_agent {w[g]} wins, rollout_agent {w[1 - g]} wins of {GAMES} games "
              f"({r['finished']} finished in {r['turns']} turns, {time.perf_counter() - t0:.1f} s)", flush=True)


def main():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                       timeout=540)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    if r.returncode == 0:
        with open(LOG, "w") as f:
            f.write(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else main())
