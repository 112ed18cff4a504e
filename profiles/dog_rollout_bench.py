"""muz_dog_rollout_search (the network-free rollout agent for DOG, csrc/dog_rollout.hip) measured: 4 players in teams
under the DOG self-play rules, B = 1024 mid-game roots, the defaults (4 rollouts per action and phase, at most 10
phases, rollouts of at most 300 turns, determinized); beside it, in the same process, k_dog_play's random-play rate at
1024 games (bench.py's dog workload: one launch of 1024 turns with auto reset).  3 repetitions, HIP events, medians.

    python profiles/dog_rollout_bench.py            # writes profiles/dog_rollout_bench.log

The measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "dog_rollout_bench.log")
B, PLIES, REPS, LAUNCHES, PLAY_TURNS = 1024, 150, 3, 3, 1024


def child():
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import dog as D

    dev = torch.device("cuda")
    # roots: PLIES turns of random play from the reset, then the unfinished games with at least two legal actions
    # (repeated to fill)
    rp = D.RandomPlay(B, seed=3)
    rp.play(PLIES)
    env = rp.env
    nleg = D.valid_actions(env).sum(dim=1)
    ok = ((env.done == 0) & (nleg >= 2)).nonzero().flatten()
    roots = env.take(ok[torch.arange(B, device=dev) % ok.numel()])
    nleg = D.valid_actions(roots).sum(dim=1).float()
    in_goal = float((roots.pins.long() >= 40).sum(dim=0).float().mean())
    ws = D.RolloutWorkspace(B, dev)
    print(f"shape: DOG 4p teams (SELFPLAY_RULES) B={B}, defaults (rollouts 4, max_phases 10, rollout_steps 300, "
          f"determinize), {int(ok.numel())} distinct roots after {PLIES} turns of random play ({in_goal:.2f} pins in "
          f"goal per game, {float(nleg.mean()):.1f} legal actions per root, max {int(nleg.max())}), {REPS} repetitions",
          flush=True)

    def search(turn, **kw):
        return D.rollout_policy(roots, seed=5, turn=turn, workspace=ws, summary=True, **kw)

    def timed(fn, count):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        ev[0].record()
        out = None
        for i in range(count):
            out = fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(count))
        return per[count // 2], per[0], per[-1], out

    search(0)
    torch.cuda.synchronize()
    ms, rolls, steps = [], [], []
    for rep in range(REPS):
        med, lo, hi, out = timed(lambda i: search(100 * rep + i), LAUNCHES)
        _, value, visits, wins, turns = out
        ms.append(med)
        rolls.append(int(visits.long().sum()))
        steps.append(int(turns.long().sum()) + rolls[-1])        # random turns + the root action of every rollout
        print(f"rep {rep} search: median {med:.2f} ms per batched search (min {lo:.2f}, max {hi:.2f}), {rolls[-1]} "
              f"rollouts and {steps[-1]} env-steps in the last one", flush=True)
    s, r, t = sorted(ms)[REPS // 2], sorted(rolls)[REPS // 2], sorted(steps)[REPS // 2]
    rate = t / (s * 1e-3)
    print(f"search: {s:.2f} ms per batched search of {B} roots ({1e3 * s / B:.1f} us per root), "
          f"{r / (s * 1e-3) / 1e6:.3f} M rollouts/s, {rate / 1e6:.1f} M rollout env-steps/s ({t / r:.1f} env-steps per "
          f"rollout of at most 301)")
    # where the time goes: the same search cut after 1, 2, .. phases (a phase's time against its rollouts), and with a
    # cap of 1 turn (the launches, item loads, determinizations and root actions without the playouts)
    prev_ms, prev_r = 0.0, 0
    for ph in (1, 2, 3, 4, 5, 6, 8, 10):
        m, _, _, o = timed(lambda i: search(500 + 10 * ph + i, max_phases=ph), LAUNCHES)
        n = int(o[2].long().sum())
        print(f"split: max_phases = {ph:2d}: {m:6.2f} ms, {n} rollouts (+{m - prev_ms:.2f} ms for +{n - prev_r} "
              f"rollouts: {1e3 * (m - prev_ms) / max(n - prev_r, 1):.2f} us per added rollout)")
        prev_ms, prev_r = m, n
    cap1, _, _, outc = timed(lambda i: search(900 + i, rollout_steps=1), LAUNCHES)
    print(f"split: {cap1:.2f} ms with rollout_steps = 1 ({int(outc[2].long().sum())} rollouts: the 31 launches, item "
          f"loads, determinizations and root actions)")

    # k_dog_play's random-play rate, bench.py's dog workload
    play = D.RandomPlay(B, seed=1)
    env_steps = torch.zeros((B,), dtype=torch.int32, device=dev)
    play.play(PLAY_TURNS, env_steps=env_steps, auto_reset=True)
    torch.cuda.synchronize()
    rates = []
    for rep in range(REPS):
        env_steps.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        play.play(PLAY_TURNS, env_steps=env_steps, auto_reset=True)
        e1.record()
        torch.cuda.synchronize()
        rates.append(int(env_steps.long().sum()) / (e0.elapsed_time(e1) * 1e-3))
    pr = sorted(rates)[REPS // 2]
    print(f"k_dog_play: {pr / 1e6:.1f} M env-steps/s at {B} games ({PLAY_TURNS} turns per launch, auto reset; "
          f"{1e6 * B / pr:.2f} us per game-turn)")
    print(f"ratio: rollout env-steps/s / k_dog_play env-steps/s = {rate / pr:.2f}")


def main():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                       timeout=420)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    if r.returncode == 0:
        with open(LOG, "w") as f:
            f.write(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else main())
