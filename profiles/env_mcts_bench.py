"""muz_detmadn_mcts (k_env_mcts, the network-free MCTS agent) measured: 2 players, B = 4096 mid-game root states,
S = 50, D = 25, rollouts of at most 300 turns; beside it the yardstick, uniform random play by k_det_round_g<32> at the
same batch (one launch per env-step of every game, with and without the observation encode), interleaved with the
search: 3 repetitions, HIP events, medians.  A rollout turn does that round's work (legal mask, pick, env_step or
no_step) plus the wins mask, and none of its launch, SoA load / store or encode.

    python profiles/env_mcts_bench.py [--parent-lib PATH]     # writes profiles/env_mcts_bench.log

--parent-lib: a libmuz.so built from the parent commit; the same measurement runs first through it, in a process of
its own (MUZ_LIB), so the log holds both commits' figures from one session.

The measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "env_mcts_bench.log")
B, S, D, ROLLOUT, PLIES, REPS, LAUNCHES, ROUNDS = 4096, 50, 25, 300, 60, 3, 5, 200
YARDSTICK_LOG = 193_954_240.3       # profiles/r3_env_variants.log: 4096 games, k_det_round_g<32>, encode included


def child():
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M

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
    in_goal = float((roots.pins_bp().long() >= 40).sum(dim=(1, 2)).float().mean())
    ws = M.EnvSearchWorkspace(B, S, dev)
    print(f"shape: {P}p B={B} S={S} D={D} rollout_steps={ROLLOUT}, {int(ok.numel())} distinct root states after "
          f"{PLIES} plies of random play ({in_goal:.2f} pins in goal per game), {REPS} repetitions, interleaved",
          flush=True)

    def search(turn, rollout_steps=ROLLOUT):
        return M.env_muzero_policy(roots, S, D, 0.0, rollout_steps=rollout_steps, seed=5, turn=turn, workspace=ws)

    renv = E.env_reset(B, num_players=P, device=dev, **EV.RULES)
    rbits = E.legal_bits(renv)
    obs = torch.empty((B, E.num_channels(P), 56), dtype=torch.int8, device=dev)

    def rounds(turn0, with_obs):
        for i in range(ROUNDS):
            E.random_round(renv, rbits, 9, turn0 + i, obs if with_obs else None, variant=2)

    def timed(fn, count):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        ev[0].record()
        for i in range(count):
            fn(i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(count))
        return per[count // 2], per[0], per[-1]

    search(0)                          # warm-up
    rounds(0, True)
    rounds(ROUNDS, False)
    torch.cuda.synchronize()
    ms = {"search": [], "tree": [], "round+obs": [], "round": []}
    turns = []
    for rep in range(REPS):
        med, lo, hi = timed(lambda i: search(100 * rep + i), LAUNCHES)
        ms["search"].append(med)
        turns.append(int(ws.rollout_turns(B).long().sum()))        # of the repetition's last search
        print(f"rep {rep} search   : median {med:.2f} ms per batched search (min {lo:.2f}, max {hi:.2f}), "
              f"{turns[-1]} rollout turns in the last one", flush=True)
        med, lo, hi = timed(lambda i: search(100 * rep + i, 0), LAUNCHES)
        ms["tree"].append(med)
        print(f"rep {rep} tree only: median {med:.2f} ms per batched search with rollout_steps = 0 (min {lo:.2f}, "
              f"max {hi:.2f})", flush=True)
        for name, with_obs in (("round+obs", True), ("round", False)):
            med, lo, hi = timed(lambda i: rounds(1000 * (rep + 1) + ROUNDS * i, with_obs), LAUNCHES)
            ms[name].append(med / ROUNDS)
            print(f"rep {rep} {name:9s}: median {1e3 * med / ROUNDS:.2f} us per round of {B} env-steps "
                  f"(min {1e3 * lo / ROUNDS:.2f}, max {1e3 * hi / ROUNDS:.2f})", flush=True)
    s = sorted(ms["search"])[REPS // 2]
    t = sorted(turns)[REPS // 2]
    rate = t / (s * 1e-3)
    tree = sorted(ms["tree"])[REPS // 2]
    per_game = t / B
    print(f"search: {s:.3f} ms per batched search, {B / (s * 1e-3) / 1e3:.1f} k searches/s, "
          f"{B * S / (s * 1e-3) / 1e6:.2f} M simulations/s")
    print(f"rollouts: {t} turns per batched search (counted on the device: {t / (B * (S + 1)):.1f} per rollout of at "
          f"most {ROLLOUT}), {rate / 1e6:.1f} M rollout env-steps/s (the search's whole time charged to them)")
    print(f"split: {tree:.2f} ms with rollout_steps = 0 (walks, transitions, masks, backups: {1e3 * tree / S:.1f} us "
          f"per simulation), so {s - tree:.2f} ms for the rollouts: {1e3 * (s - tree) / per_game:.2f} us per rollout "
          f"turn of a game's serial chain ({per_game:.0f} turns per game; a wave waits for the longer of its two "
          f"games' rollouts and the launch for its slowest wave)")
    for name in ("round+obs", "round"):
        r = B / (sorted(ms[name])[REPS // 2] * 1e-3)
        print(f"yardstick {name:9s}: {r / 1e6:.1f} M env-steps/s by k_det_round_g<32>, one launch per round; "
              f"rollout env-steps/s over it: {rate / r:.2f}")
    print(f"yardstick of profiles/r3_env_variants.log ({YARDSTICK_LOG / 1e6:.1f} M env-steps/s, encode included): "
          f"ratio {rate / YARDSTICK_LOG:.2f}")
    pol, rv = search(0)
    w = pol.action_weights
    print(f"search: mean largest visit share at the root {float(w.max(1).values.mean()):.3f}, mean root children "
          f"visited {float((w > 0).sum(1).float().mean()):.2f}, mean root value {float(rv.mean()):+.3f}")


if __name__ == "__main__":
    if "--child" in sys.argv:
        sys.exit(child())
    import _parent_lib
    sys.exit(_parent_lib.main(__file__, LOG, sys.argv))
