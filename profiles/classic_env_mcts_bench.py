"""muz_classic_mcts (k_classic_env_mcts, the network-free MCTS agent for classic MADN) measured: 4 players in teams
under the classic self-play rules, B = 4096 mid-game root states with their die thrown, S = 50, D = 25, rollouts of at
most 300 turns; beside it, in the same process and interleaved, k_env_mcts on det-MADN roots of the same batch and
search shape for scale (profiles/env_mcts_bench.py's workload): 3 repetitions, HIP events, medians.

    python profiles/classic_env_mcts_bench.py [--parent-lib PATH]     # writes profiles/classic_env_mcts_bench.log

--parent-lib: a libmuz.so built from the parent commit; the same measurement runs first through it, in a process of
its own (MUZ_LIB), so the log holds both commits' figures from one session.

The measuring step runs in a child process under its own time limit; this process never opens the GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "classic_env_mcts_bench.log")
B, S, D, ROLLOUT, PLIES, REPS, LAUNCHES = 4096, 50, 25, 300, 120, 3, 5


def child():
    import torch
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.load()
    from exploring_muzero_on_dog_amd import classic as CL
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import evaluate as EV
    from exploring_muzero_on_dog_amd import mcts as M
    from exploring_muzero_on_dog_amd import stochastic as ST

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    # classic roots: PLIES turns of random play (the die thrown every turn), one more throw, then the games that have
    # a legal pin for it (repeated to fill)
    env = CL.env_reset(B, num_players=4, device=dev, **CL.SELFPLAY_RULES)
    for turn in range(PLIES + 1):
        CL.throw_die(env, torch.rand((B,), generator=gen, device=dev))
        bits = CL.legal_bits(env)
        if turn == PLIES:
            break
        live = env.done == 0
        act = EV.classic_policy_action(env, bits, "random_agent", 3, turn)
        EV._Classic.advance(env, act, live, live & ((bits & 15) != 0))
    ok = ((env.done == 0) & ((bits & 15) != 0)).nonzero().flatten()
    roots = env.take(ok[torch.arange(B, device=dev) % ok.numel()])
    in_goal = float((roots.pins.long() >= 40).sum(dim=0).float().mean())
    ws = ST.ClassicEnvSearchWorkspace(B, S, dev)
    print(f"shape: classic 4p teams (SELFPLAY_RULES) B={B} S={S} D={D} rollout_steps={ROLLOUT}, {int(ok.numel())} "
          f"distinct root states after {PLIES} turns of random play ({in_goal:.2f} pins in goal per game), {REPS} "
          f"repetitions, interleaved with k_env_mcts on det-MADN roots", flush=True)

    # det roots, as profiles/env_mcts_bench.py makes them
    denv = E.env_reset(B, num_players=2, device=dev, **EV.RULES)
    for _ in range(60):
        dbits = E.legal_bits(denv)
        live = denv.done == 0
        EV._Det.advance(denv, EV.random_legal(dbits, gen), live, live & (dbits != 0))
    dbits = E.legal_bits(denv)
    dok = ((denv.done == 0) & (dbits != 0)).nonzero().flatten()
    droots = denv.take(dok[torch.arange(B, device=dev) % dok.numel()])
    dws = M.EnvSearchWorkspace(B, S, dev)

    def search(turn, rollout_steps=ROLLOUT):
        return ST.env_stochastic_muzero_policy(roots, S, D, 0.0, rollout_steps=rollout_steps, seed=5, turn=turn,
                                               workspace=ws)

    def det_search(turn):
        return M.env_muzero_policy(droots, S, D, 0.0, rollout_steps=ROLLOUT, seed=5, turn=turn, workspace=dws)

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
    det_search(0)
    torch.cuda.synchronize()
    ms = {"search": [], "tree": [], "det": []}
    turns, dturns = [], []
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
        med, lo, hi = timed(lambda i: det_search(100 * rep + i), LAUNCHES)
        ms["det"].append(med)
        dturns.append(int(dws.rollout_turns(B).long().sum()))
        print(f"rep {rep} det      : median {med:.2f} ms per batched k_env_mcts search (min {lo:.2f}, max {hi:.2f}), "
              f"{dturns[-1]} rollout turns in the last one", flush=True)
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
          f"turn of a game's serial chain ({per_game:.0f} turns per game, played by one lane of the game's 32)")
    d = sorted(ms["det"])[REPS // 2]
    dt = sorted(dturns)[REPS // 2]
    print(f"for scale, k_env_mcts on {int(dok.numel())} distinct det-MADN 2p roots, same B / S / D / cap: {d:.2f} ms per "
          f"batched search, {B / (d * 1e-3) / 1e3:.1f} k searches/s, {B * S / (d * 1e-3) / 1e6:.2f} M simulations/s, "
          f"{dt} rollout turns, {dt / (d * 1e-3) / 1e6:.1f} M rollout env-steps/s; classic / det time per search "
          f"{s / d:.2f}, rollout env-steps/s {rate / (dt / (d * 1e-3)):.2f}")
    pol, rv = search(0)
    w = pol.action_weights
    print(f"search: mean largest visit share at the root {float(w.max(1).values.mean()):.3f}, mean root children "
          f"visited {float((w > 0).sum(1).float().mean()):.2f}, mean root value {float(rv.mean()):+.3f}")


if __name__ == "__main__":
    if "--child" in sys.argv:
        sys.exit(child())
    import _parent_lib
    sys.exit(_parent_lib.main(__file__, LOG, sys.argv))
