"""Where dog.greedy_policy's time goes on the 1024 roots of profiles/dog_greedy_bench.py: the whole batch, the largest
root alone, batches of roots with a capped number of play-phase candidates, and 1024 copies of the largest root.  HIP
events, 5 repetitions of 20 calls, medians.

    python profiles/dog_greedy_split.py > profiles/dog_greedy_split.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import muzpkg  # noqa: E402

muzpkg.load()
from exploring_muzero_on_dog_amd import dog as D  # noqa: E402

B = 1024
dev = torch.device("cuda")
rp = D.RandomPlay(B, seed=3)
rp.play(150)
env = rp.env
nleg = D.valid_actions(env).sum(dim=1)
ok = ((env.done == 0) & (nleg >= 2)).nonzero().flatten()
roots = env.take(ok[torch.arange(B, device=dev) % ok.numel()])
nleg = D.valid_actions(roots)[:, :792].sum(dim=1)


def timed(st, count=20, reps=5):
    D.greedy_policy(st, seed=5, turn=0)
    torch.cuda.synchronize()
    meds = []
    for rep in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        ev[0].record()
        for i in range(count):
            D.greedy_policy(st, seed=5, turn=i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(count))
        meds.append(per[count // 2])
    return 1e3 * sorted(meds)[reps // 2]


big = int(nleg.argmax())
print(f"whole batch ({int(nleg.sum())} stepped, max {int(nleg.max())}): {timed(roots):.1f} us")
print(f"the largest root alone (1 game, {int(nleg[big])} stepped): {timed(roots.take(torch.tensor([big], device=dev))):.1f} us")
for cap in (0, 8, 16, 32, 64):
    idx = (nleg <= cap).nonzero().flatten()
    sub = roots.take(idx[torch.arange(B, device=dev) % idx.numel()])
    n = D.valid_actions(sub)[:, :792].sum(dim=1)
    print(f"1024 roots with at most {cap} stepped candidates ({int(n.sum())} stepped, max {int(n.max())}): "
          f"{timed(sub):.1f} us")
one = roots.take(torch.full((B,), big, device=dev))
print(f"1024 copies of the largest root ({B * int(nleg[big])} stepped): {timed(one):.1f} us")
