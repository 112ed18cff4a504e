"""k_gumbel_search's forms of MUZ_SELECT_INVARIANTS (csrc/search.hip) beside each other at the kernel: 2 players,
B = 4096, S = 50, D = 25, a randomly initialised net, root states from 40 plies of random play (real legal masks); the
forms interleaved, 3 repetitions of 16 launches each, HIP events, the median of each repetition.

    python profiles/select_invariants_bench.py 0,1,2        # MUZ_LIB=... for another build
    python profiles/select_invariants_bench.py 0,1 MUZ_RING_ADDR   # the same for another per-launch switch

The switch is read per launch, so one process measures every form of one build."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, S, D, REPS, LAUNCHES = 4096, 50, 25, 3, 16
import torch  # noqa: E402
import muzpkg  # noqa: E402

muzpkg.load()
from exploring_muzero_on_dog_amd import detmadn as E  # noqa: E402
from exploring_muzero_on_dog_amd import evaluate as EV  # noqa: E402
from exploring_muzero_on_dog_amd import mcts as M  # noqa: E402
from exploring_muzero_on_dog_amd import nets as N  # noqa: E402

forms = sys.argv[1].split(",")
SWITCH = sys.argv[2] if len(sys.argv) > 2 else "MUZ_SELECT_INVARIANTS"
dev = torch.device("cuda")
P = 2
C = E.num_channels(P)
net = N.DeviceNet(N.init_muzero_params(1, C), C, device=dev)
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
nl = torch.tensor([bin(int(b) & 0xFFFFFF).count("1") for b in bits.cpu()], dtype=torch.float32)
print(f"lib {os.environ.get('MUZ_LIB', 'in-tree')}, {SWITCH}: mean legal actions {float(nl.mean()):.2f}", flush=True)


def run(form, turn):
    os.environ[SWITCH] = form
    return M.gumbel_muzero_policy(net, lg, v, e, bits, S, D, 1.0, seed=5, turn=turn, workspace=ws)


for f in forms:
    for t in range(2):
        run(f, t)
torch.cuda.synchronize()
ms = {f: [] for f in forms}
for rep in range(REPS):
    for f in forms:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(LAUNCHES + 1)]
        ev[0].record()
        for i in range(LAUNCHES):
            run(f, 100 * rep + i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(LAUNCHES))
        ms[f].append(per[LAUNCHES // 2])
for f in forms:
    print(f"  form {f}: median ms per launch " + " ".join(f"{x:.4f}" for x in ms[f]), flush=True)
