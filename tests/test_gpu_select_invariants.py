"""k_gumbel_search's select-phase invariants (csrc/search.hip, template argument PARTS): the root's prior softmax and
largest prior kept in registers and the considered-visit sequence tabulated per game in LDS (the default form), and with
MUZ_SELECT_INVARIANTS=2 also every node's prior softmax, evaluated once at its expansion and kept in the tree's pad
slots.  Only where and how often an expression is evaluated differs from the form MUZ_SELECT_INVARIANTS=0 selects, so
every output of both is bit for bit that form's; the default form is also held against the NumPy restatement of mctx
(oracle/mctx_gumbel.py) through tests/_parity.py.

Shapes: n in {1, 15, 16, 17, 33} (a partial tile, a full one, a second tile), S in {1, 2, 17, 50}, D in {1, 3, 25},
max_num_considered in {1, 2, 16}.  Rows (_rows below): legal masks with one action, all 24 and alternating bits; rows of
all-equal logits (ties everywhere); rows with one logit 80 above the rest (every other exp(prior - max) is ~1.8e-35)
and 120 above (it is 0: the clamp at the smallest normal float engages for legal actions, not only masked ones).  No
row without a legal action: the existing search tests pass none to this entry.  The workspace is filled with 0xFF bytes
before every search, so a walk that read a word no expansion had written would meet a NaN."""
import numpy as np
import pytest
import torch

from oracle import mctx_gumbel as G
from tests._parity import search_parity
from tests import test_gpu_search as TS

pytestmark = pytest.mark.gpu

NMAX = 33
ALL, EVEN, ODD = 0xFFFFFF, 0x555555, 0xAAAAAA


def _rows():
    """legal bits [NMAX] and the rows whose root logits are replaced: row -> ('flat',) or ('peak', action, height)."""
    bits = np.zeros(NMAX, np.int64)
    for i in range(NMAX):
        bits[i] = (ALL, EVEN if i % 2 else ODD, 1 << ((7 * i) % 24))[i % 3]
    special = {0: ("flat",), 1: ("peak", 2, 80.0), 3: ("peak", 5, 80.0), 6: ("peak", 7, 120.0), 4: ("flat",),
               9: ("flat",), 10: ("peak", 1, 120.0), 12: ("peak", 23, 80.0)}
    for i, s in special.items():     # a peak sits on a legal action
        assert s[0] == "flat" or (bits[i] >> s[1]) & 1, i
    return bits.astype(np.int32), special


_CTX = {}


def _ctx():
    """Network, NMAX roots (the GPU's own root inference) with the special rows' logits, Gumbel noise: computed once."""
    if not _CTX:
        N, M, params, net, obs, valid, _ = TS.setup(2, 48, 7, "selfplay_2p")
        assert obs.shape[0] >= NMAX
        lg, v, e = N.root_inference_fn(net, torch.from_numpy(obs[:NMAX]).cuda())
        bits, special = _rows()
        lg = lg.clone()
        for i, s in special.items():
            if s[0] == "flat":
                lg[i] = 0.25
            else:
                lg[i, s[1]] = lg[i].max() + s[2]
        gum = np.random.default_rng(11).gumbel(size=(NMAX, 24)).astype(np.float32)
        _CTX.update(N=N, M=M, params=params, net=net, lg=lg, v=v, e=e, bits=bits, gum=gum)
    return _CTX


def _search(c, rows, S, D, mnc):
    """muz_gumbel_search on the given rows: (action, weights, root value) as NumPy arrays."""
    from exploring_muzero_on_dog_amd import lib as L
    M, net = c["M"], c["net"]
    so = L.load()
    idx = torch.as_tensor(rows, device="cuda")
    lg, v, e = (c[k].index_select(0, idx).contiguous() for k in ("lg", "v", "e"))
    lb = torch.from_numpy(c["bits"][rows]).cuda()
    gum = torch.from_numpy(c["gum"][rows]).cuda()
    n = len(rows)
    ws = M.SearchWorkspace(n, S)
    ws.tree.fill_(0xFF)
    cfg = M.make_cfg(S, D, 1.0, max_num_considered=mnc)
    action = torch.empty((n,), dtype=torch.int32, device="cuda")
    weights = torch.empty((n, 24), dtype=torch.float32, device="cuda")
    value = torch.empty((n,), dtype=torch.float32, device="cuda")
    L.check(so.muz_gumbel_search(net.w, cfg, L.ptr(lg), L.ptr(v), L.ptr(e), L.ptr(lb), L.ptr(gum), L.ptr(None), n,
                                 L.ptr(ws.tree), L.nbytes(ws.tree), L.ptr(action), L.ptr(weights), L.ptr(value),
                                 L.stream_ptr()), "muz_gumbel_search")
    torch.cuda.synchronize()
    return action.cpu().numpy(), weights.cpu().numpy(), value.cpu().numpy()


def _row_sets(n):
    """Rows 0..n-1; a single game takes each of the first rows in turn (every mask kind, ties, both peaks)."""
    return [[i] for i in range(7)] if n == 1 else [list(range(n))]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_outputs_bit_identical_to_per_level_form(cuda, monkeypatch, n):
    c = _ctx()
    for rows in _row_sets(n):
        for S in (1, 2, 17, 50):
            for D in (1, 3, 25):
                for mnc in (1, 2, 16):
                    monkeypatch.setenv("MUZ_SELECT_INVARIANTS", "0")
                    want = _search(c, rows, S, D, mnc)
                    for form in (None, "2"):
                        if form is None:
                            monkeypatch.delenv("MUZ_SELECT_INVARIANTS")
                        else:
                            monkeypatch.setenv("MUZ_SELECT_INVARIANTS", form)
                        got = _search(c, rows, S, D, mnc)
                        for name, g, w in zip(("action", "action_weights", "root_value_out"), got, want):
                            same = np.array_equal(g.view(np.int32), w.view(np.int32))
                            assert same, (name, form, rows[0], n, S, D, mnc)
                    legal = (c["bits"][rows][:, None] >> np.arange(24)) & 1
                    assert legal[np.arange(len(rows)), got[0]].all(), ("illegal action", rows[0], n, S, D, mnc)


# every n, S, D and max_num_considered above at least once
ORACLE_CASES = [(33, 50, 25, 16), (33, 17, 3, 2), (17, 50, 3, 1), (16, 2, 1, 2), (15, 1, 25, 16), (1, 17, 25, 2)]


@pytest.mark.parametrize("n,S,D,mnc", ORACLE_CASES)
def test_default_form_matches_mctx_restatement(cuda, monkeypatch, n, S, D, mnc):
    c = _ctx()
    monkeypatch.delenv("MUZ_SELECT_INVARIANTS", raising=False)
    # the restatement's simulate() leaves root_action_selection's max_num_considered at its default of 16 whatever
    # table it was given; pass the case's value through (16: unchanged)
    orig = G.root_action_selection
    monkeypatch.setattr(G, "root_action_selection", lambda *a, **k: orig(*a, max_num_considered=mnc, **k))
    for rows in _row_sets(n)[:3]:
        ga, gw, grv = _search(c, rows, S, D, mnc)
        idx = torch.as_tensor(rows, device="cuda")
        lg, v, e = (c[k].index_select(0, idx).cpu().numpy() for k in ("lg", "v", "e"))
        invalid = ((c["bits"][rows][:, None] >> np.arange(24)) & 1) == 0
        trace = {}
        with np.errstate(over="ignore", invalid="ignore"):
            a, w, orv, _ = G.gumbel_muzero_policy(c["params"], lg, v, e, TS.gpu_recurrent_fn(c["N"], c["net"]), S,
                                                  invalid, c["gum"][rows], max_depth=D,
                                                  max_num_considered_actions=mnc, trace=trace)
        search_parity(f"select invariants n{n} row{rows[0]} S{S} D{D} m{mnc}", ga, gw, grv, a, w, orv, trace["margin"],
                      trace["gain"])
        # both sides see the same network outputs and the tree arithmetic is restated operation for operation
        assert np.array_equal(ga, a)
        assert np.array_equal(gw.view(np.int32), w.astype(np.float32).view(np.int32))
        assert np.array_equal(grv.view(np.int32), orv.astype(np.float32).view(np.int32))


def test_selfplay_records_identical_in_every_form(cuda, monkeypatch):
    """play_stream, 96 games through 48 lanes at S = 8: the searches run on device-compacted batches (the row count
    read on the device) in the shared self-play workspace; every record buffer is equal."""
    from exploring_muzero_on_dog_amd import detmadn as E
    from exploring_muzero_on_dog_amd import game_agent as GA
    from exploring_muzero_on_dog_amd import nets as N
    C = E.num_channels(2)
    net = N.DeviceNet(N.init_muzero_params(3, C), C)

    def play():
        eng = GA.SelfPlayEngine(net, 48, num_players=2, max_steps=100, num_simulations=8, max_depth=4)
        return {k: v.clone() for k, v in eng.play_stream(96, 21, 1.0).items()}

    monkeypatch.setenv("MUZ_SELECT_INVARIANTS", "0")
    want = play()
    assert int(want["idx"].sum()) > 96 * 50     # real games, not empty records
    for form in (None, "2"):
        if form is None:
            monkeypatch.delenv("MUZ_SELECT_INVARIANTS")
        else:
            monkeypatch.setenv("MUZ_SELECT_INVARIANTS", form)
        got = play()
        for k in want:
            assert torch.equal(got[k], want[k]), (k, form)
