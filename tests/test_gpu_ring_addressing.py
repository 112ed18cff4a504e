"""The dense layers' weight addressing (csrc/nn.hpp, template flag SB): a wave-uniform base in scalar registers plus one
32-bit lane offset (the default) against a 64-bit address per lane (MUZ_RING_ADDR=0, the form before).  Both read the
same bytes into the same MFMAs in the same order, so every output of k_recurrent, k_root_dense and k_gumbel_search is
bit for bit the same in both forms; MUZ_RING_ADDR is read per launch, so one process runs both.

Shapes: n in {1, 15, 16, 17, 33} rows (a lone row, a tile edge on either side, two full tiles plus one); for the search
S in {1, 2, 17} and D in {1, 3}.  Networks: randomly initialised 2-player (18 channels) and 4-player (34 channels) nets
on observations from random play with their real legal masks; the recurrent actions include -1 and 24 (out of range: a
zero one-hot row).  The search's workspace is filled with 0xFF bytes before every call (_search)."""
import numpy as np
import pytest
import torch

from tests import test_gpu_search as TS
from tests.test_gpu_select_invariants import _search

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 33)
NETS = [(2, "selfplay_2p"), (4, "selfplay_4p_teams")]
_CTX = {}


def _ctx(P, rule_set):
    """Network, 33 roots (observations, legal bits, the default form's root inference), Gumbel noise: computed once."""
    if P not in _CTX:
        N, M, params, net, obs, valid, bits = TS.setup(P, 48, 7, rule_set)
        assert obs.shape[0] >= max(NS) and obs.shape[1] == (18, 34)[P == 4]
        obs = torch.from_numpy(obs[:max(NS)]).cuda()
        lg, v, e = N.root_inference_fn(net, obs)
        rng = np.random.default_rng(13)
        gum = rng.gumbel(size=(max(NS), 24)).astype(np.float32)
        act = rng.integers(0, 24, max(NS)).astype(np.int32)
        act[::5] = -1
        act[3::7] = 24
        _CTX[P] = dict(N=N, M=M, net=net, obs=obs, lg=lg, v=v, e=e, bits=bits[:max(NS)], gum=gum,
                       act=torch.from_numpy(act).cuda())
    return _CTX[P]


def _both_forms(monkeypatch, call):
    """call() under MUZ_RING_ADDR=0, then 1: two tuples of outputs"""
    out = []
    for form in ("0", "1"):
        monkeypatch.setenv("MUZ_RING_ADDR", form)
        out.append(call())
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("P,rule_set", NETS)
def test_recurrent_outputs_bit_identical(cuda, monkeypatch, P, rule_set):
    c = _ctx(P, rule_set)
    for n in NS:
        old, new = _both_forms(monkeypatch, lambda: c["N"].recurrent_inference_fn(c["net"], c["act"][:n], c["e"][:n]))
        for name, o, w in zip(("reward", "discount", "logits", "value", "latent"), new, old):
            assert torch.equal(o, w), (name, n)
        assert all(bool(torch.isfinite(o).all()) for o in new), n


@pytest.mark.parametrize("P,rule_set", NETS)
def test_root_outputs_bit_identical(cuda, monkeypatch, P, rule_set):
    c = _ctx(P, rule_set)
    for n in NS:
        old, new = _both_forms(monkeypatch, lambda: c["N"].root_inference_fn(c["net"], c["obs"][:n]))
        for name, o, w in zip(("logits", "value", "embedding"), new, old):
            assert torch.equal(o, w), (name, n)
        assert all(bool(torch.isfinite(o).all()) for o in new), n


@pytest.mark.parametrize("P,rule_set", NETS)
def test_search_outputs_bit_identical(cuda, monkeypatch, P, rule_set):
    c = _ctx(P, rule_set)
    monkeypatch.delenv("MUZ_SELECT_INVARIANTS", raising=False)   # the default form: the one with both addressings
    for n in (1, 16, 17, 33):
        rows = list(range(n))
        for S in (1, 2, 17):
            for D in (1, 3):
                old, new = _both_forms(monkeypatch, lambda: _search(c, rows, S, D, 16))
                for name, o, w in zip(("action", "action_weights", "root_value_out"), new, old):
                    assert torch.equal(torch.from_numpy(o), torch.from_numpy(w)), (name, n, S, D)
                legal = (c["bits"][rows][:, None] >> np.arange(24)) & 1
                assert legal[np.arange(n), new[0]].all(), ("illegal action", n, S, D)
