"""The host side of the det, classic and DOG networks after they were put on one construction path (nets.init_params,
nets.flat_f32, _Packer.from_params, Learner.from_params): what it builds, held to names and hashes recorded from the
commit before (tests/golden/nets_host.json, written by tests/golden/make_nets_host_golden.py from that commit's
package).  No GPU: packers stop before their FiLM-table kernel, learners are built on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _nets_host as H

GAMES = ("det", "classic", "dog")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nets_host.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def trees():
    """One parameter dict per game (every leaf drawn), shared and left unchanged."""
    inits = H.initialisers()
    return {g: H.pack_params(inits[g]) for g in GAMES}


@pytest.mark.parametrize("game", GAMES)
def test_initialiser_bytes_equal_parent(golden, game):
    """Same key order, shapes, dtype and bytes per seed as the three separate loops gave (one of them used
    math.sqrt, two np.sqrt)."""
    assert H.init_record(H.initialisers()[game]) == golden["init"][game]


@pytest.mark.parametrize("game", GAMES)
def test_packed_arena_and_spec_equal_parent(golden, trees, game):
    net = H.packers()[game].from_params(trees[game], device="cpu", prepare=False)
    assert H.pack_record(net._chunks, net.spec) == golden["pack"][game]
    assert np.array_equal(net.buffer.numpy(), np.concatenate(net._chunks))


@pytest.mark.parametrize("game", GAMES)
def test_from_params_infers_shape(trees, game):
    from exploring_muzero_on_dog_amd import learner as LR
    from exploring_muzero_on_dog_amd import nets as N
    assert N.infer_shape(trees[game]) == H.SHAPES[game]
    net = H.packers()[game].from_params(trees[game], device="cpu", prepare=False)
    assert (net.C, net.A) == H.SHAPES[game] and (net.w.obs_channels, net.w.num_actions) == H.SHAPES[game]
    nets = {"det": LR.MuZeroNets, "classic": LR.ClassicMuZeroNets, "dog": LR.DogMuZeroNets}[game]
    nets = nets.from_params(trees[game], device="cpu")
    assert (nets.C, nets.A) == H.SHAPES[game] and list(nets.p) == list(trees[game])


def test_dog_wrong_action_width_is_value_error():
    from exploring_muzero_on_dog_amd import learner as LR
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    from exploring_muzero_on_dog_amd import nets as N
    wrong = N.init_muzero_params(0, MD.NUM_CHANNELS, 24)       # det-shaped at C = 34: 24 actions, not 806
    wrong["representation/LayerNorm_7/scale"] = wrong["representation/LayerNorm_7/bias"] = np.ones(256, np.float32)
    with pytest.raises(ValueError):
        MD.DeviceDogNet.from_params(wrong, device="cpu", prepare=False)
    with pytest.raises(ValueError):
        LR.DogMuZeroNets.from_params(wrong, device="cpu")


def test_flat_f32_accepts_trees_and_flat_dicts_of_either_leaf():
    from exploring_muzero_on_dog_amd import checkpoint as CK
    from exploring_muzero_on_dog_amd import nets as N
    flat = N.init_muzero_params(1, 11, 24)
    mixed = {k: (torch.from_numpy(v).double().requires_grad_() if i % 2 else v.astype(np.float64))
             for i, (k, v) in enumerate(flat.items())}
    for given in (flat, mixed, CK.flat_to_muzero_tree(flat), CK.flat_to_muzero_tree(mixed)):
        got = N.flat_f32(given)
        assert set(got) == set(flat)
        for k, v in got.items():
            assert isinstance(v, np.ndarray) and v.dtype == np.float32 and np.array_equal(v, flat[k]), k


@pytest.mark.parametrize("game", GAMES)
def test_learner_and_optimizer_construction(trees, game):
    """Learner.from_params builds each of the three on the CPU, and training.Optimizer.init needs no per-game branch
    or subclass: it takes the Flax tree as the reference's optimizer.init does."""
    from exploring_muzero_on_dog_amd import checkpoint as CK
    from exploring_muzero_on_dog_amd import learner as LR
    from exploring_muzero_on_dog_amd import training as T
    cls = {"det": LR.Learner, "classic": LR.StochasticLearner, "dog": LR.DogLearner}[game]
    flat = trees[game]
    learner = cls.from_params(flat, device="cpu", unroll_steps=3)
    assert type(learner) is cls and type(learner.nets) is cls.NETS and learner.unroll_steps == 3
    assert list(learner.nets.p) == list(flat)
    for k, p in learner.nets.p.items():
        assert p.dtype == torch.float32 and np.array_equal(p.detach().numpy(), flat[k]), k
    want = LR.CLASSIC_LR_BOUNDARIES if game == "classic" else LR.DET_LR_BOUNDARIES
    assert tuple(learner.opt.boundaries) == tuple(want)
    opt = T.Optimizer(cls, 3, 0.005, 10, LR.DET_LR_BOUNDARIES, graph=False, device="cpu")
    st = opt.init(CK.flat_to_muzero_tree(flat))
    assert type(st.learner) is cls and list(st.learner.nets.p) == list(flat)
    assert st.learner.opt.boundaries == LR.DET_LR_BOUNDARIES and st.learner.unroll_steps == 3
    assert CK.muzero_tree_to_flat_any(st.tree)["prediction/Dense_2/kernel"] is st.learner.nets.p["prediction/Dense_2/kernel"]
