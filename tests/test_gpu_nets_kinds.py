"""The one construction path of the det, classic and DOG networks on the device: the weight cache behind the three
``as_device_*`` functions (nets.cached_device_net; the DOG one had no such test, and no hit path) and Learner.push_to,
which packs with the class of the net it is given.  Shapes: the games' own (C, A) at 4 players; B = 1 and B = 17 (one
row, and one row past the packed layers' 16-row tile) where a kernel runs."""
import numpy as np
import pytest
import torch

from tests import _nets_host as H

pytestmark = pytest.mark.gpu
GAMES = ("det", "classic", "dog")


def _kinds():
    from exploring_muzero_on_dog_amd import learner as LR
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    from exploring_muzero_on_dog_amd import nets as N
    from exploring_muzero_on_dog_amd import stochastic as ST
    return {"det": (N, N.as_device_net, N.DeviceNet, LR.Learner),
            "classic": (ST, ST.as_device_classic_net, ST.DeviceClassicNet, LR.StochasticLearner),
            "dog": (MD, MD.as_device_net, MD.DeviceDogNet, LR.DogLearner)}


@pytest.fixture(scope="module")
def trees():
    """Two parameter dicts per game (every leaf drawn), shared; the tests change copies only."""
    inits = H.initialisers()
    return {g: (H.pack_params(inits[g], 3), H.pack_params(inits[g], 4)) for g in GAMES}


@pytest.mark.parametrize("game", GAMES)
def test_as_device_net_cache(cuda, trees, game):
    mod, as_device, cls, _ = _kinds()[game]
    mod._NET_CACHE.clear()
    try:
        flat = {k: v.copy() for k, v in trees[game][0].items()}
        net = as_device(flat)
        assert type(net) is cls and net.buffer.device.type == "cuda"
        assert as_device(net) is net
        assert torch.equal(net.buffer, cls.from_params(flat).buffer)
        # the same, unchanged dict: the cached net, nothing re-packed (its buffer keeps a mark that packing would erase)
        assert net.buffer[0].item() != 12345.0
        net.buffer[0] = 12345.0
        assert as_device(flat) is net and net.buffer[0].item() == 12345.0
        # one leaf changed in place: the same object, now holding the new weights (and the mark gone)
        flat["dynamics/ResBlock_1/Dense_0/bias"][5] += 0.25
        assert as_device(flat) is net
        assert torch.equal(net.buffer, cls.from_params(flat).buffer)
        # another dict of the same shapes: its weights, still in the first net object
        other = trees[game][1]
        assert as_device(other) is net
        assert torch.equal(net.buffer, cls.from_params(other).buffer)
        assert not torch.equal(net.buffer, cls.from_params(flat).buffer)
        assert len(mod._NET_CACHE) == 1
    finally:
        mod._NET_CACHE.clear()


@pytest.mark.parametrize("game", GAMES)
def test_push_to_packs_with_the_nets_own_class(cuda, trees, game):
    mod, _, cls, learner_cls = _kinds()[game]
    learner = learner_cls.from_params(trees[game][0], device=cuda)
    net = cls.from_params(trees[game][1])
    before = net.buffer.clone()
    learner.push_to(net)
    fresh = cls.from_params(learner.nets.numpy())
    assert type(fresh) is cls and torch.equal(net.buffer, fresh.buffer) and not torch.equal(net.buffer, before)
    # the pushed-to net computes what the fresh one does, below and past one 16-row tile
    rng = np.random.default_rng(11)
    for B in (1, 17):
        obs = torch.from_numpy(rng.integers(0, 3, (B, net.C, 56)).astype(np.float32)).to(cuda)
        for x, y in zip(mod.root_inference_fn(net, obs), mod.root_inference_fn(fresh, obs)):
            assert torch.equal(x, y)
