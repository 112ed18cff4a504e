"""What the three network modules build on the host, as names and hashes: shared by tests/test_nets_host.py and
tests/golden/make_nets_host_golden.py, which records them from the commit before the one-construction-path refactor."""
import hashlib

import numpy as np

SEEDS = (0, 7)
SHAPES = {"det": (34, 24), "classic": (11, 4), "dog": (34, 806)}     # (C, A); det and classic at 4 players


def initialisers() -> dict:
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    from exploring_muzero_on_dog_amd import nets as N
    from exploring_muzero_on_dog_amd import stochastic as ST
    return {"det": lambda s: N.init_muzero_params(s, SHAPES["det"][0]),
            "classic": lambda s: ST.init_classic_params(SHAPES["classic"][0], s),
            "dog": lambda s: MD.init_muzero_params(s)}


def packers() -> dict:
    from exploring_muzero_on_dog_amd import muzero_dog as MD
    from exploring_muzero_on_dog_amd import nets as N
    from exploring_muzero_on_dog_amd import stochastic as ST
    return {"det": N.DeviceNet, "classic": ST.DeviceClassicNet, "dog": MD.DeviceDogNet}


def sha256(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def init_record(fn) -> dict:
    """Key order, shapes and dtypes (the same for every seed) and the SHA-256 of the concatenated bytes per seed."""
    outs = {s: fn(s) for s in SEEDS}
    first = outs[SEEDS[0]]
    for o in outs.values():
        assert list(o) == list(first) and [v.shape for v in o.values()] == [v.shape for v in first.values()]
    return {"keys": list(first), "shapes": [list(v.shape) for v in first.values()],
            "dtypes": sorted({str(v.dtype) for v in first.values()}),
            "sha256": {str(s): sha256(o.values()) for s, o in outs.items()}}


def pack_params(fn, seed: int = 3) -> dict:
    """An initialiser's tree with the biases and LayerNorm scales drawn too (they start as zeros and ones, which
    would hide two of them changing places in the arena)."""
    rng = np.random.default_rng(seed + 100)
    return {k: v if k.endswith("kernel") else rng.standard_normal(v.shape).astype(np.float32)
            for k, v in fn(seed).items()}


def pack_record(chunks, spec) -> dict:
    """The host arena (the packed chunks before upload) and the spec's offsets (nested dict / list / tuple of ints)."""
    host = np.concatenate(chunks)
    return {"floats": int(host.size), "arena_sha256": sha256([host]),
            "spec_sha256": hashlib.sha256(repr(spec).encode()).hexdigest()}
