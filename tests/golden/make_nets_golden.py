"""Records the fp32 outputs of the NumPy network restatements (oracle/nets.py, oracle/classic_nets.py,
oracle/dog_muzero.py) for a few fixed rows into tests/golden/oracle_nets_fp32.npz.

The file pins the restatements' default precision: tests/test_oracle_precision.py asserts that today's fp32 run
reproduces it bit for bit, so a change to the oracle (such as its float64 switch) cannot move the fp32 yardstick the
GPU tests compare against.  It was written by the oracle as it stood before the precision switch existed; rerun only
when the restatement itself is meant to change:  python tests/golden/make_nets_golden.py [output.npz]

fp32 matrix products are bit-reproducible only for one BLAS kernel (OpenBLAS picks its kernel by the CPU it runs on, and
the kernels block the k loop differently; its threaded drivers split small products differently again), so as a script
this file pins OpenBLAS to its Haswell kernels (AVX2 + FMA: every x86-64 machine this project runs on has them) on one
thread before NumPy loads; the recorded bits are that configuration's.
"""
import os
import subprocess
import sys

PIN = {"OPENBLAS_CORETYPE": "Haswell", "OPENBLAS_NUM_THREADS": "1"}
if __name__ == "__main__" and any(os.environ.get(k) != v for k, v in PIN.items()):
    sys.exit(subprocess.run([sys.executable] + sys.argv, env={**os.environ, **PIN}).returncode)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import classic_nets as CN  # noqa: E402
from oracle import dog_muzero as DM  # noqa: E402
from oracle import nets as ON  # noqa: E402

ROWS = 5


def inputs():
    """Seeded inputs: 0/1/2 board planes and small integer global features (the encodings' value range), unit-range
    latents, actions that include both out-of-range sides."""
    rng = np.random.default_rng(2024)
    out = {}
    for game, C in (("det", 14), ("classic", 11), ("dog", 34)):
        obs = np.zeros((ROWS, C, 56), np.float32)
        obs[:, :6] = rng.integers(0, 2, (ROWS, 6, 56))
        obs[:, 6:] = rng.integers(0, 5, (ROWS, C - 6, 1))
        out[f"{game}_obs"] = obs
    lat = rng.random((ROWS, 256), dtype=np.float32)
    out["latent"] = lat
    out["det_action"] = np.array([-1, 0, 23, 24, 7], np.int32)
    out["classic_action"] = np.array([-1, 0, 3, 4, 2], np.int32)
    out["classic_chance"] = np.array([-1, 0, 5, 6, 3], np.int32)
    out["dog_action"] = np.array([-1, 0, 805, 806, 400], np.int32)
    return out


def outputs(x):
    """Every entry point on the inputs -> {name: array}."""
    out = {}
    det = ON.init_params(14, seed=7, randomize_affine=True)
    for k, v in zip(("logits", "value", "latent"), ON.root_inference(det, x["det_obs"])):
        out[f"det_root_{k}"] = v
    for k, v in zip(("reward", "discount", "logits", "value", "latent"),
                    ON.recurrent_inference(det, x["det_action"], x["latent"])):
        out[f"det_recurrent_{k}"] = v
    cl = CN.init_params(11, seed=8, randomize_affine=True)
    for k, v in zip(("logits", "value", "latent"), CN.root_inference(cl, x["classic_obs"])):
        out[f"classic_root_{k}"] = v
    for k, v in zip(("chance_logits", "value", "afterstate", "reward", "discount"),
                    CN.decision_recurrent(cl, x["classic_action"], x["latent"])):
        out[f"classic_decision_{k}"] = v
    for k, v in zip(("logits", "value", "latent"), CN.chance_recurrent(cl, x["classic_chance"], x["latent"])):
        out[f"classic_chance_{k}"] = v
    dog = DM.init_params(seed=9, randomize_affine=True)
    for k, v in zip(("logits", "value", "latent"), DM.root_inference(dog, x["dog_obs"])):
        out[f"dog_root_{k}"] = v
    for k, v in zip(("reward", "discount", "logits", "value", "latent"),
                    DM.recurrent_inference(dog, x["dog_action"], x["latent"])):
        out[f"dog_recurrent_{k}"] = v
    return out


if __name__ == "__main__":
    x = inputs()
    y = outputs(x)
    assert all(v.dtype == np.float32 for v in y.values())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "oracle_nets_fp32.npz")
    np.savez_compressed(path, **{f"in_{k}": v for k, v in x.items()}, **y)
    print(path, os.path.getsize(path), "bytes,", len(y), "outputs")
