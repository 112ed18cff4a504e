"""The network restatements' precision switch (oracle.nets.precision) on the CPU.

* default precision: every entry point of oracle/nets.py, oracle/classic_nets.py and oracle/dog_muzero.py returns fp32
  arrays bit-identical to tests/golden/oracle_nets_fp32.npz, recorded before the switch existed
  (tests/golden/make_nets_golden.py) -- the fp32 yardstick of the GPU tests did not move.  fp32 matrix products are
  bit-reproducible only under one BLAS kernel and thread count, which must be chosen before NumPy loads, so the
  bit-for-bit comparison runs the recorder in a child process pinned the way the recording was (one second); in this
  process, under whatever kernel the CPU selects, the same outputs are held to 1e-5 of the record, the project's bar for
  two fp32 summation orders of these networks (measured between the AVX2 and AVX-512 kernels: 2.6e-6 at most);
* inside ``precision(np.float64)`` the same functions return float64, and agree with the fp32 run to 1e-4;
* the switch restores the previous precision on exit, also after an exception."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import classic_nets as CN
from oracle import dog_muzero as DM
from oracle import nets as ON

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
    spec = importlib.util.spec_from_file_location("make_nets_golden", os.path.join(HERE, "golden", "make_nets_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "oracle_nets_fp32.npz"))
    x = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    y = {k: z[k] for k in z.files if not k.startswith("in_")}
    return _gen(), x, y


def test_golden_inputs_are_the_generators(golden):
    gen, x, _ = golden
    now = gen.inputs()
    assert sorted(now) == sorted(x)
    for k in x:
        assert now[k].dtype == x[k].dtype and np.array_equal(now[k], x[k]), k


def test_default_precision_is_fp32_and_unchanged(golden, tmp_path):
    gen, x, y = golden
    path = str(tmp_path / "now.npz")
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_nets_golden.py"), path], check=True,
                   env={**os.environ, **gen.PIN}, stdout=subprocess.DEVNULL)
    out = np.load(path)
    assert sorted(k for k in out.files if not k.startswith("in_")) == sorted(y)
    for k in y:
        assert out[k].dtype == np.float32, (k, out[k].dtype)
        assert out[k].shape == y[k].shape and np.array_equal(out[k], y[k]), \
            (k, float(np.abs(out[k] - y[k]).max()))


def test_default_precision_in_process(golden):
    gen, x, y = golden
    out = gen.outputs(x)
    for k in y:
        assert out[k].dtype == np.float32 and out[k].shape == y[k].shape, (k, out[k].dtype)
        d = float(np.abs(out[k] - y[k]).max())
        assert d <= 1e-5, (k, d)


def test_float64_run(golden):
    gen, x, y = golden
    with ON.precision(np.float64):
        out = gen.outputs(x)
    for k in y:
        assert out[k].dtype == np.float64, (k, out[k].dtype)
        assert np.isfinite(out[k]).all(), k
        d = float(np.abs(out[k] - y[k]).max())
        assert d <= 1e-4, (k, d)
    # and the default is back
    again = gen.outputs(x)
    assert all(again[k].dtype == np.float32 for k in y)


def test_switch_reaches_all_three_modules_and_restores():
    assert CN.precision is ON.precision and DM.precision is ON.precision
    assert ON.one_hot(np.array([1]), 3).dtype == np.float32 and ON.support().dtype == np.float32
    with pytest.raises(RuntimeError):
        with ON.precision(np.float64):
            assert ON.one_hot(np.array([1]), 3).dtype == np.float64 and ON.support().dtype == np.float64
            with ON.precision(np.float32):
                assert ON.support().dtype == np.float32
            assert ON.support().dtype == np.float64
            raise RuntimeError("leave the block by an exception")
    assert ON.support().dtype == np.float32
    with pytest.raises(ValueError):
        with ON.precision(np.float16):
            pass


def test_float64_intermediates_are_float64():
    """No layer drops to fp32 on the way: a LayerNorm input whose fp32 variance cancels to 0 keeps its float64 one."""
    p = {"ln/scale": np.ones(4, np.float32), "ln/bias": np.zeros(4, np.float32)}
    x = np.array([[1.0, 1.0 + 2e-7, 1.0, 1.0 - 2e-7]], np.float64)
    with ON.precision(np.float64):
        y = ON.layer_norm(p, "ln", x)
    assert y.dtype == np.float64
    var = float((x * x).mean() - x.mean() ** 2)
    want = (x - x.mean()) / np.sqrt(max(var, 0.0) + 1e-6)
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-9)
    assert np.abs(y).max() > 1e-4     # (fp32 would see x = [1, 1 + 2.4e-7, 1, 1 - 1.8e-7] at best)
