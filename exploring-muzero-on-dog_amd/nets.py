"""MuZero networks of MuZero_det_MADN/muzero_deterministic_madn.py on the GPU.

Host side of the fused fp32 MFMA network kernels (csrc/nets.hip, csrc/nn.hpp):
  * parameter init / layout follow the Flax module tree (paths such as
    ``dynamics/ResBlock_0/Dense_1/kernel``), so checkpoints map 1:1 (init_muzero_params,
    lines 706-748);
  * ``DeviceNet`` packs the dense kernels into the MFMA B-fragment layout documented in
    include/muz.h, uploads everything as one device buffer and fills ``muz_net_w``;
  * ``root_inference_fn`` / ``recurrent_inference_fn`` mirror lines 621-661.
The classic (stochastic.py) and DOG (muzero_dog.py) networks are built from the same pieces: ``init_params``,
``flat_f32`` / ``infer_shape``, ``_Packer`` (``from_params``, ``prepare``), ``root_inference`` / ``recurrent_inference``
and ``cached_device_net``; each of those modules adds its shape table, its ``_spec`` and its entry-point names.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import lib as _L
from .lib import MuzNetW  # struct layout of include/muz.h

LATENT = 256


# ---------------------------------------------------------------------------------- parameters
def _resblock_shapes(s, pre):
    for d in range(2):
        s[f"{pre}/Dense_{d}/kernel"] = (LATENT, LATENT)
        s[f"{pre}/Dense_{d}/bias"] = (LATENT,)
        s[f"{pre}/LayerNorm_{d}/scale"] = (LATENT,)
        s[f"{pre}/LayerNorm_{d}/bias"] = (LATENT,)


def param_shapes(obs_channels: int, num_actions: int = 24) -> dict:
    """Flax parameter tree of (RepresentationNetwork2, DynamicsNetwork4, PredictionNetwork4), flattened."""
    C, A = obs_channels, num_actions
    s = {}
    r = "representation"
    s[f"{r}/Conv_0/kernel"], s[f"{r}/Conv_0/bias"] = (3, 6, 32), (32,)
    s[f"{r}/Conv_1/kernel"], s[f"{r}/Conv_1/bias"] = (3, 32, 64), (64,)
    s[f"{r}/Conv_2/kernel"], s[f"{r}/Conv_2/bias"] = (5, 64, 64), (64,)
    for i, n in enumerate([32, 64, 64, 256, 64, 64, 256]):
        s[f"{r}/LayerNorm_{i}/scale"] = s[f"{r}/LayerNorm_{i}/bias"] = (n,)
    for name, (i, o) in {"Dense_0": (56 * 64, 256), "Dense_1": (C - 6, 64), "Dense_2": (64, 64),
                         "Dense_3": (320, 256), "Dense_4": (256, 256)}.items():
        s[f"{r}/{name}/kernel"], s[f"{r}/{name}/bias"] = (i, o), (o,)
    for b in range(6):
        _resblock_shapes(s, f"{r}/ResBlock_{b}")
    d = "dynamics"
    for name, (i, o) in {"Dense_0": (A, 64), "Dense_1": (64, 256), "Dense_2": (64, 256), "Dense_3": (256, 256),
                         "Dense_4": (256, 256), "Dense_5": (256, 256), "Dense_6": (256 + A, 64),
                         "reward_head": (64, 3), "Dense_7": (256 + A, 64), "discount_head": (64, 3)}.items():
        s[f"{d}/{name}/kernel"], s[f"{d}/{name}/bias"] = (i, o), (o,)
    for i in range(3):
        s[f"{d}/LayerNorm_{i}/scale"] = s[f"{d}/LayerNorm_{i}/bias"] = (LATENT,)
    for b in range(2):
        _resblock_shapes(s, f"{d}/ResBlock_{b}")
    p = "prediction"
    for name, (i, o) in {"Dense_0": (256, 256), "Dense_1": (256, 128), "Dense_2": (128, A), "Dense_3": (256, 128),
                         "Dense_4": (128, 64), "Dense_5": (64, 1)}.items():
        s[f"{p}/{name}/kernel"], s[f"{p}/{name}/bias"] = (i, o), (o,)
    for i, n in enumerate([256, 256, 128, 128]):
        s[f"{p}/LayerNorm_{i}/scale"] = s[f"{p}/LayerNorm_{i}/bias"] = (n,)
    for b in range(2):
        _resblock_shapes(s, f"{p}/ResBlock_{b}")
    return s


def init_params(shapes: dict, seed: int) -> dict:
    """Flax defaults for a flat shape table: lecun_normal kernels (truncated at 2 std), zero biases, unit LayerNorm
    scales.  Seeded NumPy draws in the table's order (jax threefry is not reproduced)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, shp in shapes.items():
        if k.endswith("kernel"):
            std = math.sqrt(1.0 / int(np.prod(shp[:-1]))) / 0.87962566103423978
            out[k] = (np.clip(rng.standard_normal(shp), -2.0, 2.0) * std).astype(np.float32)
        else:
            out[k] = (np.ones if k.endswith("scale") else np.zeros)(shp, np.float32)
    return out


def init_muzero_params(seed: int, obs_channels: int, num_actions: int = 24) -> dict:
    """init_muzero_params (lines 706-748) with Flax defaults (init_params)."""
    return init_params(param_shapes(obs_channels, num_actions), seed)


def flat_tree(params) -> dict:
    """Reference params -> flat ``{"net/Layer/param": leaf}``, the leaves as they are: init_muzero_params' nested Flax
    tree (``{"representation": {"params": ...}, "dynamics": ..., "prediction": ...}``) or an already flat dict."""
    if isinstance(params, dict) and all(isinstance(k, str) and "/" in k for k in params):
        return params
    from . import checkpoint as CK
    return CK.muzero_tree_to_flat_any(params)


def flat_f32(params) -> dict:
    """flat_tree with every leaf (torch, on any device, or NumPy) as a host float32 ndarray."""
    return {k: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float32)
            for k, v in flat_tree(params).items()}


def infer_shape(flat: dict, obs_channels: int | None = None) -> tuple:
    """(C, A) of a flat parameter dict: the representation's Dense_1 takes the C - 6 non-board channels, the
    prediction's Dense_2 gives the A logits."""
    C = int(flat["representation/Dense_1/kernel"].shape[0]) + 6 if obs_channels is None else int(obs_channels)
    return C, int(flat["prediction/Dense_2/kernel"].shape[1])


# ---------------------------------------------------------------------------------- packing
def nt_for(N: int, nw: int) -> int:
    """16-column MFMA tiles per wave for a layer of N outputs split over nw waves (csrc/nn.hpp:nt_for)."""
    return -(-N // (16 * nw))


def pack_dense(W: np.ndarray, nw: int, nt: int) -> np.ndarray:
    """MFMA 16x16x4 B-fragment packing (layout documented in include/muz.h):
    out[w][kb][lane][t][j] = W[kb*16 + 4*(lane>>4) + j][(w*nt + t)*16 + (lane&15)]."""
    W = np.asarray(W, np.float32)
    K, N = W.shape
    KB = (K + 15) // 16
    Np = nw * nt * 16
    if N > Np:
        raise ValueError(f"N={N} does not fit {nw} groups x {nt} tiles")
    Wp = np.zeros((KB * 16, Np), np.float32)
    Wp[:K, :N] = W
    arr = Wp.reshape(KB, 4, 4, nw, nt, 16).transpose(3, 0, 1, 5, 4, 2)
    return np.ascontiguousarray(arr).reshape(-1)


class _Packer:
    """Builds one device buffer of packed parameters and fills a ctypes weight table from a nested spec
    (leaf = offset in floats, (w, b) pair = muz_dense / muz_ln, list = array field, dict = sub-struct).

    A subclass names its weight table, its C entry points and, where the game fixes them, its (C, A); ``_spec`` lays
    the parameters out.  Its constructor and ``from_params`` both end in ``_pack``."""

    TABLE = None                          # the ctypes weight table (include/muz.h)
    PREPARE = ROOT = RECURRENT = None     # C entry points (lib.SIGNATURES)
    SHAPE = (None, None)                  # (C, A) where the game fixes one

    @classmethod
    def from_params(cls, flat: dict, device="cuda", obs_channels: int | None = None, prepare: bool = True):
        """A flat parameter dict -> the packed net, (C, A) read from its shapes (infer_shape).  prepare=False stops
        after the upload (the host layout alone, no kernel)."""
        net = cls.__new__(cls)
        net._pack(flat, *infer_shape(flat, obs_channels), device, prepare)
        return net

    def _pack(self, params: dict, obs_channels: int, num_actions: int, device, prepare: bool = True):
        self.C, self.A = int(obs_channels), int(num_actions)
        if any(want is not None and want != got for want, got in zip(self.SHAPE, (self.C, self.A))):
            raise ValueError(f"{type(self).__name__}: (C, A) = {(self.C, self.A)} != {self.SHAPE}")
        self.waves = _L.load().muz_tile_waves()   # column groups of the packed 16-row layers (csrc/nn.hpp kWaves)
        self._chunks = []
        self._off = 0
        self.params = {k: np.asarray(v, np.float32) for k, v in params.items()}
        self.w = self.TABLE()
        self.w.obs_channels, self.w.num_actions = self.C, self.A
        self.spec = self._spec()
        self.buffer = torch.from_numpy(np.concatenate(self._chunks)).to(device)
        self._fill(self.w, self.spec, self.buffer.data_ptr())
        if prepare:
            self.prepare()

    def prepare(self):
        """Re-derive the FiLM tables from the packed weights (after they change in place, e.g. a parameter
        broadcast from the learner)."""
        with torch.cuda.device(self.buffer.device):
            _L.check(getattr(_L.load(), self.PREPARE)(ctypes.byref(self.w), _L.stream_ptr()), self.PREPARE)

    def _put(self, arr) -> int:
        a = np.ascontiguousarray(np.asarray(arr, np.float32).reshape(-1))
        pad = (-a.size) % 4          # keep every array 16-byte aligned for f32x4 loads
        if pad:
            a = np.concatenate([a, np.zeros(pad, np.float32)])
        off = self._off
        self._chunks.append(a)
        self._off += a.size
        return off

    def _dense_k(self, k, b):
        return (self._put(pack_dense(k, self.waves, nt_for(k.shape[1], self.waves))), self._put(b))

    def _dense(self, name):
        return self._dense_k(self.params[f"{name}/kernel"], self.params[f"{name}/bias"])

    def _plain(self, name):
        return (self._put(self.params[f"{name}/kernel"]), self._put(self.params[f"{name}/bias"]))

    def _ln(self, name):
        return (self._put(self.params[f"{name}/scale"]), self._put(self.params[f"{name}/bias"]))

    def _rb(self, pre):
        return dict(d0=self._dense(f"{pre}/Dense_0"), ln0=self._ln(f"{pre}/LayerNorm_0"), d1=self._dense(f"{pre}/Dense_1"),
                    ln1=self._ln(f"{pre}/LayerNorm_1"))

    def _repr_spec(self):
        P, put, r = self.params, self._put, "representation"
        return dict(
            conv0=(put(P[f"{r}/Conv_0/kernel"]), put(P[f"{r}/Conv_0/bias"])), ln0=self._ln(f"{r}/LayerNorm_0"),
            # the conv kernels as 4 column groups of one 16-channel tile each (k_repr_conv: one group per wave)
            conv1=(put(pack_dense(P[f"{r}/Conv_1/kernel"].reshape(96, 64), 4, 1)), put(P[f"{r}/Conv_1/bias"])),
            ln1=self._ln(f"{r}/LayerNorm_1"),
            conv2=(put(pack_dense(P[f"{r}/Conv_2/kernel"].reshape(320, 64), 4, 1)), put(P[f"{r}/Conv_2/bias"])),
            ln2=self._ln(f"{r}/LayerNorm_2"), d0=self._dense(f"{r}/Dense_0"), ln3=self._ln(f"{r}/LayerNorm_3"),
            d1=self._dense(f"{r}/Dense_1"), ln4=self._ln(f"{r}/LayerNorm_4"), d2=self._dense(f"{r}/Dense_2"),
            ln5=self._ln(f"{r}/LayerNorm_5"), d3=self._dense(f"{r}/Dense_3"), ln6=self._ln(f"{r}/LayerNorm_6"),
            rb=[self._rb(f"{r}/ResBlock_{i}") for i in range(6)], d4=self._dense(f"{r}/Dense_4"))

    def _pred_spec(self, logits: bool = True):
        """PredictionNetwork4; logits=False leaves Dense_2 (``d2``) to the caller (DOG packs it in column chunks)."""
        P, p = self.params, "prediction"
        spec = dict(
            ln0=self._ln(f"{p}/LayerNorm_0"), rb=[self._rb(f"{p}/ResBlock_{i}") for i in range(2)],
            d03=self._dense_k(np.concatenate([P[f"{p}/Dense_0/kernel"], P[f"{p}/Dense_3/kernel"]], 1),
                              np.concatenate([P[f"{p}/Dense_0/bias"], P[f"{p}/Dense_3/bias"]])),
            ln1=self._ln(f"{p}/LayerNorm_1"), d1=self._dense(f"{p}/Dense_1"), ln2=self._ln(f"{p}/LayerNorm_2"))
        if logits:
            spec["d2"] = self._dense(f"{p}/Dense_2")
        spec.update(ln3=self._ln(f"{p}/LayerNorm_3"), d4=self._dense(f"{p}/Dense_4"), d5=self._plain(f"{p}/Dense_5"))
        return spec

    def _dyn_spec(self):
        """DynamicsNetwork4 (lines 391-457); the FiLM table [A + 1][512] is derived on the device (prepare)."""
        P, put, A, d = self.params, self._put, self.A, "dynamics"
        k6, k7 = P[f"{d}/Dense_6/kernel"], P[f"{d}/Dense_7/kernel"]
        return dict(
            d0=self._plain(f"{d}/Dense_0"), ln0=self._ln(f"{d}/LayerNorm_0"),
            d12=self._dense_k(np.concatenate([P[f"{d}/Dense_1/kernel"], P[f"{d}/Dense_2/kernel"]], 1),
                              np.concatenate([P[f"{d}/Dense_1/bias"], P[f"{d}/Dense_2/bias"]])),
            d3=self._dense(f"{d}/Dense_3"), ln1=self._ln(f"{d}/LayerNorm_1"), d4=self._dense(f"{d}/Dense_4"),
            ln2=self._ln(f"{d}/LayerNorm_2"), rb=[self._rb(f"{d}/ResBlock_{i}") for i in range(2)],
            d5=self._dense(f"{d}/Dense_5"),
            d67=self._dense_k(np.concatenate([k6[:LATENT], k7[:LATENT]], 1),
                              np.concatenate([P[f"{d}/Dense_6/bias"], P[f"{d}/Dense_7/bias"]])),
            d67_onehot=put(np.concatenate([k6[LATENT:LATENT + A], k7[LATENT:LATENT + A]], 1)),
            reward_head=self._plain(f"{d}/reward_head"), discount_head=self._plain(f"{d}/discount_head"),
            film=put(np.zeros((A + 1) * 2 * LATENT, np.float32)))

    @staticmethod
    def _fill(struct, spec, base):
        for name, val in spec.items():
            field = getattr(struct, name)
            if isinstance(val, int):
                setattr(struct, name, base + 4 * val)
            elif isinstance(val, tuple):
                field.__setattr__(field._fields_[0][0], base + 4 * val[0])
                field.__setattr__(field._fields_[1][0], base + 4 * val[1])
            elif isinstance(val, list):
                for i, sub in enumerate(val):
                    if isinstance(sub, tuple):     # array of muz_dense / muz_ln
                        f = field[i]
                        f.__setattr__(f._fields_[0][0], base + 4 * sub[0])
                        f.__setattr__(f._fields_[1][0], base + 4 * sub[1])
                    else:
                        _Packer._fill(field[i], sub, base)
            elif isinstance(val, dict):
                _Packer._fill(field, val, base)
            else:
                raise TypeError(name)


class DeviceNet(_Packer):
    """Packed device copy of a det-MADN parameter dict + the ``muz_net_w`` table the kernels read."""

    TABLE = MuzNetW
    PREPARE, ROOT, RECURRENT = "muz_net_prepare", "muz_nets_root", "muz_nets_recurrent"

    def __init__(self, params: dict, obs_channels: int, num_actions: int = 24, device="cuda"):
        self._pack(params, obs_channels, num_actions, device)

    def _spec(self):
        return {"repr": self._repr_spec(), "dyn": self._dyn_spec(), "pred": self._pred_spec()}


# ---------------------------------------------------------------------------------- inference
def root_inference(net: _Packer, observation: torch.Tensor, scratch: torch.Tensor | None = None):
    """root_inference_fn (lines 621-630) of any of the three games' nets (``net.ROOT``): obs [B, C, 56] ->
    (prior_logits [B, A], value [B], embedding [B, 256])."""
    lib = _L.load()
    obs = observation.to(dtype=torch.float32).contiguous()
    B, dev = obs.shape[0], obs.device
    if tuple(obs.shape[1:]) != (net.C, 56):
        raise ValueError(f"observation shape {tuple(obs.shape)} != (B, {net.C}, 56)")
    need = lib.muz_nets_root_scratch_bytes(B)
    if scratch is None or _L.nbytes(scratch) < need:
        scratch = torch.empty(need // 4, dtype=torch.float32, device=dev)
    logits = torch.empty((B, net.A), dtype=torch.float32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    emb = torch.empty((B, LATENT), dtype=torch.float32, device=dev)
    _L.check(getattr(lib, net.ROOT)(net.w, _L.ptr(obs), B, _L.ptr(scratch), _L.nbytes(scratch), _L.ptr(logits),
                                    _L.ptr(value), _L.ptr(emb), _L.stream_ptr()), net.ROOT)
    return logits, value, emb


def recurrent_inference(net: _Packer, action: torch.Tensor, embedding: torch.Tensor):
    """recurrent_inference_fn (lines 632-661) of the det or the DOG net (``net.RECURRENT``) ->
    (reward, discount, prior_logits [B, A], value, next_embedding)."""
    emb = embedding.to(dtype=torch.float32).contiguous()
    act = action.to(device=emb.device, dtype=torch.int32).contiguous()
    B, dev = emb.shape[0], emb.device
    reward = torch.empty((B,), dtype=torch.float32, device=dev)
    discount = torch.empty((B,), dtype=torch.float32, device=dev)
    logits = torch.empty((B, net.A), dtype=torch.float32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    nxt = torch.empty((B, LATENT), dtype=torch.float32, device=dev)
    _L.check(getattr(_L.load(), net.RECURRENT)(net.w, _L.ptr(act), _L.ptr(emb), B, _L.ptr(reward), _L.ptr(discount),
                                               _L.ptr(logits), _L.ptr(value), _L.ptr(nxt), _L.stream_ptr()),
             net.RECURRENT)
    return reward, discount, logits, value, nxt


root_inference_fn, recurrent_inference_fn = root_inference, recurrent_inference


# ---------------------------------------------------------------------------------- reference params
_NET_CACHE: dict = {}


def rng_key_to_seed(rng_key) -> int:
    """The reference's ``rng_key`` argument -> this engine's 64-bit counter-RNG seed.  Accepts an int or a
    jax-style uint32[2] key (key data as a list / NumPy / torch array).  jax's threefry streams are not
    reproduced: the key only selects the engine's own noise stream, deterministically."""
    if isinstance(rng_key, (int, np.integer)):
        return int(rng_key) & ((1 << 64) - 1)
    k = np.asarray(rng_key.cpu() if isinstance(rng_key, torch.Tensor) else rng_key).astype(np.uint64).ravel()
    if k.size != 2:
        raise ValueError(f"rng_key must be an int or a uint32[2] key, got shape {k.shape}")
    return int((int(k[0]) << 32) | int(k[1]))


def _device_of(device) -> torch.device:
    """torch.device(device) as a tensor's ``.device`` states it: "cuda" is the current device, "cuda:0"."""
    d = torch.device(device)
    return torch.device(d.type, torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def cached_device_net(cache: dict, cls, params, device="cuda", obs_channels: int | None = None):
    """The reference's ``params`` argument -> a ``cls`` net, packed once per params object: ``cache`` (one per game)
    holds the one live weight set, which is what the reference's loops use.  Accepts what the reference passes around
    -- init_muzero_params' nested Flax tree, a flat ``"net/Layer/param"`` dict -- or a ``cls`` net.  An in-place
    update of the same tree re-packs (params_fingerprint)."""
    if isinstance(params, cls):
        return params
    fp = params_fingerprint(params)
    hit = cache.get(id(params))
    if hit is not None and hit[0] is params and hit[2] == fp and hit[1].buffer.device == _device_of(device):
        return hit[1]
    net = cls.from_params(flat_f32(params), device, obs_channels)
    prev = next(iter(cache.values()), None)
    if prev is not None and (prev[1].C, prev[1].A) == (net.C, net.A) and prev[1].buffer.shape == net.buffer.shape \
            and prev[1].buffer.device == net.buffer.device:
        # same shapes: the new weights go into the live net, so engines cached on it (game_agent.cached_engine) keep
        # their state, workspace and buffers across a training loop's iterations
        prev[1].buffer.copy_(net.buffer)
        prev[1].prepare()
        net = prev[1]
    cache.clear()
    cache[id(params)] = (params, net, fp)
    return net


def as_device_net(params, obs_channels: int | None = None, device="cuda") -> DeviceNet:
    """cached_device_net for det-MADN: the channel count is read from the representation's Dense_1 kernel (C - 6
    inputs) when not given."""
    return cached_device_net(_NET_CACHE, DeviceNet, params, device, obs_channels)


_VERSIONED = {}    # id(tree) -> (tree, version()): trees whose owner updates the leaves in place


def register_versioned_params(tree, version):
    """``tree``'s leaves are updated in place by an owner that counts its updates (training.OptState: the
    learner's steps): params_fingerprint of that tree is then the count, not an inference from the values."""
    _VERSIONED[id(tree)] = (tree, version)


def params_fingerprint(params) -> tuple:
    """Content fingerprint of a parameter tree, so an in-place update of the same dict / arrays between
    calls invalidates as_device_net's cache: a tree registered by its owner (register_versioned_params: the
    learner's live tree) by the owner's update count; otherwise per NumPy leaf a CRC32 of its bytes (~10 ms for
    the 11 MB det tree), the torch leaves (e.g. a learner's live parameters, which the fused AdamW kernel updates through
    raw pointers, so torch's version counters do not move) by their L2 norms, all in one multi-tensor kernel
    and one device-to-host copy."""
    hit = _VERSIONED.get(id(params))
    if hit is not None and hit[0] is params:
        return (("version", int(hit[1]())),)
    import zlib
    out, tens = [], []

    def walk(t, pre):
        if isinstance(t, dict):
            for k in sorted(t):
                walk(t[k], f"{pre}/{k}")
        elif isinstance(t, torch.Tensor):
            out.append((pre, tuple(t.shape), t.data_ptr()))
            tens.append(t.detach())
        else:
            a = np.ascontiguousarray(np.asarray(t))
            out.append((pre, zlib.crc32(a.view(np.uint8).reshape(-1)), a.shape))
    walk(params, "")
    if tens:
        norms = torch.stack([n.double() for n in torch._foreach_norm(tens)]).cpu().numpy()
        out.append(("norms", norms.tobytes()))
    return tuple(out)
