"""libmuz.so loads and exports exactly what include/muz.h declares (CPU only: no compute calls)."""
import ctypes
import os
import re

import muzpkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muz.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(muz_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_entry_points():
    names = declared_functions()
    assert "muz_detmadn_step" in names and "muz_version" in names


def test_library_exports_every_declared_symbol():
    from exploring_muzero_on_dog_amd import lib as L
    assert os.path.exists(L.LIB_PATH), "libmuz.so not built"
    so = ctypes.CDLL(L.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(so, n)]
    assert not missing, missing
    # the python binding covers every declared symbol with a signature
    assert set(declared_functions()) <= set(L.SIGNATURES), set(declared_functions()) - set(L.SIGNATURES)


def test_library_is_gfx950_code():
    from exploring_muzero_on_dog_amd import lib as L
    data = open(L.LIB_PATH, "rb").read()
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in data   # offload bundle entry of the fat binary


def _al256(x):
    return (x + 255) & ~255


def _selfplay_bytes(n, S, C, A, tree):
    """The self-play carve: the search tree, then the per-turn arrays, each piece rounded up to 256 bytes."""
    n16 = (n + 15) // 16 * 16
    pieces = [tree, n16 * (56 * 64 + 512) * 4, n16 * C * 56 * 4] + [n * 4] * 5 + \
             [n16 * A * 4, n16 * 4, n16 * 256 * 4, n16 * 4, n16 * A * 4, n16 * 4, 64, n * 4, 64]
    return sum(_al256(p) for p in pieces)


# (n, S) -> bytes of every exported *_workspace_bytes function, as the layouts stood when the tree workspaces and the
# self-play carves were first shared (det self-play at 18 observation channels, classic at 7)
WORKSPACE_BYTES = {
    "muz_search_workspace_bytes": {
        (1, 1): 3584, (1, 50): 91392, (1, 100): 180992, (17, 1): 60928, (17, 50): 1553664, (17, 100): 3076864,
        (4096, 1): 14680064, (4096, 50): 374341632, (4096, 100): 741343232},
    "muz_stochastic_workspace_bytes": {
        (1, 1): 2832, (1, 50): 72216, (1, 100): 143016, (17, 1): 48144, (17, 50): 1227672, (17, 100): 2431272,
        (4096, 1): 11599872, (4096, 50): 295796736, (4096, 100): 585793536},
    "muz_dog_search_workspace_bytes": {
        (1, 1): 47744, (1, 50): 1135936, (1, 100): 2246336, (17, 1): 811648, (17, 50): 19310912, (17, 100): 38187712,
        (4096, 1): 195559424, (4096, 50): 4652793856, (4096, 100): 9200992256},
    "muz_selfplay_workspace_bytes": {
        (1, 1): 352512, (1, 50): 440320, (1, 100): 529920, (17, 1): 755968, (17, 50): 2248704, (17, 100): 3771904,
        (4096, 1): 103432704, (4096, 50): 463094272, (4096, 100): 830095872},
    "muz_classic_selfplay_workspace_bytes": {
        (1, 1): 310016, (1, 50): 379392, (1, 100): 450048, (17, 1): 659456, (17, 50): 1838848, (17, 100): 3042560,
        (4096, 1): 89604608, (4096, 50): 373801472, (4096, 100): 663798272},
}


def test_workspace_bytes_are_pinned():
    """Every exported *_workspace_bytes at n in {1, 17, 4096} x S in {1, 50, 100}: literal values, cross-checked
    against the layouts (det tree n(S+1)1792, classic n(S+1)1416, DOG n(S+1)22208 + 3328 n; the self-play carves'
    rounding of n to 16 rows and of every piece to 256 bytes)."""
    from exploring_muzero_on_dog_amd import lib as L
    so = L.load()
    for n in (1, 17, 4096):
        for S in (1, 50, 100):
            scfg = L.MuzSearchCfg(num_simulations=S, max_depth=S, max_num_considered=16)
            ccfg = L.MuzStochCfg(num_simulations=S, max_depth=S)
            got = {
                "muz_search_workspace_bytes": so.muz_search_workspace_bytes(n, ctypes.byref(scfg)),
                "muz_stochastic_workspace_bytes": so.muz_stochastic_workspace_bytes(n, S),
                "muz_dog_search_workspace_bytes": so.muz_dog_search_workspace_bytes(n, ctypes.byref(scfg)),
                "muz_selfplay_workspace_bytes": so.muz_selfplay_workspace_bytes(n, 18, ctypes.byref(scfg)),
                "muz_classic_selfplay_workspace_bytes":
                    so.muz_classic_selfplay_workspace_bytes(n, 7, ctypes.byref(ccfg)),
            }
            for name, value in got.items():
                assert value == WORKSPACE_BYTES[name][(n, S)], (name, n, S, value)
            det, cls = n * (S + 1) * 1792, n * (S + 1) * 1416
            assert got["muz_search_workspace_bytes"] == det
            assert got["muz_stochastic_workspace_bytes"] == cls
            assert got["muz_dog_search_workspace_bytes"] == n * (S + 1) * 22208 + n * 3328
            assert got["muz_selfplay_workspace_bytes"] == _selfplay_bytes(n, S, 18, 24, det)
            assert got["muz_classic_selfplay_workspace_bytes"] == _selfplay_bytes(n, S, 7, 4, cls)
    assert sorted(WORKSPACE_BYTES) == sorted(f for f in declared_functions() if f.endswith("_workspace_bytes"))


def test_version_string_without_gpu():
    from exploring_muzero_on_dog_amd import lib as L
    so = L.load()
    assert so.muz_version().startswith(b"libmuz")
    assert so.muz_error_string(L.MUZ_E_INVALID) == b"invalid argument"
