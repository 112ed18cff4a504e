"""The refusals of the classic self-play entry points (muz_classic_selfplay / _stream) and of the Gumbel det ones
(muz_detmadn_selfplay / _stream), in the style of tests/test_puct_selfplay_host.py, which covers the PUCT pair: every
call here is refused (or accepted with no game to play) before any launch, so it runs on a host without a GPU.  The
pointers are dummies that are never dereferenced.  The expected codes pin the order of the drivers' checks: where two
faults meet in one call, the one checked first decides between MUZ_E_INVALID and MUZ_E_UNSUPPORTED."""
import ctypes

import pytest

TRAJ_KEYS = ("obs", "act", "rew", "val", "pol", "mask", "player", "team", "discount", "idx")


class _Call:
    """One game's batch and streaming entry points.  ``null``: names of pointers passed as null -- "cfg", "w",
    "workspace", a trajectory key or a chance key; ``net``: fields of the network struct to override."""

    def __init__(self, game):
        from exploring_muzero_on_dog_amd import lib as L
        self.L, self.game = L, game
        self.so = L.load()
        self.raw = (ctypes.c_char * 128)()
        self.p = (ctypes.addressof(self.raw) + 15) & ~15        # 16-byte aligned, never dereferenced
        if game == "classic":
            from exploring_muzero_on_dog_amd import classic as E
            from exploring_muzero_on_dog_amd import stochastic as ST
            self.E, self.make_cfg, self.actions = E, ST.make_cfg, 4
            self.names = ("muz_classic_selfplay", "muz_classic_selfplay_stream")
            self.bytes_fn = self.so.muz_classic_selfplay_workspace_bytes
        else:
            from exploring_muzero_on_dog_amd import detmadn as E
            from exploring_muzero_on_dog_amd import mcts as M
            self.E, self.make_cfg, self.actions = E, M.make_cfg, 24
            self.names = ("muz_detmadn_selfplay", "muz_detmadn_selfplay_stream")
            self.bytes_fn = self.so.muz_selfplay_workspace_bytes

    def need(self, n, S, P=2):
        return self.bytes_fn(n, self.E.num_channels(P), ctypes.byref(self.make_cfg(S, 1)))

    def __call__(self, stream, n=1, games=None, P=2, S=50, D=25, null=(), net=None, T=10, stride=None,
                 ws_bytes=1 << 40, misaligned=False):
        L, null = self.L, ((null,) if isinstance(null, str) else tuple(null))
        rules = self.E.make_rules(P, **self.E.SELFPLAY_RULES)
        if self.game == "classic":
            w, st = L.MuzClassicNetW(), L.MuzClassicSoA()
            w.sdyn.act_film_tab = w.sdyn.chance_film_tab = self.p
            rows = ("board", "pins", "current_player", "reward", "done", "die")
        else:
            w, st = L.MuzNetW(), L.MuzDetSoA()
            rows = ("board", "pins", "current_player", "reward", "done", "action_set")
        w.obs_channels, w.num_actions = self.E.num_channels(P), self.actions
        for k, v in (net or {}).items():
            setattr(w, k, v)
        for k in rows:
            setattr(st, k, self.p)
        st.stride = max(n, 0) if stride is None else stride
        tr = L.MuzTraj()
        for k in TRAJ_KEYS:
            setattr(tr, k, None if k in null else self.p)
        tr.max_steps = T
        records = [tr]
        if self.game == "classic":
            ch = L.MuzTrajChance()
            ch.dice = None if "dice" in null else self.p
            ch.dice_dist = None if "dice_dist" in null else self.p
            records.append(ch)
        cfg = self.make_cfg(S, D)
        head = [rules, None if "w" in null else ctypes.byref(w), None if "cfg" in null else ctypes.byref(cfg), st]
        size = [n if games is None else games, n] if stream else [n]
        wsp = None if "workspace" in null else self.p + (4 if misaligned else 0)
        return getattr(self.so, self.names[stream])(*head, *records, *size, wsp, ws_bytes, None, None)


@pytest.fixture(scope="module")
def classic():
    return _Call("classic")


@pytest.fixture(scope="module")
def det():
    return _Call("det")


INVALID, UNSUPPORTED = "MUZ_E_INVALID", "MUZ_E_UNSUPPORTED"

# (case, the call's keywords, the code)
COMMON = [
    ("null cfg", dict(null="cfg"), INVALID),
    ("null w", dict(null="w"), INVALID),
    ("null cfg and w", dict(null=("cfg", "w")), INVALID),
    ("stride < lanes", dict(n=8, stride=7), INVALID),
    ("null workspace", dict(null="workspace"), INVALID),
    ("null tr.obs", dict(null="obs"), INVALID),
    ("null tr.idx", dict(null="idx"), INVALID),
    ("max_steps 0", dict(T=0), INVALID),
    ("num_simulations 0", dict(S=0), UNSUPPORTED),
    ("num_simulations 101", dict(S=101), UNSUPPORTED),
    ("max_depth 0", dict(D=0), UNSUPPORTED),
    ("max_depth 65", dict(D=65), UNSUPPORTED),
    ("negative n", dict(n=-1), INVALID),
    # two faults in one call: the arguments are checked before the search limits, the network before the arguments
    ("null workspace, num_simulations 0", dict(null="workspace", S=0), INVALID),
    ("null tr.idx, max_depth 65", dict(null="idx", D=65), INVALID),
    ("workspace too small, num_simulations 101", dict(ws_bytes=0, S=101), UNSUPPORTED),
]
CLASSIC = COMMON + [
    ("obs_channels != 2P + 3", dict(net=dict(obs_channels=11)), UNSUPPORTED),
    ("obs_channels out of range", dict(net=dict(obs_channels=6)), UNSUPPORTED),
    ("num_actions 24", dict(net=dict(num_actions=24)), UNSUPPORTED),
    ("null ch.dice", dict(null="dice"), INVALID),
    ("null ch.dice_dist", dict(null="dice_dist"), INVALID),
    ("obs_channels != 2P + 3, null workspace", dict(net=dict(obs_channels=11), null="workspace"), UNSUPPORTED),
    ("obs_channels != 2P + 3, null cfg", dict(net=dict(obs_channels=11), null="cfg"), INVALID),
    ("null ch.dice, num_simulations 0", dict(null="dice", S=0), INVALID),
]
DET = COMMON + [
    ("obs_channels != 8P + 2", dict(net=dict(obs_channels=34)), UNSUPPORTED),
    ("num_actions 4", dict(net=dict(num_actions=4)), UNSUPPORTED),
    ("misaligned workspace", dict(misaligned=True), INVALID),
    ("obs_channels != 8P + 2, null workspace", dict(net=dict(obs_channels=34), null="workspace"), UNSUPPORTED),
    ("obs_channels != 8P + 2, null cfg", dict(net=dict(obs_channels=34), null="cfg"), INVALID),
]


@pytest.mark.parametrize("stream", [False, True], ids=["batch", "stream"])
@pytest.mark.parametrize("case,kw,code", CLASSIC, ids=[c[0] for c in CLASSIC])
def test_classic_selfplay_refusals(classic, case, kw, code, stream):
    assert classic(stream, **kw) == getattr(classic.L, code)


@pytest.mark.parametrize("stream", [False, True], ids=["batch", "stream"])
@pytest.mark.parametrize("case,kw,code", DET, ids=[c[0] for c in DET])
def test_gumbel_selfplay_refusals(det, case, kw, code, stream):
    assert det(stream, **kw) == getattr(det.L, code)


@pytest.mark.parametrize("game", ["classic", "det"])
def test_selfplay_workspace_one_byte_short_is_refused(game, request):
    """One byte less than the game's workspace size is MUZ_E_INVALID at every (n, S); exactly that size passes every
    check (a stream of no games, or a batch of none, returns MUZ_OK before any launch); negative game counts are
    invalid."""
    call = request.getfixturevalue(game)
    L = call.L
    for n in (1, 17, 4096):
        for S in (1, 50, 100):
            need = call.need(n, S)
            kw = dict(n=n, S=S, D=min(S, 64))
            assert call(False, ws_bytes=need - 1, **kw) == L.MUZ_E_INVALID, (n, S)
            assert call(True, ws_bytes=need - 1, **kw) == L.MUZ_E_INVALID, (n, S)
            assert call(True, games=0, ws_bytes=need - 1, **kw) == L.MUZ_E_INVALID, (n, S)
            assert call(True, games=0, ws_bytes=need, **kw) == L.MUZ_OK, (n, S)
            need0 = call.need(0, S)
            assert call(False, n=0, S=S, D=1, ws_bytes=need0) == L.MUZ_OK
            assert call(True, n=0, S=S, D=1, ws_bytes=need0) == L.MUZ_OK
            assert call(False, n=0, S=S, D=1, ws_bytes=need0 - 1) == L.MUZ_E_INVALID
    assert call(True, n=4, games=-1) == L.MUZ_E_INVALID
    assert call(True, n=-1, games=4) == L.MUZ_E_INVALID


# muz_classic_selfplay_workspace_bytes at (n, obs_channels, num_simulations)
PINNED_BYTES = {(0, 11, 8): 512, (1, 11, 1): 324352, (16, 11, 50): 1476864, (17, 7, 100): 3042560}


def test_classic_selfplay_workspace_bytes_are_pinned(classic):
    from exploring_muzero_on_dog_amd import stochastic as ST
    got = {(n, C, S): classic.bytes_fn(n, C, ctypes.byref(ST.make_cfg(S, 1)))
           for n, C, S in ((0, 11, 8), (1, 11, 1), (16, 11, 50), (17, 7, 100))}
    assert got == PINNED_BYTES
    cfg = ST.make_cfg(8, 1)
    assert classic.bytes_fn(-1, 11, ctypes.byref(cfg)) == -1
    assert classic.bytes_fn(4, 11, None) == -1
    assert classic.bytes_fn(4, 11, ctypes.byref(ST.make_cfg(0, 1))) == -1
