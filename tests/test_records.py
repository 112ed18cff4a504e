"""records.py on the CPU: the record dict of every engine (keys, dtypes, shapes), its view as muz_traj /
muz_traj_chance, and the reference-shaped copies."""
import pytest
import torch

KEYS = ("obs", "act", "rew", "val", "pol", "mask", "player", "team", "discount", "idx")


def _R():
    from exploring_muzero_on_dog_amd import records as R
    return R


def _expected(n, T, C, A, chance):
    i32, f32 = torch.int32, torch.float32
    want = {"obs": ((n, T, C, 56), torch.int8), "act": ((n, T), i32), "rew": ((n, T), i32), "val": ((n, T), f32),
            "pol": ((n, T, A), f32), "mask": ((n, T), f32), "player": ((n, T), i32), "team": ((n, T), i32),
            "discount": ((n, T), i32), "idx": ((n,), i32)}
    if chance:
        want.update(dice=((n, T), i32), dice_dist=((n, T, chance), f32))
    return want


@pytest.mark.parametrize("C,A,chance", [(18, 24, None), (34, 24, None), (7, 4, 6), (11, 4, 6), (34, 806, None)],
                         ids=["det-2p", "det-4p", "classic-2p", "classic-4p", "dog"])
def test_alloc_records_keys_dtypes_shapes(C, A, chance):
    R = _R()
    n, T = 3, 5
    buf = R.alloc_records(n, T, C, A, device="cpu", chance=chance)
    assert {k: (tuple(v.shape), v.dtype) for k, v in buf.items()} == _expected(n, T, C, A, chance)
    assert all(v.device.type == "cpu" and v.is_contiguous() for v in buf.values())
    assert R.RECORD_KEYS == KEYS and set(R.REFERENCE_DTYPES) == set(KEYS)
    assert R.REFERENCE_DTYPES["obs"] == torch.float32
    assert all(R.REFERENCE_DTYPES[k] == buf[k].dtype for k in KEYS if k != "obs")


def test_reference_dtypes_are_one_object():
    from exploring_muzero_on_dog_amd import game_agent as GA
    from exploring_muzero_on_dog_amd import game_agent_dog as GD
    R = _R()
    assert GA.REFERENCE_DTYPES is R.REFERENCE_DTYPES and GD.REFERENCE_DTYPES is R.REFERENCE_DTYPES
    assert GA.reference_buffers is R.reference_buffers


def test_as_traj_puts_each_pointer_in_its_field():
    R = _R()
    buf = R.alloc_records(2, 7, 11, 4, device="cpu", chance=6)
    t = R.as_traj(buf, 7)
    assert t.max_steps == 7
    ptrs = {k: getattr(t, k) for k in KEYS}
    assert ptrs == {k: buf[k].data_ptr() for k in KEYS}
    assert len(set(ptrs.values())) == len(KEYS) and all(ptrs.values())
    ch = R.as_traj_chance(buf)
    assert (ch.dice, ch.dice_dist) == (buf["dice"].data_ptr(), buf["dice_dist"].data_ptr())
    assert R.as_traj(buf).max_steps == 0                       # packed rows carry no step bound
    with pytest.raises(KeyError):
        R.as_traj({k: v for k, v in buf.items() if k != "team"}, 7)
    empty = R.alloc_records(0, 7, 11, 4, device="cpu", chance=6)
    assert all(not getattr(R.as_traj(empty, 7), k) for k in KEYS)


def test_stats_dict_and_cached():
    from exploring_muzero_on_dog_amd import lib as L
    R = _R()
    st = L.MuzSpStats()
    st.turns, st.searches, st.search_ms, st.total_ms = 3, 17, 0.5, 2.0
    assert R.stats_dict(st, True) == {"turns": 3, "searches": 17, "search_ms": 0.5, "total_ms": 2.0}
    assert R.stats_dict(st, False) is None

    class Eng:
        def __init__(self, net):
            self.net = net
    cache, net_a, net_b, made = {}, object(), object(), []

    def make(net):
        made.append(net)
        return Eng(net)
    e1 = R.cached(cache, "k", net_a, lambda: make(net_a))
    assert R.cached(cache, "k", net_a, lambda: make(net_a)) is e1 and len(made) == 1
    e2 = R.cached(cache, "k", net_b, lambda: make(net_b))       # same key, another weight set: rebuilt
    assert e2 is not e1 and list(cache.values()) == [e2]
    e3 = R.cached(cache, "k2", net_b, lambda: make(net_b))      # another key: the cache holds one engine
    assert list(cache) == ["k2"] and cache["k2"] is e3 and len(made) == 3


def test_reference_buffers_restores_the_initial_rows_past_idx():
    R = _R()
    n, T = 3, 5
    buf = R.alloc_records(n, T, 7, 4, device="cpu", chance=6)
    g = torch.Generator().manual_seed(0)
    for k, v in buf.items():
        v.copy_(torch.randint(1, 5, v.shape, generator=g).to(v.dtype))
    buf["idx"].copy_(torch.tensor([0, 2, T], dtype=torch.int32))
    keep = {k: v.clone() for k, v in buf.items()}
    dt = dict(R.REFERENCE_DTYPES, dice=torch.int32, dice_dist=torch.float32)
    out = R.reference_buffers(buf, dt)
    assert set(out) == set(buf)
    for k, v in buf.items():
        assert torch.equal(v, keep[k]), k                       # the engine's buffers are left alone
        assert out[k].dtype == dt[k] and out[k].data_ptr() != v.data_ptr()
    assert torch.equal(out["idx"], keep["idx"])
    for i, L_ in enumerate((0, 2, T)):
        for k in out:
            if k == "idx":
                continue
            assert torch.equal(out[k][i, :L_], keep[k][i, :L_].to(dt[k])), k
            assert (out[k][i, L_:] == (-1 if k == "team" else 0)).all(), k
    assert out["obs"].dtype == torch.float32
    assert R.reference_buffers(buf, dict(dt, obs=torch.int8))["obs"].dtype == torch.int8
