"""soa.py on the CPU: what DetMADNState, ClassicMADNState and DOGState get from their base -- the documented shape
and dtype of every field, the struct of addresses, gather / scatter of games, clone -- and the one make_rules behind
the three modules'."""
import ctypes

import numpy as np
import pytest
import torch

B = 5
GAMES = ("det", "classic", "dog")
# the documented layout (include/muz.h): 2-D field -> rows at P players, the 1-D fields, the dtypes that are not int8
LAYOUT = {
    "det": ({"board": lambda P: 56, "pins": lambda P: 4 * P, "action_set": lambda P: 6 * P},
            ("current_player", "reward", "done")),
    "classic": ({"board": lambda P: 56, "pins": lambda P: 4 * P}, ("current_player", "reward", "done", "die")),
    "dog": ({"board": lambda P: 56, "pins": lambda P: 4 * P, "deck": lambda P: 14, "hands": lambda P: 14 * P,
             "swap_choices": lambda P: 4},
            ("current_player", "round_starter", "phase", "hand_size", "reward", "done", "deal")),
}
DTYPES = {"done": torch.uint8, "deal": torch.int32}


def _module(game):
    from exploring_muzero_on_dog_amd import classic, detmadn, dog
    return {"det": detmadn, "classic": classic, "dog": dog}[game]


def _class(game):
    return getattr(_module(game), {"det": "DetMADNState", "classic": "ClassicMADNState", "dog": "DOGState"}[game])


def _state(game, P=4):
    """5 games built with state_from_host, every field different from game to game."""
    m = _module(game)
    rng = np.random.default_rng(7)
    pins = rng.integers(-1, 56, (B, P, 4)).astype(np.int8)
    board = rng.integers(-1, P, (B, 56)).astype(np.int8)
    per_game = lambda lo: (np.arange(B) + lo).astype(np.int8)            # noqa: E731
    rules = m.make_rules(P)
    if game == "det":
        st = m.state_from_host(pins, per_game(0) % P, rules, action_set=rng.integers(0, 5, (B, P, 6)).astype(np.int8),
                               done=per_game(0) % 2, reward=per_game(-2), board=board, device="cpu")
    elif game == "classic":
        st = m.state_from_host(pins, per_game(0) % P, rules, die=per_game(1), done=per_game(0) % 2,
                               reward=per_game(-2), board=board, device="cpu")
    else:
        st = m.state_from_host(dict(pins=pins, board=board, deck=rng.integers(0, 9, (B, 14)),
                                    hands=rng.integers(0, 5, (B, P, 14)), swap_choices=rng.integers(-1, 14, (B, 4)),
                                    current_player=per_game(0) % P, round_starter=per_game(1) % P, phase=per_game(0) % 2,
                                    hand_size=per_game(2), reward=per_game(-2), done=per_game(0) % 2,
                                    deal=np.arange(B) + 2 ** 31), rules, seed=11, device="cpu")
    for k in ("board", "pins"):
        cols = getattr(st, k).T.tolist()
        assert len({tuple(c) for c in cols}) == B, k
    return st


def _fields(game):
    rows, vec = LAYOUT[game]
    return tuple(rows) + vec


def _same(a, b, game):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in _fields(game))


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("P", [2, 4])
def test_alloc_shapes_and_dtypes(game, P):
    rules = _module(game).make_rules(P)
    extra = {"seed": 9} if game == "dog" else {}
    st = _class(game).alloc(3, P, rules, "cpu", **extra)
    rows, vec = LAYOUT[game]
    want = {k: ((r(P), 3), DTYPES.get(k, torch.int8)) for k, r in rows.items()}
    want.update({k: ((3,), DTYPES.get(k, torch.int8)) for k in vec})
    got = {k: (tuple(v.shape), v.dtype) for k, v in vars(st).items() if isinstance(v, torch.Tensor)}
    assert got == want
    assert all(getattr(st, k).is_contiguous() for k in want)
    assert st.batch == 3 and st.num_players == P and st.rules is rules and st.pins_bp().shape == (3, P, 4)
    if game == "dog":
        assert st.seed == 9


@pytest.mark.parametrize("game", GAMES)
def test_soa_holds_each_address_and_the_stride(game):
    st = _state(game)
    s = st.soa()
    assert [name for name, _ in s._fields_] == list(_struct_order(game)) + ["stride"]
    for k in _fields(game):
        assert getattr(s, k) == getattr(st, k).data_ptr(), k
    assert s.stride == st.batch == B


def _struct_order(game):
    return {"det": ("board", "pins", "current_player", "reward", "done", "action_set"),
            "classic": ("board", "pins", "current_player", "reward", "done", "die"),
            "dog": _fields("dog")}[game]


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("idx", [torch.tensor([3, 0, 4]), slice(1, 4)], ids=["index", "slice"])
def test_take_gathers_contiguous_columns(game, idx):
    st = _state(game)
    sub = st.take(idx)
    assert type(sub) is type(st) and sub.batch == 3
    for k in _fields(game):
        v, w = getattr(st, k), getattr(sub, k)
        assert w.is_contiguous() and w.dtype == v.dtype, k
        assert torch.equal(w, v[:, idx] if v.dim() == 2 else v[idx]), k
    assert sub.rules is st.rules and sub.num_players == st.num_players
    if game == "dog":
        assert sub.seed == st.seed == 11
    assert torch.equal(sub.pins_bp(), st.pins_bp()[idx])


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("idx", [torch.tensor([3, 0, 4]), slice(1, 4)], ids=["index", "slice"])
def test_put_into_a_clone_restores_equality(game, idx):
    st = _state(game)
    c = st.clone()
    for k in _fields(game):
        v = getattr(c, k)
        v[(slice(None), idx) if v.dim() == 2 else idx] = 101
    assert not _same(c, st, game)
    c.put(idx, st.take(idx))
    assert _same(c, st, game)


@pytest.mark.parametrize("game", GAMES)
def test_put_of_a_permuted_take_permutes_the_games(game):
    st = _state(game)
    perm = torch.tensor([3, 0, 4, 1, 2])
    c = st.clone()
    c.put(torch.arange(B), st.take(perm))
    for k in _fields(game):
        v, w = getattr(st, k), getattr(c, k)
        assert torch.equal(w, v[:, perm] if v.dim() == 2 else v[perm]), k
    assert not _same(c, st, game)
    c.put(perm, c.take(torch.arange(B)))     # and back
    assert _same(c, st, game)


@pytest.mark.parametrize("game", GAMES)
def test_clone_shares_no_storage(game):
    st = _state(game)
    c = st.clone()
    assert type(c) is type(st) and _same(c, st, game)
    assert c.rules is st.rules and c.num_players == st.num_players
    for k in _fields(game):
        assert getattr(c, k).data_ptr() != getattr(st, k).data_ptr(), k
        getattr(c, k).add_(1)
    assert _same(st, _state(game), game)
    assert all(not torch.equal(getattr(c, k), getattr(st, k)) for k in _fields(game))


def _bytes(rules):
    return ctypes.string_at(ctypes.addressof(rules), ctypes.sizeof(rules))


def test_make_rules_is_one_function():
    """The same arguments give the same muz_rules bytes in the three modules.  Det and classic share every det rule;
    DOG has no enable_start_on_1 / enable_bonus_turn_on_6 (its struct keeps them 0), so det is given them as False."""
    det, cla, dog = (_module(g) for g in GAMES)
    shared = dict(enable_teams=True, enable_initial_free_pin=True, enable_circular_board=False,
                  enable_start_blocking=True, enable_jump_in_goal_area=False, enable_friendly_fire=True,
                  must_traverse_start=True)
    pos = dict(num_players=3, layout=(True, False, True, True), distance=7, starting_player=2)
    assert set(shared) == set(det.DEFAULT_RULES) & set(cla.DEFAULT_RULES) & set(dog.DEFAULT_RULES)
    a = det.make_rules(**pos, **shared)
    assert _bytes(a) == _bytes(cla.make_rules(**pos, **shared))
    assert (a.num_players, a.distance, list(a.layout), a.starting_player) == (3, 7, [1, 0, 1, 1], 2)
    assert all(getattr(a, k) == int(v) for k, v in shared.items())
    assert a.enable_start_on_1 == 1 and a.enable_bonus_turn_on_6 == 1       # a module's own defaults still apply
    off = dict(enable_start_on_1=False, enable_bonus_turn_on_6=False)
    assert _bytes(det.make_rules(**pos, **shared, **off)) == _bytes(dog.make_rules(**pos, **shared))
    assert _bytes(det.make_rules()) == _bytes(cla.make_rules()) != _bytes(dog.make_rules())
    assert dog.make_rules().must_traverse_start == 1 and det.make_rules().must_traverse_start == 0


@pytest.mark.parametrize("game", GAMES)
def test_make_rules_refuses_an_unknown_rule(game):
    m = _module(game)
    with pytest.raises(TypeError, match="unknown rule"):
        m.make_rules(4, enable_flying_pins=True)
    foreign = {"det": "disable_joker", "classic": "disable_joker", "dog": "enable_dice_rethrow"}[game]
    with pytest.raises(TypeError, match=foreign):
        m.make_rules(4, **{foreign: True})
