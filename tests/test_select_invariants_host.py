"""The Gumbel search's considered-visit table (csrc/tree.hpp fill_considered_visits, the function k_gumbel_search's
lanes run once per search to fill the game's LDS row) through its host entry muz_considered_visits, against
seq_halving.get_sequence_of_considered_visits as oracle/mctx_gumbel.py restates it.  No GPU."""
import ctypes

from oracle import mctx_gumbel as G


def _lib():
    from exploring_muzero_on_dog_amd import lib as L
    return L, L.load()


def test_considered_visit_table_equals_mctx_sequence():
    """Every number of considered actions a 24-action root can have (0..24; the search passes
    min(max_num_considered, legal actions)) x every supported S (1..100), every index."""
    L, so = _lib()
    for m in range(25):
        for S in range(1, 101):
            out = (ctypes.c_uint8 * (S + 1))(*([0xEE] * (S + 1)))
            assert so.muz_considered_visits(m, S, out) == L.MUZ_OK
            assert tuple(out[:S]) == G.get_sequence_of_considered_visits(m, S), (m, S)
            assert out[S] == 0xEE, (m, S)     # nothing past the S entries


def test_considered_visit_table_refuses_what_the_search_refuses():
    L, so = _lib()
    out = (ctypes.c_uint8 * 128)()
    assert so.muz_considered_visits(16, 0, out) == L.MUZ_E_UNSUPPORTED
    assert so.muz_considered_visits(16, 101, out) == L.MUZ_E_UNSUPPORTED
    assert so.muz_considered_visits(-1, 50, out) == L.MUZ_E_INVALID
    assert so.muz_considered_visits(16, 50, None) == L.MUZ_E_INVALID
