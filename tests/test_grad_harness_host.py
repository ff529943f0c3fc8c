"""tests/grad_harness.py is the one witness of the GPU tests of the backward family: its primitives, held to their word on CPU tensors."""
import numpy as np
import pytest

import grad_harness as H
from grad_harness import F32, PAD, SENTINEL, Guarded, check, from_sm, outside_keeps_sentinel, same, to_sm

torch = pytest.importorskip("torch")


class P:
    """the counts check() cuts the per-stream rows to"""
    n_state, n_param, n_const = 2, 1, 0


def test_the_harness_imports_without_torch_at_module_level():
    assert "torch" not in vars(H)


@pytest.mark.parametrize("at", [PAD - 1, PAD + 24], ids=["just_before", "just_after"])
def test_one_float_written_next_to_the_middle_breaks_the_guards(at):
    g = Guarded((2, 3, 4), device="cpu")
    assert g.guards_kept() and g.untouched() and tuple(g.mid.shape) == (2, 3, 4) and g.buf.numel() == 2 * PAD + 24
    g.buf[at] = 0.0
    assert not g.guards_kept() and not g.untouched()


def test_one_float_written_in_the_middle_is_seen_and_leaves_the_guards():
    g = Guarded((5, 7), init=np.arange(35, dtype=F32).reshape(5, 7), device="cpu")
    assert g.untouched() and g.mid[4, 6] == 34.0
    g.mid[2, 3] += 1.0
    assert not g.untouched() and g.guards_kept()


def test_untouched_compares_bits():
    g = Guarded((4,), init=np.zeros(4, F32), device="cpu")
    g.mid[1] = -0.0
    assert not g.untouched()


def test_same_is_bitwise_with_nan_equal_to_nan():
    nan2 = np.array([0x7fc00001], np.uint32).view(F32)
    assert same([1.0, np.nan], [1.0, np.nan]) and same([np.nan], nan2)
    assert not same([0.0], [-0.0])
    assert not same(np.zeros((2, 3), F32), np.zeros((3, 2), F32)) and not same(np.zeros(3, F32), np.zeros(4, F32))
    assert not same([1.0], [np.nan]) and not same([1.0], [np.nextafter(F32(1.0), F32(2.0))])


def test_outside_keeps_sentinel_sees_one_row_outside_and_ignores_the_window():
    buf = np.full((3, 12, 2), SENTINEL, F32)
    buf[:, 4:9] = 1.0                                             # the window [4, 9): whatever it holds
    assert outside_keeps_sentinel(buf, 4, 5)
    for row in (3, 9, 0, 11):
        bad = buf.copy()
        bad[1, row, 1] = 0.0
        assert not outside_keeps_sentinel(bad, 4, 5), row
    assert not outside_keeps_sentinel(buf, 4, 4) and not outside_keeps_sentinel(buf, 5, 4)


def test_check_strict_fails_on_a_missing_key_and_lenient_skips_what_got_lacks():
    a = {"x": np.ones((2, 3, 1), F32), "state": np.ones((2, 3), F32)}
    check(P, a, dict(a), "equal", ("x", "state"), require=True)
    check(P, a, dict(a), "got lacks params", ("x", "state", "params"))
    with pytest.raises(AssertionError, match="params is missing"):
        check(P, a, dict(a), "strict", ("x", "state", "params"), require=True)
    with pytest.raises(AssertionError, match="state is missing"):
        check(P, a, {"x": a["x"]}, "strict, want lacks it", ("x", "state"), require=True)
    with pytest.raises(AssertionError, match="state is missing"):
        check(P, a, {"x": a["x"]}, "lenient, want lacks what got holds", ("x", "state"))


def test_check_compares_bits_and_cuts_per_stream_rows_to_the_graphs_counts():
    a = {"x": np.ones((2, 3, 1), F32), "state": np.ones((2, 3), F32), "consts": np.ones((1, 3), F32)}
    padded = dict(a, state=np.concatenate([a["state"], np.full((1, 3), 9.0, F32)]), consts=np.zeros((1, 3), F32))
    check(P, a, padded, "rows beyond n_state and the placeholder row of n_const = 0", ("x", "state", "consts"), require=True)
    with pytest.raises(AssertionError, match="x differs in 1 of 6"):
        check(P, a, dict(a, x=np.where(np.arange(6).reshape(2, 3, 1) == 4, -1.0, 1.0).astype(F32)), "one float", ("x",))
    with pytest.raises(AssertionError, match="state differs"):
        check(P, {"state": np.zeros((2, 3), F32)}, {"state": -np.zeros((2, 3), F32)}, "-0 against +0", ("state",))


def test_to_sm_and_from_sm_round_trip_at_a_row_offset():
    a = np.random.default_rng(3).standard_normal((5, 3, 2)).astype(F32)
    sm = to_sm(a, 12, 4, 7.0)
    assert sm.shape == (3, 12, 2) and same(sm[1, 4 + 2], a[2, 1]) and np.all(sm[:, :4] == 7.0) and np.all(sm[:, 9:] == 7.0)
    assert same(from_sm(sm, 5, 4), a) and from_sm(sm, 5, 4).flags["C_CONTIGUOUS"]
    assert to_sm(a, row0=4).shape == (3, H.up4(9), 2) and [H.up4(n) for n in (0, 1, 4, 5)] == [0, 4, 4, 8]


def test_launch_names_every_entry_point_itself():
    from zignal_amd import _capi as CA
    assert set(H.ENTRY.values()) <= set(CA.EXPORTS) and len(H.ENTRY) == 16       # every corner: 2 x 2 x 2 x 2
    for (ring, loss, window, rec), name in H.ENTRY.items():
        words = name.split("_")
        assert ("ring" in words) == ring and ("loss" in words) == loss and ("recording" in words) == rec, name
        assert name.endswith("_stream_major") == (window and not (rec and not ring)), name      # (the plain recording call takes the layout)
