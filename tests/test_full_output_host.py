"""The whole-output checker without a GPU: it finds single-bit flips where kernels go wrong (first and last stream, both sides of a slice
seam, the last sample, inside a tile) at the right (stream, sample), passes an exact copy and NaNs of any payload; and every leg of
test_full_output_gpu.py resolves to the kernel it is listed for."""
import os

import numpy as np
import pytest

import full_check as FC
import full_legs as FL

SEED = 20241015
NS, T, TILE, K = 300, 64, 100, 64             # slices of 64 streams: seams at 64, 128, ...; tiles of 100 streams: slices straddle them


def reference(workload="cascade6", seed=SEED):
    return FL.reference(workload, seed, T)


def layouts(want_sm):
    """the oracle's own output as the three device layouts hold it: stream-major, time-major rows, tiles"""
    rows = np.ascontiguousarray(want_sm.transpose(1, 0, 2))
    w = want_sm.shape[2]
    tiles = np.ascontiguousarray(want_sm.reshape(NS // TILE, TILE, T, w).transpose(0, 2, 1, 3))
    return {"sm": want_sm.copy(), "rows": rows, "tiles": tiles}


def legs_of(arrs, x=None):
    fi = (lambda s0, s1: x[s0:s1]) if x is not None else None
    return [FC.Leg("sm", "k_sm", FC.stream_major(arrs["sm"]), fi), FC.Leg("rows", "k_rows", FC.rows(arrs["rows"]), fi),
            FC.Leg("tiles", "k_tiles", FC.tiles(arrs["tiles"]), fi)]


def flip(arrs, layout, s, t, w=0, bit=0):
    a = arrs[layout]
    idx = (s, t, w) if layout == "sm" else ((t, s, w) if layout == "rows" else (s // TILE, t, s % TILE, w))
    a.view(np.uint32)[idx] ^= np.uint32(1 << bit)


@pytest.fixture(scope="module")
def oracle_out():
    x, want = reference()(0, NS)
    assert np.isfinite(want).all()
    return x, want


def test_exact_copies_pass(oracle_out):
    x, want = oracle_out
    rep = FC.check(legs_of(layouts(want)), reference(), NS, K, threads=4)
    assert rep.ok and [r.checked_streams for r in rep.legs] == [NS] * 3, str(rep)


@pytest.mark.parametrize("s,t", [(0, 0), (NS - 1, 17), (63, 5), (64, 5), (127, T - 1), (128, 0), (150, 33), (199, T - 1), (200, 1)],
                         ids=["first-stream", "last-stream", "before-seam", "after-seam", "last-sample", "seam-t0", "inside-tile",
                              "tile-end", "tile-start"])
@pytest.mark.parametrize("layout", ["sm", "rows", "tiles"])
def test_single_bit_flips_are_found_where_they_are(oracle_out, layout, s, t):
    _, want = oracle_out
    for bit in (0, 31):                                         # the lowest mantissa bit and the sign
        arrs = layouts(want)
        flip(arrs, layout, s, t, bit=bit)
        rep = FC.check(legs_of(arrs), reference(), NS, K, threads=3)
        assert not rep.ok
        for r in rep.legs:
            if r.leg.name == layout:
                assert (r.bad_streams, r.first) == (1, (s, t, 0)), r.report()
                assert r.input_equal is None                     # (no device input to compare: said so)
                assert f"stream {s} sample {t}" in r.report() and "k_" + layout in r.report()
            else:
                assert r.bad_streams == 0, r.report()


def test_many_mismatches_report_the_first_and_count_streams(oracle_out):
    x, want = oracle_out
    arrs = layouts(want)
    for s, t in ((250, 3), (70, 40), (70, 2), (299, 63)):
        flip(arrs, "rows", s, t, bit=7)
    rep = FC.check(legs_of(arrs, x), reference(), NS, K, threads=4)
    r = rep.legs[1]
    assert (r.bad_streams, r.first, r.input_equal) == (3, (70, 2, 0), True), r.report()
    assert "equal to the host-generated" in r.report()


def test_a_generator_slip_is_told_from_a_kernel_slip(oracle_out):
    x, want = oracle_out
    arrs = layouts(want)
    flip(arrs, "sm", 130, 9)
    xd = x.copy()
    xd.view(np.uint32)[140, 20, 0] ^= 1                        # the device input of the same slice differs too
    rep = FC.check([FC.Leg("sm", "k_sm", FC.stream_major(arrs["sm"]), lambda s0, s1: xd[s0:s1])], reference(), NS, K, threads=2)
    assert rep.legs[0].input_equal is False and "DIFFERENT" in str(rep)


def test_nan_payloads_compare_equal_and_nan_against_numbers_does_not():
    a = np.zeros((3, 4, 2), np.float32)
    b = a.copy()
    a.view(np.uint32)[0, 1, 0] = 0x7FC00000
    b.view(np.uint32)[0, 1, 0] = 0xFFC00123                    # other sign, other payload
    a.view(np.uint32)[2, 3, 1] = 0x7F800001                    # a signalling NaN
    b.view(np.uint32)[2, 3, 1] = 0x7FFFFFFF
    assert not FC.mismatch(a, b).any()
    b[1, 0, 0] = np.nan
    a.view(np.uint32)[2, 0, 0] = 0x80000000                     # -0 against +0 differs
    m = FC.mismatch(a, b)
    assert m.sum() == 2 and m[1, 0, 0] and m[2, 0, 0]
    assert FC._first(m, 10) == (2, (11, 0, 0))


def test_multi_slot_outputs_report_the_slot():
    """the complex one-pole's (re, im) frames: a flip in the imaginary slot"""
    x, want = FL.reference("c32onepole", SEED, T)(0, NS)
    assert want.shape == (NS, T, 2) and np.isfinite(want).all()
    arrs = layouts(want)
    flip(arrs, "tiles", 101, 50, w=1, bit=3)
    rep = FC.check(legs_of(arrs), FL.reference("c32onepole", SEED, T), NS, K, threads=4)
    assert [(r.bad_streams, r.first) for r in rep.legs] == [(0, None), (0, None), (1, (101, 50, 1))], str(rep)


def test_slices_and_threads_stay_bounded(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert FC.n_threads() == min(3, len(os.sched_getaffinity(0)))
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert 1 <= FC.n_threads() <= 16
    for T_, w, tile in ((4096, 1, 0), (4096, 4, 4096), (4096, 2, 8192), (24, 1, 8192), (4096, 1, 8192)):
        k = FC.slice_streams(T_, w, tile)
        assert k * T_ * w * 4 <= FC.SLICE_BYTES and (not tile or tile % k == 0)


def test_every_leg_resolves_to_its_kernel(monkeypatch):
    """a planner change that moves a leg to another body fails here first; the second variant is another kernel"""
    monkeypatch.setenv("FLOWZ_HIP_AUTOTUNE", "0")
    monkeypatch.setenv("FLOWZ_HIP_NO_PLAN_CACHE", "1")
    seen = set()
    for name, pri, workload, seed, ns, T_, legs in FL.GROUPS:
        assert pri in "abc" and workload in FL.WORKLOADS
        prog = FL.program(workload)
        for layout, tile, kernel in legs:
            assert (name, layout) not in seen
            seen.add((name, layout))
            assert FL.kernel_name(prog, layout, ns, T_, tile) == kernel, (name, layout)
            assert FL.kernel_name(prog, layout, ns, T_, tile, FL.SECOND[layout]) != kernel, (name, layout)
    # the groups of one workload and stream count that do not share an oracle pass use different seeds
    keys = [(g[2], g[3], g[4]) for g in FL.GROUPS]
    assert len(set(keys)) == len(keys)
