"""fz_run_block_far_stream_major without a GPU: its scope and the reasons of what it refuses, the argument checks one by one, the
kernels for gfx950 (no scratch, the LDS bytes of the stated formula, G, R and lanes of the static rule, no contraction), the committed
kernel manifest, the number of random graphs the GPU file runs, and the old door, which keeps refusing in its old words."""
import ctypes

import pytest

import delay_cells as DC
import far_sm_forward as FF
from far_sm_graphs import AsRingFamily, far_entry_points
from grad_host_harness import ADJOINT, FakeCall, assert_no_contraction, code_objects, invalid, kernel_ops, recipe_of, replay, write_manifest
from graphs import DEL, IN, add, fb, lit, mod, mul, seq
from zignal_amd import _capi as C
from zignal_amd import flowz as F

NEW_EXPORTS = ("fz_run_block_far_stream_major", "fz_program_far_stream_major_check", "fz_program_far_stream_major_resources",
               "fz_program_far_stream_major_kernel_symbol", "fz_program_far_stream_major_source")
OLD_WORDS = "stream-major frames: delay lines beyond 256 samples are not supported"


def test_the_abi_exports_the_call_and_its_inspectors():
    for name in NEW_EXPORTS:
        assert hasattr(C.lib, name), name
    hdr = open(__file__.replace("tests/test_far_sm_forward_host.py", "include/flowz_hip.h")).read()
    assert all(name + "(" in hdr for name in NEW_EXPORTS)


# ---- scope ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FF.GRAPHS))
def test_every_graph_is_accepted(name):
    p = FF.prog(name)
    assert p.max_delay == FF.DEEPEST[name] > DC.LDS_MAX
    assert p.far_stream_major_supported() and p.far_stream_major_unsupported_reason() == ""
    assert FF.SYMBOL.match(p.far_stream_major_kernel_symbol())
    src = p.far_stream_major_source()
    assert "#define FZ_FLAGS %du" % FF.FAR_SM in src and "#define FZ_P 1\n" in src and "fz_far_sm_args" in src
    assert "#define FZ_RING_G 0 " in src                            # (LDS rings read in place, as in the short stream-major body)


def refused(p, word):
    assert not p.far_stream_major_supported()
    why = p.far_stream_major_unsupported_reason()
    assert word in why, why
    res = C.KernelResources()
    assert C.lib.fz_program_far_stream_major_resources(p._h, ctypes.byref(res)) == C.FZ_E_UNSUPPORTED and word in C.last_error()
    assert C.lib.fz_program_far_stream_major_kernel_symbol(p._h, None, 0) == C.FZ_E_UNSUPPORTED
    assert C.lib.fz_run_block_far_stream_major(p._h, 1 << 40, 2 << 40, 3 << 40, None, 64, 16, 0, 16, None) == C.FZ_E_UNSUPPORTED and word in C.last_error()
    return why


def test_each_refused_class_gets_its_reason():
    far = DC.sexpr("fb", (300,))
    refused(F.compile(F.from_sexpr(far), in_dtypes=["f32"]), "typed programs (fz_compile_typed)")
    refused(F.compile(F.from_sexpr(far), in_dtypes=["cf32"]), "typed programs (fz_compile_typed)")
    refused(F.compile(F.from_sexpr(fb(add(mul(mod(0), DEL(1, 300)), IN(2))))), "sample-rate modulators (fz_modulator)")
    # three LDS rings of 256 samples and a far line: 768 slots x 64 lanes x 4 bytes pass a workgroup's LDS before the shortest patch
    big = F.compile(F.from_sexpr(seq(DC.sexpr("fb", (256,)), DC.sexpr("fb", (256,)), DC.sexpr("fb", (256,)), far)))
    why = refused(big, "do not fit the 163840 bytes of LDS of a workgroup")
    assert "(768 samples)" in why and "a patch of 16 rows of 2 wires, %d bytes per 64 lanes" % (768 * 256 + 64 * (4 * 16 * 2 + 16)) in why
    # two such rings fit: 64 lanes
    ok = F.compile(F.from_sexpr(seq(DC.sexpr("fb", (256,)), DC.sexpr("fb", (256,)), far)))
    assert ok.far_stream_major_supported() and FF.geometry(ok) == FF.rule(ok) == (16, 32, 64)
    assert C.lib.fz_program_far_stream_major_check(None) == C.FZ_E_INVALID


@pytest.mark.parametrize("tmpl,args", [("fb", (8,)), ("fb", (40,)), ("mixed", (3, 40)), ("ff", (256,))])
def test_a_graph_without_a_far_line_runs_the_stream_major_default_kernel(tmpl, args):
    p = F.compile(F.from_sexpr(DC.sexpr(tmpl, args)))
    sm = F.make_variant(0, 0, 0, DC.SM)
    assert p.far_stream_major_supported()
    sym = p.far_stream_major_kernel_symbol()
    assert sym == p.kernel_symbol(sm) and sym.startswith("fz_block_kernel_p")
    P, U, B, flags = (int(v) for v in DC._NAME.match(p.kernel_name(sm)).groups()[:4])
    assert p.far_stream_major_source() == p.source(F.make_variant(P, U, B, flags)) and "fz_far_sm_args" not in p.far_stream_major_source()
    assert p.far_stream_major_resources() == p.kernel_resources(sm, 1 << 20, 1 << 20)


def test_the_old_door_keeps_refusing_in_its_old_words():
    p = FF.prog("far_comb")
    sm = F.make_variant(0, 0, 0, DC.SM)
    with pytest.raises(F.FlowzError, match=OLD_WORDS):
        p.kernel_name(sm)
    with pytest.raises(F.FlowzError, match=OLD_WORDS):
        p.build(sm, 64, 64)
    rc = C.lib.fz_run_block_stream_major(p._h, 1 << 40, 2 << 40, 3 << 40, None, 64, 64, 0, 64, None, None)
    if C.lib.fz_device_count() == 0:                                # (that call asks for the device before it plans)
        assert rc == C.FZ_E_NO_DEVICE
    else:
        assert rc == C.FZ_E_UNSUPPORTED and OLD_WORDS in C.last_error()
    # and a caller's variant that names the new kernel's reserved bits stays refused
    for flags in (FF.FAR_SM, FF.FAR_SM | DC.SM, 1 << 18, 1):
        with pytest.raises(F.FlowzError, match="reserved"):
            p.kernel_name(F.make_variant(0, 0, 0, flags))


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far_comb", "far_mixed", "far_two_in", "two_out"])
def test_argument_checks_fail_one_by_one_with_their_reason(name):
    p = FF.prog(name)
    with far_entry_points():
        b = FakeCall(AsRingFamily(p), 1000, 40, ring=True, window=(48, 0))      # (its addresses: in_, out_grad as out, state, params)

    def run(ns=1000, rows=48, row0=0, T=40, **over):
        a = dict(in_=b.addr["in_"], out=b.addr["out_grad"], state=b.addr["state"], params=b.addr["params"] if p.n_param else None)
        a.update(over)
        return C.lib.fz_run_block_far_stream_major(p._h, a["in_"], a["out"], a["state"], a["params"], ns, rows, row0, T, None)

    assert invalid(C.lib.fz_run_block_far_stream_major(None, 1 << 40, 2 << 40, 3 << 40, None, 64, 48, 0, 40, None), "null program")
    assert invalid(run(rows=0, T=0), "rows_total must be > 0")
    # an empty block is FZ_OK and touches nothing, whatever the pointers
    assert run(T=0) == C.FZ_OK and run(ns=0) == C.FZ_OK and run(T=0, in_=None, out=None, state=None) == C.FZ_OK
    assert invalid(run(T=0xFFFFFFFF), "n_samples must be below 2^32 - 1")
    assert invalid(run(row0=12, T=40), "reaches beyond rows_total = 48")
    assert invalid(run(T=49), "reaches beyond rows_total")
    # the alignment rule names the first side that is off the 16-byte grid, for rows_total and for row0
    for rows, row0 in ((49, 0), (50, 0), (48, 1), (48, 2)):
        side = next((sd for sd, w in (("in", p.n_in), ("out", p.n_out)) if (rows * w) % 4 or (row0 * w) % 4), None)
        if side:
            assert invalid(run(rows=rows, row0=row0, T=40), side + ": rows_total x wires and row0 x wires must be multiples of 4 on a float32 side"), (rows, row0)
    assert run(rows=49) == C.FZ_E_INVALID and run(row0=1, T=40) == C.FZ_E_INVALID     # (an odd count is off the grid of every graph here)
    for key, what in (("out", "out is null but the graph has output wires"), ("in_", "in is null but the graph has input wires"),
                      ("state", "state is null but the graph has delay lines")):
        assert invalid(run(**{key: None}), what)
    if p.n_param:
        assert invalid(run(params=None), "params is null but the graph has per-stream coefficients")
    for key in ("in_", "out", "state"):
        assert invalid(run(**{key: b.addr["state"] + 4}), "device pointers must be 16-byte aligned")
    assert run(ns=1 << 30) == C.FZ_E_UNSUPPORTED and "2^30 streams or more" in C.last_error()
    # what passes every check stops at the missing device (with one, fake addresses are not launched on)
    if C.lib.fz_device_count() == 0:
        assert run() == C.FZ_E_NO_DEVICE, C.last_error()
        assert run(row0=8, T=40) == C.FZ_E_NO_DEVICE, C.last_error()
        assert run(ns=1, rows=4, T=1) == C.FZ_E_NO_DEVICE, C.last_error()


# ---- the kernels for gfx950 --------------------------------------------------------------------------------------------------------------------
EXPECTED = {"far_comb": (16, 32, 256), "far_tap1": (8, 32, 256), "far_two_in": (16, 16, 256), "far_mixed": (16, 32, 128),
            "taps257_128_9_3": (4, 32, 256), "mixed3_40_300": (16, 32, 128), "two_out": (16, 16, 256)}


@pytest.mark.parametrize("name", sorted(FF.GRAPHS))
def test_kernel_resources_and_the_static_rule(name):
    p = FF.prog(name)
    G, R, block = FF.geometry(p)
    assert (G, R, block) == FF.rule(p) and block in (64, 128, 256) and G in (4, 8, 16) and R % G == 0 and R % 4 == 0
    assert 2 * G <= min(FF.far_reads(p)) and 2 * G * len(FF.far_reads(p)) <= FF.READ_REGS
    if name in EXPECTED:
        assert (G, R, block) == EXPECTED[name]
    r = p.far_stream_major_resources()
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["unroll"] == G, r
    assert r["lds_bytes"] == FF.lds_bytes(p, block, R) <= FF.LDS_BYTES, r
    src = p.far_stream_major_source()
    assert "#define FZ_R %d\n" % R in src and "#define FZ_U %d\n" % G in src and "#define FZ_BLOCK %d\n" % block in src


def test_the_lds_formula_in_numbers():
    assert FF.prog("far_comb").far_stream_major_resources()["lds_bytes"] == 4 * 64 * (4 * 32 * 2 + 16) == 69632
    assert FF.lds_slots(FF.prog("far_mixed")) == 32 and FF.prog("far_mixed").far_stream_major_resources()["lds_bytes"] == 4 * 32 * 128 + 2 * 17408


@pytest.mark.parametrize("name,divides", [("far_comb", False), ("far_mixed", False), ("far_adjacent", True), ("gated", False)])
def test_no_contraction_no_barrier_no_atomic(monkeypatch, tmp_path, name, divides):
    _, r, ops, every = kernel_ops(monkeypatch, tmp_path, FF.GRAPHS[name](), "far_stream_major_resources")
    assert r["scratch_bytes"] == 0
    assert_no_contraction(every, divides=divides, lds=True)
    assert "v_mul_f32_e32" in ops or "v_mul_f32_e64" in ops
    assert "v_readfirstlane_b32" in every                           # (the phase of the ring, once per line)


# ---- the kernel manifest of the GPU tests -------------------------------------------------------------------------------------------------
def test_the_committed_manifest_holds_the_kernels_the_gpu_tests_launch():
    recs = FF.manifest_variants()
    got = sorted(v[:4] for v in recs if v[3] == FF.FAR_SM)
    named = [FF.geometry(FF.prog(n)) for n in sorted(FF.GRAPHS)]
    rand = [FF.geometry(F.compile(F.from_sexpr(g))) for _, g, _, _ in FF.random_graphs()]
    assert got == sorted((R, G, block, FF.FAR_SM) for G, R, block in named + rand)
    assert len({(v[:4], v[4]) for v in recs if v[3] == FF.FAR_SM}) == len(FF.GRAPHS) + FF.RANDOM_KEPT
    # nothing else but the time-major forward kernels compared with, and the stream-major kernel of the graph without a far line
    others = [v for v in recs if v[3] != FF.FAR_SM]
    assert all(not (v[3] & ADJOINT) and v[0] in (1, 2, 4) for v in others) and len({(v[:4], v[4]) for v in others if v[3] & DC.SM}) == 1
    counts = replay(FF.MANIFEST)
    assert counts["failed"] == 0 and counts["records"] == len({(v[:4], v[4]) for v in recs}), counts


def test_a_manifest_cannot_ask_for_a_kernel_the_call_would_not_make(tmp_path):
    """one field off the rule -- G, R, the lanes, a flag more or less --, or a graph without a far line: counted as failed, nothing built"""
    p = FF.prog("far_comb")
    G, R, block = FF.geometry(p)
    assert (G, R, block) == (16, 32, 256)
    recipe = recipe_of(FF.GRAPHS["far_comb"]())
    assert (R, G, block, FF.FAR_SM, recipe) in FF.manifest_variants()
    assert F.compile(F.from_sexpr(DC.sexpr("fb", (40,)))).far_stream_major_supported()
    bad = [(R, 8, block, FF.FAR_SM, recipe), (R, 4, block, FF.FAR_SM, recipe), (R, 32, block, FF.FAR_SM, recipe), (R, 0, block, FF.FAR_SM, recipe),
           (16, G, block, FF.FAR_SM, recipe), (64, G, block, FF.FAR_SM, recipe), (1, G, block, FF.FAR_SM, recipe), (24, G, block, FF.FAR_SM, recipe),
           (R, G, 128, FF.FAR_SM, recipe), (R, G, 64, FF.FAR_SM, recipe), (R, G, 512, FF.FAR_SM, recipe),
           (R, G, block, FF.FAR_SM, recipe_of(DC.sexpr("fb", (40,)))), (R, G, block, FF.FAR_SM, recipe_of(DC.sexpr("fb", (300,)), typed=1))]
    write_manifest(tmp_path / "bad.fzm", bad)
    counts = replay(tmp_path / "bad.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == len(bad) and counts["built"] == 0 and counts["at_hand"] == 0, counts
    assert not (tmp_path / "cache").exists() or not code_objects(str(tmp_path / "cache"))
    write_manifest(tmp_path / "good.fzm", [(R, G, block, FF.FAR_SM, recipe)])
    counts = replay(tmp_path / "good.fzm", {"FLOWZ_HIP_CACHE": str(tmp_path / "cache")})
    assert counts["failed"] == 0 and counts["built"] == 1, counts


# ---- the random graphs of the GPU file ------------------------------------------------------------------------------------------------------
def test_the_seed_range_holds_the_pinned_number_of_random_graphs():
    """with the oracle alone: every kept graph lowers, stays finite at the GPU test's length, reaches beyond 256 samples and is accepted"""
    import numpy as np
    from oracle import flowz_oracle as O
    kept = FF.random_graphs()
    assert len(kept) == FF.RANDOM_KEPT == 12 >= 8, [k[0] for k in kept]
    T = FF.RANDOM_SHAPE[1]
    for seed, g, n_in, n_out in kept:
        assert (T * n_in) % 4 == 0 and (T * n_out) % 4 == 0
        want = O.compile(g, 2).run(O.synth_input(seed, np.arange(2), T, n_wires=n_in))
        assert np.isfinite(want).all() and np.abs(want).max() < 1e6, seed
