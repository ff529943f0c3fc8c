"""The fuzz of the backward of a whole recording without a GPU (tests/recording_fuzz.py, test_recording_fuzz_gpu.py): the pins of the
block-start-states kernels and the table of their classes by input frame width; the shapes rule gives every graph what it promises;
tests/recording_ref.py equals the single call bit for bit on every graph at every triple, plain and under the loss; the GPU test's
inputs tell a chain that hands every block the caller's state gradient from the right one, in every stream; the states kernels of the
crafted graphs compile for gfx950 without scratch or VGPR spills; what the stream-major calls refuse (the 40-wire graph) and take
(block windows off the 4-row grid) is decided before a device is needed; and the recorded manifest holds exactly the kernels
recording_fuzz.resolve_kernels() resolves."""
import ctypes
import gzip
import re

import numpy as np
import pytest

import grad_fuzz_cells as GC
import recording_fuzz as RF
from grad_harness import same
from grad_host_harness import ADJOINT, ADJOINT_LOSS, ADJOINT_SM, STATES, FakeCall
from zignal_amd import _capi as C
from zignal_amd import flowz as F

KEYS = ("x", "state", "params", "consts")
N_CHUNKS = 8
_restated = {}


def restated(name, i, loss=False):
    """recording_ref.grad of triple i, computed once for the tests that need it and left unchanged"""
    if (name, i, loss) not in _restated:
        ns, T, B = RF.shapes(name)[i]
        _restated[name, i, loss] = RF.restated(name, RF.draw(name, ns, T, RF.BASE + i), B, loss)
    return _restated[name, i, loss]


# ---- pins and classes -----------------------------------------------------------------------------------------------------------------
def test_the_pins_hold():
    """tests/golden/recording_fuzz_pins.json is what the library resolves now: a planner change that moves a class shows as a diff"""
    pins = RF.load_pins()
    assert list(pins) == RF.NAMES
    for name in RF.NAMES:
        assert RF.resolved(name) == pins[name], name


def test_every_class_of_the_states_kernels_is_reached_in_both_layouts():
    """the table of recording_fuzz.CLASSES: every graph's pin is its row's, every row has a graph, and both layouts of it (the 40-wire
    graph is in the last row time-major only)"""
    pins = RF.load_pins()
    reached = {}
    for name, pin in pins.items():
        n_in = pin["sizes"][0]
        row = next(i for i, (lo, hi, _, _) in enumerate(RF.CLASSES) if lo <= n_in and (hi is None or n_in <= hi))
        _, _, tm, sm = RF.CLASSES[row]
        assert pin["time_major"] == f"fz_states_kernel_{tm}b256", name
        assert pin["stream_major"] == (None if name in RF.TIME_MAJOR_ONLY else f"fz_states_sm_kernel_{sm}b256"), name
        if pin["sizes"][2]:                                       # (a graph without state launches no states kernel)
            reached.setdefault(row, set()).update({False} | ({True} if pin["stream_major"] else set()))
    assert reached == {i: {False, True} for i in range(len(RF.CLASSES))}, reached
    assert sum(1 for c in GC.CELLS if pins[c]["sizes"][0] == 3) >= 19
    for name, (n_in, n_out) in RF.WIDE.items():
        p = RF.prog(name)
        assert (p.n_in, p.n_out, p.n_state) == (n_in, n_out, n_in + 1) and p.grad_supported(), name


def test_the_shapes_rule_gives_every_graph_what_it_promises():
    for name in RF.NAMES:
        s, sh = RF.strides(name), RF.shapes(name)
        Ts, what = [t for _, t, _ in sh], (name, s, sh)
        assert len(sh) <= 8 and len(set(sh)) == len(sh), what
        assert {ns for ns, _, _ in sh} == {1, 64, 65, 321}, what
        assert all(B % 4 == 0 and B > 0 for _, _, B in sh), what
        assert 1 in Ts, what
        for u in (s["u_tm"], s["u_sm"]):
            assert u + 1 in Ts and (u <= 2 or any(1 < t < u for t in Ts)), what
        assert s["r"] in Ts and s["r"] + 1 in Ts and 2 * s["r_adj"] + 3 in Ts, what
        assert any(B == 4 and T >= 9 for _, T, B in sh), what
        assert s["c"] <= 4 or any(B % s["c"] and T > B for _, T, B in sh), what
        assert any(B >= T for _, T, B in sh) and any(T > B and T % B for _, T, B in sh), what
        assert max(Ts) <= 2 * 32 + 3 and RF.chain_triple(name)[1][1] >= 9, what
    for name, (ns, T, B, row0) in RF.SM_ONLY.items():
        p = RF.prog(name)
        ok = lambda b, r: b % 4 and not any((v * w) % 4 for v in (b, r) for w in (p.n_in, p.n_out))   # noqa: E731
        assert ok(B, row0) and not any(ok(b, row0) for b in range(5, B)) and not any(ok(B, r) for r in range(row0 + 1, 4)), name
        assert T > 2 * B and T % B, name


# ---- the restatement is sound on every graph --------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_the_restatement_is_the_single_call_bitwise_at_every_triple(part):
    """recording_ref.grad against the one adjoint_ref.grad / loss_grad_ref.loss_grad over all rows: what the GPU test compares the
    kernels with is sound at every shape it uses, the stream-major-only triples with their odd block lengths included"""
    for name in RF.NAMES[part::N_CHUNKS]:
        p = RF.prog(name)
        for i, (ns, T, B) in enumerate(RF.shapes(name)):
            d = RF.draw(name, ns, T, RF.BASE + i)
            for loss in (False, True):
                got, one = restated(name, i, loss), RF.single(name, d, loss)
                for k in KEYS + (("loss", "out") if loss else ()):
                    assert same(got[k], one[k]), (name, (ns, T, B), k, loss)
                assert got["starts"].shape == (-(-T // min(B, T)), p.n_state, ns)
        if name in RF.SM_ONLY:
            ns, T, B, _ = RF.SM_ONLY[name]
            d = RF.draw(name, ns, T, RF.BASE + len(RF.shapes(name)))
            for loss in (False, True):
                got, one = RF.restated(name, d, B, loss), RF.single(name, d, loss)
                assert all(same(got[k], one[k]) for k in KEYS + (("loss", "out") if loss else ())), (name, B, loss)


# ---- the inputs can tell a wrong chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(N_CHUNKS))
def test_the_gpu_tests_inputs_tell_a_chain_that_hands_on_the_callers_state_gradient(part, capsys):
    """at every graph's triple with blocks of 4 rows and the largest T: a backward whose every block gets the caller's state_grad
    instead of the gradient the block behind it wrote differs from the right one in at least one of x, state, params, consts in EVERY
    stream without specials -- so a driver that chains wrongly cannot pass test_recording_fuzz_gpu.py on any graph with a delay line.
    (Block starts that are one block stale are not asked to show in a gradient: cmp60, grad16 and passes_input_and_delayed_input are
    linear in their state; the GPU test compares the starts themselves.)"""
    lines = []
    for name in RF.NAMES[part::N_CHUNKS]:
        p = RF.prog(name)
        if not p.n_state:
            continue
        i, (ns, T, B) = RF.chain_triple(name)
        d = RF.draw(name, ns, T, RF.BASE + i)
        assert all(np.all(a != 0) for a in d[4:] if a.size), name    # dL/d(state after) and the three accumulators
        right, wrong = restated(name, i), RF.wrong_chain(name, d, B)
        clean = RF.clean_streams(name, ns)
        differs = {}
        for k in KEYS:
            g, w = right[k], wrong[k]
            ne = ~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))
            differs[k] = ne.any(axis=(0, 2)) if k == "x" else ne.any(axis=0)
        told = np.any([v for v in differs.values()], axis=0)
        lines.append(f"  {name:40} ns={ns:3} T={T:2}: streams told apart " + ", ".join(f"{k} {int((v & clean).sum())}" for k, v in differs.items())
                     + f" of {int(clean.sum())}")
        assert np.all(told[clean]), (name, int((~told & clean).sum()))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- the states kernels of the crafted graphs for gfx950 --------------------------------------------------------------------------
@pytest.mark.parametrize("name", RF.CRAFTED)
def test_states_kernels_jit_compile_without_scratch_or_vgpr_spills(name, capsys):
    """test_recording_grad_host.py's test of the same name on the graphs it does not reach; the register bound is the loss fuzz's:
    `vgprs` counts the unified file, accumulation registers included"""
    p = RF.prog(name)
    lines = []
    for sm in RF.layouts(name):
        r, sym = p.states_resources(sm), p.states_kernel_symbol(sm)
        m = re.fullmatch(r"fz_states_sm_kernel_u(\d+)r(\d+)b256_g[0-9a-f]{8}" if sm else r"fz_states_kernel_u(\d+)b256_g[0-9a-f]{8}", sym)
        assert m, sym
        U, R = int(m.group(1)), int(m.group(2)) if sm else 0
        assert sym.endswith(p.grad_kernel_symbol()[-10:]) and r["unroll"] == U and U in (1, 2, 4, 8) and U * p.n_in <= max(16, p.n_in)
        if sm:
            assert R % 4 == 0 and R % U == 0 and R * p.n_in >= 32
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
        # the stated LDS: four waves' patches of x alone; nothing where no state depends on an input wire (the fetch feeds dead code)
        reads = RF.wires_the_state_reads(p)
        assert r["lds_bytes"] == (4 * 64 * (R * p.n_in + 4) * 4 if sm and reads else 0) <= 160 * 1024, r
        if name in RF.WIDE:       # the whole frame is live: the group of U n_in frame registers (time-major: and the next group's) and the state
            assert reads == set(range(p.n_in)) and r["vgprs"] >= (1 if sm else 2) * U * p.n_in + p.n_state, (r, U)
        assert r["agprs"] <= r["vgprs"] <= 512 and r["vgprs"] - r["agprs"] <= 256, r
        src = p.states_source(sm)
        assert sym in src and "fz_adj::fwd" in src and f"#define FZ_U {U} " in src
        lines.append(f"{name} {sym}: {r['vgprs']} VGPRs, {r['sgpr_spills']} SGPR spills, {r['lds_bytes']} B LDS")
    with capsys.disabled():                                       # (SGPR spills are reported, not asserted: correct, slower)
        print("\n" + "\n".join(lines))


# ---- what the stream-major calls refuse and take ----------------------------------------------------------------------------------------
def test_the_40_wire_graph_is_refused_in_stream_major_before_a_device_is_needed():
    p = RF.prog("wide40x1")
    assert re.fullmatch(r"fz_states_kernel_u1b256_g[0-9a-f]{8}", p.states_kernel_symbol(False))
    assert p.states_resources(False)["scratch_bytes"] == 0
    for call in (p.states_kernel_symbol, p.states_resources, p.states_source):
        with pytest.raises(F.FlowzError) as ei:
            call(True)
        assert ei.value.code == C.FZ_E_UNSUPPORTED and "LDS" in str(ei.value)
    for loss in (False, True):
        b = FakeCall(p, 65, 11, loss=loss, recording=4)
        fn = b.fn
        a = b.args()
        assert fn(p._h, ctypes.byref(a), 1, 65, 24, 8, 11, 4, None, None) == C.FZ_E_UNSUPPORTED and "LDS" in C.last_error()
        if C.lib.fz_device_count() == 0:                          # the time-major call passes every check and stops at the device
            assert b.run(a) == C.FZ_E_NO_DEVICE, C.last_error()


@pytest.mark.parametrize("loss", [False, True], ids=["grad", "loss_grad"])
@pytest.mark.parametrize("name", sorted(RF.SM_ONLY))
def test_block_windows_off_the_4_row_grid_are_taken(name, loss):
    """the stream-major-only triples of the GPU test: the recording call (which checks every block launch as a direct call) and the
    one-launch call over the same window pass every check; time-major the block length is refused"""
    p = RF.prog(name)
    ns, T, B, row0 = RF.SM_ONLY[name]
    rows = RF.up4(row0 + T + 9) + 4
    b = FakeCall(p, ns, T, loss=loss, window=(rows, 0), recording=B)
    if C.lib.fz_device_count() == 0:
        assert b.run(b.args(), row0=row0) == C.FZ_E_NO_DEVICE, C.last_error()
        a = b.args(workspace_bytes=p.grad_workspace_bytes(ns, T))
        one = C.lib.fz_run_block_loss_grad_stream_major if loss else C.lib.fz_run_block_grad_stream_major
        assert one(p._h, ctypes.byref(a), ns, rows, row0, T, None) == C.FZ_E_NO_DEVICE, C.last_error()
    if (row0 + 1) * min(p.n_in, p.n_out) % 4:                     # (four wires: every row is on the float4 grid)
        assert b.run(b.args(), row0=row0 + 1) == C.FZ_E_INVALID and "row0" in C.last_error()
    with pytest.raises(F.FlowzError, match="multiple of 4"):
        p.recording_workspace_bytes(ns, T, B)


# ---- the manifest -------------------------------------------------------------------------------------------------------------------
def test_the_recorded_manifest_holds_the_kernels_of_the_gpu_test(tmp_path):
    """tests/golden/recording_fuzz_kernels.fzm.gz: the states kernels of every graph with state in both layouts, the wide graphs' adjoint
    and loss kernels, one forward kernel per graph with state; none refused, and record for record what resolve_kernels() writes now"""
    have = RF.records(gzip.open(RF.MANIFEST, "rb").read())
    flags = [r[3] for r in have]
    with_state = [n for n in RF.NAMES if RF.prog(n).n_state]
    states = [f for f in flags if f & ADJOINT and f & STATES]
    assert len(states) == sum(len(RF.layouts(n)) for n in with_state)
    assert sum(1 for f in states if f & ADJOINT_SM) == len(with_state) - len(RF.TIME_MAJOR_ONLY)
    n_wide = sum(len(RF.layouts(n)) for n in RF.WIDE)
    assert sum(1 for f in flags if f & ADJOINT and f & ADJOINT_LOSS) == n_wide
    assert sum(1 for f in flags if f & ADJOINT and not f & (STATES | ADJOINT_LOSS)) == n_wide
    assert sum(1 for f in flags if not f & ADJOINT) >= len(with_state)      # (forward kernels: one per graph, a few graphs' in two parts)
    r = F.manifest_build(RF.MANIFEST)
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] == len(have), r
    assert RF.records(RF.record(str(tmp_path / "now.fzm"))) == have
