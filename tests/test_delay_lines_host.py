"""The delay-line matrix (tests/delay_cells.py) without a GPU: every cell resolves to the kernel and the ring plan pinned for it
(tests/golden/delay_line_pins.json; `python tests/delay_cells.py` rewrites it), the programs' line layout follows from the depths, the
matrix covers every ring plan and storage boundary, the planner refuses what it must, the inputs tell a tap that is off by one, and
the lowering of deep lines agrees with the oracle on the IR interpreter -- also on random graphs with deep delays (randgraphs.make_deep)."""
import numpy as np
import pytest

import delay_cells as D
import randgraphs as R
from ir_interp import run_ir
from oracle import flowz_oracle as O
from test_graph_functions_gpu import ndiff
from zignal_amd import flowz as F

PINS = D.load_pins()
BY_ID = {c["id"]: c for c in D.CELLS}
TIME_MAJOR_BODIES = ("free", "lockstep", "stepdown", "tiles", "tilesL")


def body_of(c):
    """the kernel body a cell is there for"""
    name = PINS[c["id"]][0]
    lock = name.split("f")[-1].rstrip("RMLS").isdigit() and int(name.split("f")[-1].rstrip("RMLS")) & D.L
    if c["layout"] == "sm":
        return "sm"
    if c["layout"] == "tiles":
        return "tilesL" if lock else "tiles"
    return ("stepdown" if PINS[c["id"]][2] == 1 else "lockstep") if lock else "free"


def test_every_cell_is_pinned_and_no_pin_is_left_over():
    assert set(PINS) == set(BY_ID)


def all_kernels():
    """(cell id, which, kernel name, code id) of everything the GPU test of the matrix launches: each cell's own kernel, the other body of
    its chained run, the plain kernel its state is compared with"""
    out = []
    for c in D.CELLS:
        prog = D.compile_cell(c)
        for which, v, layout in (("own", D.variant(c), c["layout"]), ("other", F.make_variant(*D.other_body(c)), "rows"), ("plain", F.make_variant(*D.plain(c)), "rows")):
            tile = c["tile"] if layout == "tiles" else 0
            out.append((c["id"], which, prog.kernel_name(v, c["ns"], c["T"], tile), prog.kernel_code_id(v, c["ns"], c["T"], tile)))
    return out


def test_the_matrix_stays_within_its_kernel_budget():
    """distinct code objects of the whole matrix (graphs that differ in literals only share one): own, other and plain bodies counted"""
    n = len({k[3] for k in all_kernels()})
    assert 300 <= n <= 600, n


def test_the_manifest_of_the_matrix_builds_every_kernel_the_cells_resolve(tmp_path):
    """tests/golden/delay_line_kernels.fzm.gz (recorded while test_delay_lines_gpu.py ran) replayed into an empty cache:
    nothing fails, and every kernel of every cell -- own, other, plain -- is then at hand: resolving them all builds nothing more"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, os, json\nsys.path.insert(0, %r)\nfrom zignal_amd import flowz as F\n"
            "r = [F.manifest_build(os.path.join(%r, 'golden', 'delay_line_kernels.fzm.gz'))]\n"
            "before = sorted(os.listdir(os.environ['FLOWZ_HIP_CACHE']))\n"
            "import test_delay_lines_host as H\nids = sorted({k[3] for k in H.all_kernels()})\n"
            "print(json.dumps([r, before, sorted(os.listdir(os.environ['FLOWZ_HIP_CACHE'])), ids]))\n") % (here, here)
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_CACHE=str(tmp_path)), cwd=os.path.dirname(here), text=True)
    import json
    r, before, after, ids = json.loads(out.splitlines()[-1])
    assert r[0]["failed"] == 0 and r[0]["records"] >= 300, r
    have = {f[:-6] for f in before if f.endswith(".hsaco")}
    missing = [i for i in ids if i not in have]
    assert not missing, (len(missing), missing[:5])
    assert [f for f in after if f.endswith(".hsaco")] == [f for f in before if f.endswith(".hsaco")]


@pytest.mark.parametrize("part", range(8))
def test_cells_resolve_to_their_pinned_kernels_and_ring_plans(part):
    """the kernel name of the launch; FZ_P, FZ_U, FZ_BLOCK, FZ_RING_G, FZ_LDS_SLOTS of the generated configuration and how the generated
    body reads its rings -- and the block after each cut of the chained run is another kernel"""
    for c in D.CELLS[part::8]:
        prog = D.compile_cell(c)
        got = list(D.resolved(prog, c))
        assert got == PINS[c["id"]], (c["id"], got, PINS[c["id"]])
        o = D.other_body(c)
        assert prog.kernel_name(F.make_variant(*o), c["ns"], c["T"], 0) != got[0] or c["layout"] != "rows", c["id"]
        name, P, U, B, G, slots, how = got
        T = c["T"]
        assert c["tail"] or ((U == 1 or T % U) and (not G or T % G)), c["id"]       # (but the blocks as long as the line)
        assert c["ns"] % P == 0 and sum(D.pieces(c, G, U)) == T + c["tail"]


def test_line_layout_follows_from_the_depths():
    """max_delay, n_lds_slots, n_state, line_dtypes from the rules of fz_lower.cpp: a ring in LDS of the next power of two from depth 9 on, in
    HBM (the line's state rows and one phase row) beyond 256; a double slot takes two float rows"""
    seen = set()
    for c in D.CELLS:
        key = (c["tmpl"], c["args"], c["dtype"])
        depths = D.graph_depths(c["tmpl"], c["args"])
        if key in seen:
            continue
        seen.add(key)
        prog = D.compile_cell(c)
        rd = D.reads(c["tmpl"], c["args"])
        assert prog.max_delay == max(r for _, r in rd), key
        assert sorted(d for _, d in prog.lines()) == sorted(depths * (2 if c["dtype"] == "cf32" else 1)), key
        w = 2 if c["dtype"] == "f64" else 1
        lines = depths * (2 if c["dtype"] == "cf32" else 1)
        assert prog.n_lds_slots == sum(w * D.ring_size(d) for d in lines if D.storage(d) == "lds"), key
        assert prog.n_state == sum(w * d for d in lines) + sum(D.storage(d) == "far" for d in lines), key
        want_dt = {"f64": ["f64"], "cf32": ["re", "im"], None: ["f32"] * len(lines)}[c["dtype"]]
        assert prog.line_dtypes() == want_dt, key
        assert {D.storage(d) for d in lines} == {D.storage(dl) for dl, _ in rd}


def _cells(pred):
    return [c["id"] for c in D.CELLS if pred(c, *PINS[c["id"]])]


def test_the_matrix_covers_every_ring_plan_and_storage_boundary():
    """every condition names the cells that meet it: remove the only cell of one and this fails"""
    lds1 = lambda c: c["tmpl"] in ("ff", "fb") and D.storage(c["d"]) == "lds" and not c["dtype"]     # noqa: E731  (one float LDS line, one read)
    # every G
    for g in (0, 2, 4, 8, 16, 32):
        assert _cells(lambda c, n, P, U, B, G, s, how: s > 0 and G == g), g
    # every residue of d mod (4 / P) on a vectorised cell
    for p in (1, 2, 4):
        for r in range(4 // p):
            assert _cells(lambda c, n, P, U, B, G, s, how: lds1(c) and how == "vec" and P == p and c["d"] % (4 // p) == r), (p, r)
    # each way of reading with ring size == depth and with ring size > depth
    for h in ("vec", "front", "place"):
        assert _cells(lambda c, n, P, U, B, G, s, how: lds1(c) and how == h and D.ring_size(c["d"]) == c["d"]), h
        assert _cells(lambda c, n, P, U, B, G, s, how: lds1(c) and how == h and D.ring_size(c["d"]) > c["d"]), h
    # G lowered because it does not divide the chunk
    def first_g(c, P, U):
        g = 1
        while g * 2 <= min(r for dl, r in D.reads(c["tmpl"], c["args"]) if D.storage(dl) == "lds") and g * 2 <= U:
            g *= 2
        return g

    # (first_g and est restate ring_plan() in zignal_amd/csrc/fz_codegen.cpp -- the two `while` loops over G and its lambda `regs` -- to say WHY a
    #  pinned G is what it is; an editor of that arithmetic changes these two with it)
    def est(c, P, g):                                            # ring_plan's register estimate at G = g
        tw = 4 // P
        rd = {(i, r) for i, (dl, r) in enumerate(D.reads(c["tmpl"], c["args"])) if D.storage(dl) == "lds"}
        if c["tmpl"] == "many":                                  # (i: the read's line)
            rd = {(i // c["args"][2], r) for i, r in rd}
        n_lines = len(D.graph_depths(c["tmpl"], c["args"]) or [1])
        return n_lines * g * P + sum(((tw - r % tw) % tw + g + tw - 1) // tw * 4 for _, r in rd)
    assert _cells(lambda c, n, P, U, B, G, s, how: lds1(c) and how == "vec" and U % first_g(c, P, U) and G < first_g(c, P, U))
    # ... because the register estimate passed 200; given up for that reason
    float_rows = lambda c: not c["dtype"] and c["layout"] != "sm" and c["tmpl"] == "many"              # noqa: E731
    assert _cells(lambda c, n, P, U, B, G, s, how: float_rows(c) and how == "vec" and U % first_g(c, P, U) == 0 and G < first_g(c, P, U) and est(c, P, first_g(c, P, U)) > 200 >= est(c, P, G))
    assert _cells(lambda c, n, P, U, B, G, s, how: float_rows(c) and how != "vec" and U >= 2 and first_g(c, P, U) >= max(4 // P, 2) and est(c, P, max(4 // P, 2)) > 200)
    # a workgroup shrunk to fit the LDS (block 0 asked for: 256 lanes, or what divides the tile)
    shrunk = _cells(lambda c, n, P, U, B, G, s, how: c["v"] and c["v"][2] == 0 and c["layout"] == "rows" and s and B < 256 and s * 256 * 4 * P > D.MAX_LDS_BYTES >= s * B * 4 * P)
    assert shrunk and "many4_128_2-p1u16" in shrunk
    # the LDS / HBM boundary on every time-major body
    for d in (255, 256, 257):
        for b in TIME_MAJOR_BODIES:
            if d == 257 and b == "stepdown":                     # (far lines take no third buffer: refused, below)
                continue
            assert _cells(lambda c, n, P, U, B, G, s, how: c["d"] == d and body_of(c) == b), (d, b)
    # every depth on a time-major body; 9..256 on the stream-major short body and as a double line
    for d in D.DEPTHS:
        assert _cells(lambda c, n, P, U, B, G, s, how: c["d"] == d and c["tmpl"] in ("ff", "fb") and body_of(c) in TIME_MAJOR_BODIES), d
    for d in D.LDS_DEPTHS:
        assert _cells(lambda c, n, P, U, B, G, s, how: c["d"] == d and body_of(c) == "sm"), d
        assert _cells(lambda c, n, P, U, B, G, s, how: c["d"] == d and c["dtype"] == "f64"), d
    # far lines: the youngest ring read 9 (chunks of 4 at most) and 32 or more (16); a shadow register
    far_min = lambda c: min([r for dl, r in D.reads(c["tmpl"], c["args"]) if dl > D.LDS_MAX and r > D.REG_MAX] or [0])   # noqa: E731
    assert _cells(lambda c, n, P, U, B, G, s, how: far_min(c) == 9 and U == 4)
    assert _cells(lambda c, n, P, U, B, G, s, how: far_min(c) >= 32 and U == 16)
    assert _cells(lambda c, n, P, U, B, G, s, how: any(dl > D.LDS_MAX and r <= D.REG_MAX for dl, r in D.reads(c["tmpl"], c["args"])))
    # every unroll and lane packing of the free-running kernel; lockstep workgroups of 256 and 1024 lanes; the library's own choice
    for u in (1, 2, 3, 4, 8, 12, 16, 32):
        assert _cells(lambda c, n, P, U, B, G, s, how: body_of(c) == "free" and U == u and s), u
    for p in (1, 2, 4):
        assert _cells(lambda c, n, P, U, B, G, s, how: body_of(c) == "free" and P == p and s), p
        assert _cells(lambda c, n, P, U, B, G, s, how: body_of(c) == "free" and P == p and D.storage(c["d"]) == "far"), p
    for b in (256, 1024):
        assert _cells(lambda c, n, P, U, B, G, s, how: body_of(c) == "lockstep" and B == b and s), b
        assert _cells(lambda c, n, P, U, B, G, s, how: body_of(c) == "lockstep" and B == b and D.storage(c["d"]) == "far"), b
    assert _cells(lambda c, n, P, U, B, G, s, how: c["v"] is None)
    assert _cells(lambda c, n, P, U, B, G, s, how: n.endswith("L") and P == 4 and s)                 # lane groups over an LDS ring
    # blocks shorter than, as long as and one longer than the line, in every storage class
    for st in ("lds", "far"):
        for k in (-3, 0, 1):
            assert _cells(lambda c, n, P, U, B, G, s, how: D.storage(c["d"]) == st and c["T"] == c["d"] + k), (st, k)
    # complex and double rings up to the deepest
    assert _cells(lambda c, n, P, U, B, G, s, how: c["dtype"] == "cf32" and c["d"] == 256) and _cells(lambda c, n, P, U, B, G, s, how: c["dtype"] == "f64" and c["d"] == 256)


@pytest.mark.parametrize("r", D.REFUSALS, ids=lambda r: f"{r[0]}{'_'.join(map(str, r[1]))}-{r[3]}")
def test_the_planner_refuses_what_does_not_fit(r):
    tmpl, args, dtype, v, sm, code, msg = r
    prog = D.compile_cell({"tmpl": tmpl, "args": args, "dtype": dtype})
    with pytest.raises(F.FlowzError) as e:
        prog.kernel_name(F.make_variant(v[0], v[1], v[2], v[3] | (D.SM if sm else 0)), 512, 1001, 0)
    assert e.value.code == code and msg in str(e.value), e.value


def test_one_line_fewer_than_the_refused_graph_fits():
    """many(5, 128, 2) runs (a cell, in 64-lane workgroups); many(6, 128, 2) is refused above"""
    assert PINS["many5_128_2-p1u1"][3] == 64 and PINS["many5_128_2-p1u1"][5] * 64 * 4 == D.MAX_LDS_BYTES


def test_a_far_line_on_a_double_wire_is_refused_at_compile_time():
    """the rings in HBM hold floats: depth 257 on a double wire is no program; on a std::complex<float> wire it is two float rings (cells)"""
    with pytest.raises(F.FlowzError) as e:
        F.compile(F.from_sexpr(D.fbk(257)), in_dtypes=["f64"])
    assert e.value.code == F.C.FZ_E_UNSUPPORTED and "a double delay line deeper than 256" in str(e.value), e.value
    F.compile(F.from_sexpr(D.fbk(256)), in_dtypes=["f64"])
    z = F.compile(F.from_sexpr(D.fbk(257)), in_dtypes=["cf32"])
    assert [d for _, d in z.lines()] == [257, 257] and z.line_dtypes() == ["re", "im"] and z.n_lds_slots == 0 and z.n_state == 2 * (257 + 1)
    assert [c["id"] for c in D.CELLS if c["dtype"] == "cf32" and c["d"] > D.LDS_MAX]


# ---- the inputs are not blind to an off-by-one ------------------------------------------------------------------------------------
def _graph_cases():
    seen, out = set(), []
    for c in D.CELLS:
        key = (c["tmpl"], c["args"], c["dtype"], c["ns"], c["T"] + c["tail"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("part", range(8))
def test_the_oracle_output_differs_in_every_stream_when_a_tap_moves_by_one(part):
    """for every graph and input of the matrix: the oracle's output with one read moved by one sample differs from the cell's in at least
    one sample of EVERY stream of the cell"""
    for c in _graph_cases()[part::8]:
        x, wires = D.frames(c)
        ids = np.arange(c["ns"])
        want = D.oracle_run(c, x=x, wires=wires, streams=ids)
        ok = ~np.isin(ids, D.edge_streams(c))
        assert D.all_finite(c, want[:, ok]), c["id"]
        for args in D.neighbours(c["tmpl"], c["args"]):
            if c["dtype"] == "f64" and max(args) > D.LDS_MAX:
                continue                                         # (no such program: refused at compile time)
            other = D.oracle_run(c, args=args, x=x, wires=wires, streams=ids)
            I = np.uint32
            differ = ((want.view(I) != other.view(I)) & ~(np.isnan(want) & np.isnan(other))).any(axis=(0, 2))
            assert differ.all(), (c["id"], args, ids[~differ][:8])


# ---- the lowering of deep lines -------------------------------------------------------------------------------------------------------
LOWERING = [("ff", (d,)) for d in (8, 9, 16, 256, 257, 513)] + [("fb", (d,)) for d in (8, 12, 64, 255, 258, 512)] + \
           [("taps", a) for a in ((16, 12, 9, 3), (256, 100, 9, 7), (257, 128, 9, 3), (513, 257, 32))] + \
           [("mixed", (3, 40, 300)), ("mixed", (8, 9)), ("mixed2", (5, 16, 257)), ("mixed2", (8, 256)), ("many", (4, 16, 3)), ("many", (3, 128, 2))]


@pytest.mark.parametrize("case", LOWERING, ids=lambda c: c[0] + "_".join(map(str, c[1])))
def test_lowering_of_deep_lines_matches_the_oracle(case):
    tmpl, args = case
    g = D.sexpr(tmpl, args)
    p = F.compile(F.from_sexpr(g))
    T = 2 * p.max_delay + 3
    x = O.synth_input(D.SEED + sum(args), np.arange(2), T, n_wires=p.n_in)
    want = O.compile(g, 2).run(x)
    got, st = run_ir(p, x)
    assert ndiff(got, want) == 0 and np.isfinite(want).all()
    # two chained blocks on the interpreter: its state rows carry every line
    ya, s = run_ir(p, x[:p.max_delay + 1])
    yb, s = run_ir(p, x[p.max_delay + 1:], state=s)
    assert ndiff(np.concatenate([ya, yb]), want) == 0 and ndiff(s, st) == 0


@pytest.mark.parametrize("dtype", ["f64", "cf32"])
def test_lowering_of_typed_deep_lines_matches_the_oracle(dtype):
    for d in (9, 64, 256):
        c = {"tmpl": "fb", "args": (d,), "dtype": dtype, "ns": 2, "T": 2 * d + 3, "tail": 0}
        x, wires = D.frames(c)
        got, _ = run_ir(D.compile_cell(c), x)
        assert ndiff(got, D.oracle_run(c, x=x, wires=wires)) == 0, d


# ---- random graphs with deep delays -----------------------------------------------------------------------------------------------
def usable_deep(seed):
    """a make_deep graph the oracle takes and that has a delay beyond the registers"""
    g, n_in, n_out = R.make_deep(seed)
    try:
        ok = O.input_arity(g) == n_in and O.output_arity(g) == n_out
        O.compile(g, 1)
    except O.GraphError:
        return None
    deep = any(isinstance(e, tuple) and e[0] == "del" and e[2] > D.REG_MAX for e in _walk(g))
    return (g, n_in, n_out) if ok and deep else None


def _walk(e):
    yield e
    for c in e:
        if isinstance(c, tuple):
            yield from _walk(c)


def test_make_deep_leaves_make_alone_and_reaches_every_storage_class():
    classes = set()
    for seed in range(9000, 9100):
        g0, g1 = R.make(seed), R.make_deep(seed)
        assert g1[1:] == g0[1:] and R.make(seed) == g0
        d0 = [e[2] for e in _walk(g0[0]) if e[0] == "del"]
        d1 = [e[2] for e in _walk(g1[0]) if e[0] == "del"]
        assert len(d0) == len(d1) and all(a == b or b in R.DEEP_DELAYS for a, b in zip(d0, d1))
        classes |= {D.storage(d) for d in d1}
    assert classes == {"reg", "lds", "far"}


@pytest.mark.parametrize("chunk", range(4))
def test_lowering_matches_oracle_on_random_graphs_with_deep_delays(chunk):
    n = 0
    for seed in range(9000 + chunk * 25, 9000 + chunk * 25 + 25):
        u = usable_deep(seed)
        if u is None:
            continue
        g, n_in, n_out = u
        p = F.compile(F.from_sexpr(g))
        assert (p.n_in, p.n_out) == (n_in, n_out)
        x = O.synth_input(seed, np.arange(2), 2 * p.max_delay + 3, n_wires=n_in)
        want = O.compile(g, 2).run(x)
        got, _ = run_ir(p, x)
        assert ndiff(got, want) == 0, f"seed {seed}: {g}"
        assert np.isfinite(want).all(), f"seed {seed} blew up"
        n += 1
    assert n >= 10


DEEP_GPU_CHUNKS, DEEP_GPU_MIN, DEEP_GPU_SHAPE = 2, 10, (136, 620)


def deep_gpu_seeds(chunk):
    return range(9200 + chunk * 20, 9200 + chunk * 20 + 20)


def deep_packings(prog, ns, T):
    """the streams per lane the planner takes for a deep random graph at the GPU test's shape (a ring of 256 slots does not fit the LDS with
    four streams per lane)"""
    out = []
    for P in (1, 2, 4):
        try:
            prog.kernel_name(F.make_variant(P, 0), ns, T)
            out.append(P)
        except F.FlowzError as e:
            assert e.code == F.C.FZ_E_UNSUPPORTED and "delay lines too long for the LDS ring buffers" in str(e), e
    return out


# seed -> the streams per lane the GPU test runs it with: decided and checked here, on the CPU; the GPU test reads this table and catches nothing
DEEP_PACKINGS = {seed: [1, 2, 4] for c in range(DEEP_GPU_CHUNKS) for seed in deep_gpu_seeds(c)}
# (no seed of these ranges holds a ring that four or two streams per lane cannot fit; one that did would be listed here: seed -> [1, 2])


@pytest.mark.parametrize("chunk", range(DEEP_GPU_CHUNKS))
def test_the_gpu_seed_ranges_hold_enough_usable_deep_graphs(chunk):
    """the oracle alone, at the GPU test's length: enough graphs per chunk that lower, stay finite and reach beyond the registers"""
    n = full = 0
    for seed in deep_gpu_seeds(chunk):
        u = usable_deep(seed)
        if u is None:
            continue
        g, n_in, _ = u
        ps = deep_packings(F.compile(F.from_sexpr(g)), *DEEP_GPU_SHAPE)
        assert ps == DEEP_PACKINGS[seed] and ps[0] == 1, (seed, ps)
        full += ps == [1, 2, 4]
        want = O.compile(g, 2).run(O.synth_input(seed, np.arange(2), DEEP_GPU_SHAPE[1], n_wires=n_in))
        assert np.isfinite(want).all() and np.abs(want).max() < 1e6, seed
        n += 1
    assert n >= DEEP_GPU_MIN and full >= DEEP_GPU_MIN - 2
