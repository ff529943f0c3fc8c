"""The random-graph body matrix (tests/fuzz_bodies.py) without a GPU: the walk over the seed ranges reproduces the committed pins byte for
byte (tests/golden/fuzz_bodies_pins.json; `PYTHONPATH=. python tests/fuzz_bodies.py` rewrites them), every cell resolves to the kernel
pinned for it and the block behind its cut to another, the planner refuses what UNREACHABLE says it refuses, the matrix meets the
conditions it is there for, every cell's lowering agrees with the oracle on the IR interpreter, the inputs can tell a wrong kernel from a
right one, and the committed kernel manifest holds what the GPU test launches."""
import gzip
import re

import numpy as np
import pytest

import fuzz_bodies as FB
from ir_interp import run_ir
from zignal_amd import flowz as F

CELLS = FB.CELLS
_walked = {}


def walk():
    """FB.select(), once"""
    if not _walked:
        _walked["pins"], _walked["walk"] = FB.select()
    return _walked["pins"], _walked["walk"]


def cells(pred):
    return [cid for cid, p in CELLS.items() if pred(p)]


def G(pin):
    return FB.graph(pin["family"], pin["seed"])


# ---- the pins -----------------------------------------------------------------------------------------------------------------------
def test_a_selection_from_scratch_reproduces_the_committed_pins():
    with open(FB.PINS_FILE) as f:
        assert FB.dump(walk()[0]) == f.read()


def test_seed_ranges_are_apart_from_one_another_and_from_the_one_body_fuzz():
    """test_fuzz_graphs.py draws seeds 0 .. 7059, test_delay_lines_*.py 9000 .. 9239"""
    firsts = sorted(first for _, first in FB.FAMILIES.values())
    assert firsts[0] >= 10000 and all(b - a >= FB.WALK for a, b in zip(firsts, firsts[1:]))
    for pin in CELLS.values():
        first = FB.FAMILIES[pin["family"]][1]
        assert first <= pin["seed"] < first + FB.WALK


@pytest.mark.parametrize("part", range(8))
def test_cells_resolve_to_their_pinned_kernels(part):
    """the kernel of the launch, the layout, variant and shape of the cell's body, and another kernel behind the cut"""
    for cid, pin in list(CELLS.items())[part::8]:
        g = G(pin)
        layout, v, ns, T, tile, _ = FB.ALL_BODIES[pin["body"]]
        assert (pin["layout"], pin["variant"], pin["shape"], pin["tile"]) == (layout, None if v is None else list(v), [ns, T], tile), cid
        assert FB.resolve(pin["family"], pin["seed"], pin["body"]) == pin, cid
        cut, after = pin["cut"], tuple(pin["after"])
        assert cut % 2 == 1 and 0 < cut < T
        # the rows up to the cut run the cell's body, the rows behind it another one
        assert g["prog"].kernel_name(FB.variant(v, layout), ns, cut, tile) == pin["kernel"] or v is None, cid
        assert g["prog"].kernel_name(FB.variant(after, layout), ns, T - cut, tile) != pin["kernel"], cid
        if layout != "sm":
            assert after == FB.plain_of(g, ns, T, FB.out_f64(pin), other_than=pin["kernel"]) and (after == FB.PLAIN or pin["family"] == "deep" or FB.out_f64(pin)), cid


def test_a_cell_moved_to_the_plain_kernel_is_noticed():
    """the pins hold every cell to its body: the plain kernel's name is no cell's (but where the library chooses it by itself)"""
    for cid, pin in CELLS.items():
        if pin["variant"] is None:
            continue
        g = G(pin)
        ns, T = pin["shape"]
        assert g["prog"].kernel_name(FB.variant(FB.plain_of(g, ns, T, FB.out_f64(pin))), ns, T, 0) != pin["kernel"], cid


# ---- what the planner refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(FB.UNREACHABLE)), ids=lambda k: f"{'-'.join(FB.UNREACHABLE[k][0])}-{FB.UNREACHABLE[k][1]}-{FB.UNREACHABLE[k][2][0]}".replace(" ", "_"))
def test_the_planner_refuses_what_unreachable_names(k):
    """every entry on the first two seeds of its class in each family's range, on each of its bodies -- and no cell is of such a class"""
    families, cls, bodies, status, msg = FB.UNREACHABLE[k]
    for family in families:
        first = FB.FAMILIES[family][1]
        for body in bodies:
            n = 0
            for seed in range(first, first + FB.WALK):
                g = FB.graph(family, seed)
                if g is None or FB.unreachable(family, g, body) is not FB.UNREACHABLE[k]:
                    continue
                r = FB.refusal(g, body)
                assert r is not None and r[0] == status and msg in r[1], (family, seed, body, r)
                n += 1
                if n == 2:
                    break
            assert n, (family, cls, body)
    for cid, pin in CELLS.items():
        assert FB.unreachable(pin["family"], G(pin), pin["body"]) is None, cid


def test_at_most_half_of_the_seeds_walked_are_refused():
    """per (family, body), over the seeds no entry of UNREACHABLE holds; and every body keeps its K seeds of every family that reaches it"""
    for (family, body), (kept, refused, walked) in walk()[1].items():
        assert 2 * len(refused) <= walked, (family, body, refused)
        first = FB.FAMILIES[family][1]
        reachable = any(g is not None and FB.unreachable(family, g, body) is None and FB.wanted(g, body) for g in (FB.graph(family, s) for s in range(first, first + 120)))
        K = FB.K_MORE.get((family, body), FB.ALL_BODIES[body][5])
        assert len(kept) == (K if reachable else 0) or body in FB.OUT64_BODIES, (family, body, kept)


def test_every_body_has_cells_of_every_family_that_reaches_it():
    none = {(f, b) for f in FB.TABLE_FAMILIES for b in FB.BODIES if not cells(lambda p: p["family"] == f and p["body"] == b)}
    assert none == {("deep", b) for b in ("ragged-p2", "ragged-p4", "sm-short-1x1") + FB.LONG_BODIES}
    for b in FB.OUT64_BODIES:
        assert cells(lambda p: p["body"] == b)
    # fz_compile_typed: a lane-pair cell free-running and one in lockstep (a double input wire: a 2-wire frame), and a graph with float and
    # double inputs on both bodies
    lock = lambda p: int(re.search(r"f(\d+)[RMLS]*$", p["kernel"]).group(1)) & FB.L                      # noqa: E731
    for b in FB.TIN_BODIES:
        mine = [p for p in CELLS.values() if p["body"] == b]
        assert mine and all(p["family"] == "tin" and "f64" in p["in_dtypes"] and bool(lock(p)) == b.endswith("lock") for p in mine), b
        if FB.WANTS[b] == "pairs":
            assert all(p["kernel"].endswith("L") and p["frame"][0] == 2 for p in mine), b
        else:
            assert all({"f32", "f64"} <= set(p["in_dtypes"]) for p in mine), b


def test_the_input_types_of_a_typed_compile_say_nothing_about_the_graph():
    """the types come from a stream of their own: among the one-input graphs of the range both float and double occur, among the two-input
    ones all four pairs"""
    import randgraphs as R
    first = FB.FAMILIES["tin"][1]
    seen = {1: set(), 2: set()}
    for seed in range(first, first + 120):
        n_in = R.make_typed(seed)[1]
        if n_in in seen:
            rng = np.random.default_rng(seed + 88000)
            seen[n_in].add(tuple(str(rng.choice(["f32", "f64"])) for _ in range(n_in)))
    assert len(seen[1]) == 2 and len(seen[2]) == 4, seen
    assert FB.in_dtypes("tin", first, 1) in (None, ["f64"])


def test_a_stream_major_short_cell_hands_its_state_to_the_long_body():
    """the 1 in / 1 out short cells: the block behind the cut runs the long-run body; the other short cells continue on short with
    another chunk, the long and pair cells on short"""
    one = [p for p in CELLS.values() if p["body"] == "sm-short-1x1"]
    assert len(one) == 3
    for p in one:
        g, (ns, T) = G(p), p["shape"]
        assert p["after"][3] & FB.SML and g["prog"].kernel_name(FB.variant(tuple(p["after"]), "sm"), ns, T - p["cut"], 0).endswith("b64f%d" % (FB.SML | FB.SM))
    for p in CELLS.values():
        if p["body"] in FB.LONG_BODIES:
            assert p["after"][3] & FB.SMS and not p["after"][3] & FB.SML, p


# ---- the conditions the matrix is there for -------------------------------------------------------------------------------------------
def test_frame_widths_lane_groups_types_rings_and_comparisons():
    lock = lambda p: int(re.search(r"f(\d+)[RMLS]*$", p["kernel"]).group(1)) & FB.L                      # noqa: E731
    for body in FB.BODIES:
        if body in FB.LONG_BODIES or FB.WANTS.get(body) == "1x1":
            assert {tuple(p["frame"]) for p in CELLS.values() if p["body"] == body} == {(1, 1)}
        else:
            assert len({tuple(p["frame"]) for p in CELLS.values() if p["body"] == body}) >= 3, body
    # lane groups: pairs with four streams per lane, singles with two -- free-running and in lockstep
    for bodies, letter in ((FB.P4_BODIES, "L"), (FB.P2_BODIES, "S")):
        for locked in (False, True):
            assert cells(lambda p: p["body"] in bodies and p["kernel"].endswith(letter) and bool(lock(p)) == locked), (letter, locked)
    # ragged stream counts, lockstep bodies four workgroups at least (but the 1024-lane geometry), stream tiles
    assert all(p["kernel"].endswith("RM") for p in CELLS.values() if p["body"].startswith("ragged"))
    for p in CELLS.values():
        m = re.match(r"fz_block_kernel_p(\d+)u(\d+)b(\d+)", p["kernel"])
        P, B = int(m.group(1)), int(m.group(3))
        if p["variant"] and p["variant"][3] & FB.L:
            assert lock(p) and (B == 1024 or -(-p["shape"][0] // (P * B)) >= 4), p
        assert p["shape"][0] <= 4096 and p["shape"][0] * p["shape"][1] <= 4096 * 300
    for kind in ("double", "complex", "cdouble"):
        assert cells(lambda p: p["family"] == "typed" and p["kind"] == kind), kind
    for ring in ("lds", "far"):
        assert cells(lambda p: p["family"] == "deep" and ring in G(p)["rings"]), ring
    for op in FB.COMPARISONS:
        assert cells(lambda p: p["family"] == "cmp" and op in G(p)["nodes"]), op
    # what the random graphs have and the hand-written ones do not
    assert cells(lambda p: p["frame"][0] != p["frame"][1] and max(p["frame"]) in (3, 5, 7))
    assert cells(lambda p: "neg" in G(p)["nodes"] and "fb" in G(p)["nodes"]) and cells(lambda p: "div" in G(p)["nodes"] and "fb" in G(p)["nodes"])
    assert cells(lambda p: p["family"] == "cmp" and FB.compares_in_double(G(p)["g"]))                   # a comparison made in double
    assert cells(lambda p: p["family"] == "deep" and {"lds", "far"} <= G(p)["rings"] and min(FB.delays(G(p)["g"])) <= FB.REG_MAX)
    # float64 output frames: every typed graph of the rows cells with a double result, free-running and in lockstep
    want = {p["seed"] for p in CELLS.values() if p["family"] == "typed" and p["shape"] == [2048, 300] and FB.has_double_result(G(p))}
    for body in FB.OUT64_BODIES:
        assert {p["seed"] for p in CELLS.values() if p["body"] == body} == want and want, body


# ---- the lowering and the inputs --------------------------------------------------------------------------------------------------------
def _graph_cases():
    """one cell per (family, seed, shape)"""
    seen = {}
    for cid, p in CELLS.items():
        seen.setdefault((p["family"], p["seed"], tuple(p["shape"]), p["cut"]), cid)
    return list(seen.items())


@pytest.mark.parametrize("part", range(8))
def test_lowering_matches_the_oracle_on_the_first_and_last_streams(part):
    """tests/ir_interp.py on the cell's own input, the first and the last 3 streams and all rows, bit for bit (a NaN equal to a NaN); a
    program compiled with input types against oracle.run_typed"""
    for (family, seed, (ns, T), cut), cid in _graph_cases()[part::8]:
        g = FB.graph(family, seed)
        x, wires = FB.frames(family, seed, FB.slice_streams(ns), T)
        want, _ = FB.oracle_run(family, seed, x, wires)
        got, _ = run_ir(g["prog"], x)
        assert FB.ndiff(got, want) == 0, cid
        assert FB.all_finite(g, want), cid


@pytest.mark.parametrize("part", range(8))
def test_the_inputs_tell_a_wrong_kernel_from_a_right_one(part):
    """on the oracle alone: no output wire constant, every input wire reaches the output, the cut moved by one row leaves another state"""
    for (family, seed, (ns, T), cut), cid in _graph_cases()[part::8]:
        assert FB.discriminates(family, seed, ns, T, cut) is None, cid


def test_a_seed_whose_inputs_tell_nothing_is_passed_over():
    """the walk replaces such a seed by the next one: among the first 40 seeds of the plain, cmp and deep ranges there are such seeds (the
    typed range has none there), and none of any family is a cell"""
    for family in FB.TABLE_FAMILIES:
        first = FB.FAMILIES[family][1]
        blind = [s for s in range(first, first + 40) if FB.graph(family, s) is not None and FB.discriminates(family, s, 334, 300, FB.CUT_SM) is not None]
        assert blind or family == "typed", family
        assert not {p["seed"] for p in CELLS.values() if p["family"] == family} & set(blind)


# ---- the manifest -----------------------------------------------------------------------------------------------------------------------
def test_the_recorded_manifest_holds_the_kernels_of_the_gpu_test(tmp_path):
    """tests/golden/fuzz_bodies_kernels.fzm.gz: none refused, and record for record what resolve_kernels() writes now"""
    have = FB.records(gzip.open(FB.MANIFEST, "rb").read())
    r = F.manifest_build(FB.MANIFEST)
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] == len(have), r
    assert FB.records(FB.record(str(tmp_path / "now.fzm"))) == have


def test_a_damaged_manifest_is_reported(tmp_path):
    """a manifest is data from elsewhere: records with three streams per lane, a workgroup that is no multiple of a wave, a chunk of a thousand
    rows or both stream-major bodies at once are counted as failed, not built"""
    import os
    import subprocess
    import sys
    text = gzip.open(FB.MANIFEST, "rb").read()
    m = re.compile(rb"FZM1 (\d+) (\d+) (\d+) (\d+) (\d+)\n").match(text)
    P, U, B, flags, n = (int(x) for x in m.groups())
    recipe = text[m.end():m.end() + n]
    rec = lambda P_, U_, B_, f_: b"FZM1 %d %d %d %d %d\n" % (P_, U_, B_, f_, n) + recipe   # noqa: E731
    bad = [rec(3, U, B, flags), rec(P, U, 100, flags), rec(P, 1000, B, flags), rec(1, 64, 0, FB.SM | FB.SML | FB.SMS)]
    path = tmp_path / "bad.fzm"
    path.write_bytes(b"".join(bad) + rec(P, U, B, flags))
    code = "import sys\nsys.path.insert(0, %r)\nfrom zignal_amd import flowz as F\nprint(F.manifest_build(%r, 2))" % (os.path.dirname(FB.HERE), str(path))
    env = {k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(env, FLOWZ_HIP_CACHE=str(tmp_path / "cache")), text=True)
    r = eval(out.splitlines()[-1])
    assert r["records"] == len(bad) + 1 and r["failed"] == len(bad) and r["built"] + r["at_hand"] == 1, r
