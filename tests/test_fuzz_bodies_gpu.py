"""Random graphs on every body of the forward block kernel (tests/fuzz_bodies.py; the cells are tests/golden/fuzz_bodies_pins.json): each
cell's whole output equals oracle.flowz_oracle's bit for bit (a NaN equal to a NaN) on all streams; the state after the block equals, word
for word, the state the plain kernel leaves on the same input; the block cut at the pinned odd row and continued on another body gives the
same output and the same final state; ragged cells and the 2-stream stream-major cells write nothing outside `out` and `state` (views
into padded buffers, sentinels on both sides); stream-major cells also equal the rows result on the transposed buffer.  No tolerance and
no skip anywhere: what the planner refuses is fuzz_bodies.UNREACHABLE, asserted in test_fuzz_bodies_host.py, and is no cell.

One MI355X, the kernel cache build() leaves: 350 tests in 6.3 s."""
import numpy as np
import pytest

import fuzz_bodies as FB

pytestmark = pytest.mark.gpu
PAD, SENTINEL, STATE_SENTINEL = 64, 12345.0, 777.0


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    t.cuda.set_device(0)
    return t


@pytest.fixture(scope="module")
def F():
    from zignal_amd import flowz
    assert flowz.device_count() >= 1
    return flowz


_WANT = {}


def expected(torch, F, pin):
    """(frames, the oracle's output, the plain kernel's output and state) of a cell, computed once per (graph, shape, frame type): the cells
    that share them follow one another"""
    ns, T = pin["shape"]
    f64 = FB.out_f64(pin)
    key = (pin["family"], pin["seed"], ns, T, f64)
    if key not in _WANT:
        g = FB.graph(pin["family"], pin["seed"])
        x, wires = FB.frames(pin["family"], pin["seed"], np.arange(ns), T)
        want, _ = FB.oracle_run(pin["family"], pin["seed"], x, wires, out_f64=f64)
        assert FB.all_finite(g, want), key
        y0, st0 = run(torch, F, g["prog"], "rows", x, FB.plain_of(g, ns, T, f64), 0, T, None, 0)
        _WANT.clear()
        _WANT[key] = (x, want, y0, st0.cpu().numpy())
    return _WANT[key]


def padded(torch, shape, dtype, sentinel, fill=None):
    """(the whole buffer, a view of `shape` into it with PAD sentinels on both sides)"""
    n = int(np.prod(shape))
    big = torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device="cuda")
    if fill is not None:
        big[PAD:PAD + n] = fill
    view = big[PAD:PAD + n].view(*shape)
    assert view.data_ptr() % 16 == 0
    return big, view


def untouched(big, sentinel):
    b = big.cpu().numpy()
    return bool((b[:PAD] == sentinel).all() and (b[-PAD:] == sentinel).all())


def run(torch, F, prog, layout, x, v, t0, t1, state, tile, guard=False):
    """rows [t0, t1) of the frames x (host, [T, ns, slots]) through variant v in the given layout, from `state` (device); returns the output
    as host [t1 - t0, ns, n_out] and the state.  guard: `out` and `state` are views into padded buffers whose sentinels must not change"""
    var = FB.variant(v, layout)
    f64 = bool(v and v[3] & FB.OUT64)
    ns, n = x.shape[1], t1 - t0
    rows = (n + 3) // 4 * 4 if layout == "sm" else n
    oshape = (ns, rows, prog.n_out) if layout == "sm" else (n, ns, prog.n_out)
    out = sbig = obig = None
    if guard:
        assert layout != "tiles"
        obig, out = padded(torch, oshape, torch.float64 if f64 else torch.float32, SENTINEL)
        sbig, sview = padded(torch, (max(prog.n_state, 1), ns), torch.float32, STATE_SENTINEL, fill=0)
        if state is not None:
            sview.copy_(state)
        state = sview
    if layout == "sm":                                          # a buffer of its own per block (rows a multiple of 4 floats)
        buf = np.zeros((ns, rows, x.shape[2]), np.float32)
        buf[:, :n] = np.transpose(x[t0:t1], (1, 0, 2))
        if out is None:
            out = torch.zeros(oshape, dtype=torch.float32, device="cuda")
        y, st = prog.run_block_stream_major(torch.from_numpy(buf).cuda(), state=state, out=out, variant=var, row0=0, n_samples=n)
        y = y[:, :n].permute(1, 0, 2).cpu().numpy()
    else:
        xd = torch.from_numpy(np.ascontiguousarray(x[t0:t1])).cuda()
        if layout == "tiles":
            y, st = prog.run_block(F.to_tiled(xd, tile), state=state, variant=var, out_f64=f64)
            y = F.from_tiled(y).cpu().numpy()
        else:
            y, st = prog.run_block(xd, state=state, out=out, variant=var, out_f64=f64)
            y = y.cpu().numpy()
    if guard:
        assert untouched(obig, SENTINEL), "a sentinel next to out has changed"
        assert untouched(sbig, STATE_SENTINEL), "a sentinel next to the state rows has changed"
        st = st.clone()
    return y, st


def same_words(a, b):
    """two states word for word: double lines hold double words, no float of its own"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("cid", list(FB.CELLS), ids=str)
def test_random_graph_on_kernel_body(torch, F, cid):
    pin = FB.CELLS[cid]
    g = FB.graph(pin["family"], pin["seed"])
    prog, layout, (ns, T), tile, cut = g["prog"], pin["layout"], pin["shape"], pin["tile"], pin["cut"]
    v = None if pin["variant"] is None else tuple(pin["variant"])
    after = tuple(pin["after"])
    assert prog.kernel_name(FB.variant(v, layout), ns, T, tile) == pin["kernel"], cid
    guard = layout != "tiles" and (ns == 2 or pin["kernel"].endswith("M"))
    assert guard or not (pin["body"].startswith("ragged") or ns == 2)
    x, want, y0, st0 = expected(torch, F, pin)
    # one block: the oracle's output on every stream, the plain kernel's state
    y, st = run(torch, F, prog, layout, x, v, 0, T, None, tile, guard)
    assert FB.ndiff(y, want) == 0, cid
    assert same_words(st.cpu().numpy(), st0), cid
    if layout == "sm":                                          # the rows result of the same cell on the transposed buffer
        assert FB.ndiff(y, y0) == 0, cid
    # two chained blocks: this body up to the cut, another one behind it
    y1, s1 = run(torch, F, prog, layout, x, v, 0, cut, None, tile, guard)
    y2, s2 = run(torch, F, prog, layout, x, after, cut, T, s1, tile, guard)
    assert FB.ndiff(np.concatenate([y1, y2]), want) == 0, cid
    assert same_words(s2.cpu().numpy(), st0), cid
