"""Delay lines of every depth class on every kernel body (tests/delay_cells.py): each cell's output equals oracle.flowz_oracle's bit for bit
(NaNs of any payload equal); the same block cut into chained pieces -- of lengths 1, G - 1, d - 1, d, d + 1 and a long one, alternating
between the cell's body and a plain free-running kernel, state handed on -- gives the same output; the state after one block equals the
plain kernel's (HBM rings, whose rows are a ring with a phase: compared through one more block run from both states).  No cell is skipped
or tolerated here: what the planner refuses is asserted in test_delay_lines_host.py and is no cell."""
import numpy as np
import pytest

import delay_cells as D
from test_graph_functions_gpu import ndiff

pytestmark = pytest.mark.gpu
PINS = D.load_pins()


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


def expected(c):
    """(frames, the typed wires or None, the oracle's output) of a cell, computed once per graph and shape (cells that share them are consecutive)"""
    key = (c["tmpl"], c["args"], c["dtype"], c["ns"], c["T"] + c["tail"])
    if key not in _WANT:
        x, wires = D.frames(c)
        want = D.oracle_run(c, x=x, wires=wires)
        ok = np.ones(c["ns"], bool)
        ok[D.edge_streams(c)] = False
        assert D.all_finite(c, want[:, ok]), c["id"]
        _WANT.clear()
        _WANT[key] = (x, wires, want)
    return _WANT[key]


def run(torch, F, prog, c, x, v, layout, t0, t1, state):
    """rows [t0, t1) of the frames x (host, [T, ns, slots]) through variant v in the given layout, from `state` (device); returns the output
    as host [t1 - t0, ns, n_out] and the state"""
    var = None if v is None else F.make_variant(v[0], v[1], v[2], v[3] | (D.SM if layout == "sm" else 0))
    if layout == "sm":                                          # a buffer of its own per block (rows a multiple of 4 floats)
        n, w = t1 - t0, x.shape[2]
        rows = (n + 3) // 4 * 4
        buf = np.zeros((x.shape[1], rows, w), np.float32)
        buf[:, :n] = np.transpose(x[t0:t1], (1, 0, 2))
        out = torch.zeros((x.shape[1], rows, prog.n_out), dtype=torch.float32, device="cuda")
        y, st = prog.run_block_stream_major(torch.from_numpy(buf).cuda(), state=state, out=out, variant=var, row0=0, n_samples=n)
        return y[:, :n].permute(1, 0, 2).cpu().numpy(), st
    xd = torch.from_numpy(np.ascontiguousarray(x[t0:t1])).cuda()
    if layout == "tiles":
        y, st = prog.run_block(F.to_tiled(xd, c["tile"]), state=state, variant=var)
        return F.from_tiled(y).cpu().numpy(), st
    y, st = prog.run_block(xd, state=state, variant=var)
    return y.cpu().numpy(), st


@pytest.mark.parametrize("c", D.CELLS, ids=lambda c: c["id"])
def test_delay_cell_matches_the_oracle(torch, F, c):
    cid = c["id"]
    name, P, U, B, G, slots, how = PINS[cid]
    prog = D.compile_cell(c)
    assert D.cell_name(prog, c) == name, cid
    x, wires, want = expected(c)
    T, total = c["T"], c["T"] + c["tail"]
    far = any(D.storage(dl) == "far" for dl, _ in D.reads(c["tmpl"], c["args"]))
    # one block
    y, st = run(torch, F, prog, c, x, c["v"], c["layout"], 0, T, None)
    assert ndiff(y, want[:T]) == 0, cid
    # its state: the plain kernel's
    plain = D.plain(c)
    y0, st0 = run(torch, F, prog, c, x, plain, "rows", 0, T, None)
    assert ndiff(y0, want[:T]) == 0, cid
    if far:
        # ring rows and a phase: one more block from both states, against the oracle -- the d + 2 samples behind a short block, else the
        # block's first samples once more
        if c["tail"]:
            t0, t1, more = T, total, want[T:]
        else:
            t0, t1 = 0, min(T, c["d"] + 3)
            again = None if wires is None else [np.concatenate([w[:T], w[:t1]]) for w in wires]
            more = D.oracle_run(c, x=np.concatenate([x[:T], x[:t1]]), wires=again)[T:]
        ya, _ = run(torch, F, prog, c, x, plain, "rows", t0, t1, st.clone())
        yb, _ = run(torch, F, prog, c, x, plain, "rows", t0, t1, st0.clone())
        assert ndiff(ya, more) == 0 and ndiff(yb, more) == 0, cid
    else:
        assert ndiff(st.cpu().numpy(), st0.cpu().numpy()) == 0, cid
    # chained pieces, this body and the other one in turn
    other = D.other_body(c)
    outs, pos, state = [], 0, None
    for k, n in enumerate(D.pieces(c, G, U)):
        own = k % 2 == 0
        yk, state = run(torch, F, prog, c, x, c["v"] if own else other, c["layout"] if own else "rows", pos, pos + n, state)
        outs.append(yk)
        pos += n
    assert pos == total and ndiff(np.concatenate(outs), want) == 0, cid
    if not far:                                                  # the state behind the whole chain: the plain kernel's over the same samples
        if c["tail"]:
            _, st0 = run(torch, F, prog, c, x, plain, "rows", 0, total, None)
        assert ndiff(state.cpu().numpy(), st0.cpu().numpy()) == 0, cid


import test_delay_lines_host as H  # noqa: E402  (the seed ranges, checked there with the oracle alone)


@pytest.mark.parametrize("chunk", range(H.DEEP_GPU_CHUNKS))
def test_kernels_match_oracle_on_random_graphs_with_deep_delays(torch, F, chunk):
    """randgraphs.make_deep: the random graphs with a share of their delays in LDS and HBM rings -- P in {1, 2, 4} with the library's chunk
    (within the far lines' cap), a chained split, stream-major buffers where no line is far"""
    from oracle import flowz_oracle as O
    ns, T = H.DEEP_GPU_SHAPE
    n = 0
    for seed in H.deep_gpu_seeds(chunk):
        u = H.usable_deep(seed)
        if u is None:
            continue
        g, n_in, n_out = u
        p = F.compile(F.from_sexpr(g))
        x = O.synth_input(seed, np.arange(ns), T, n_wires=n_in)
        want = O.compile(g, ns).run(x)
        xd = torch.from_numpy(x).cuda()
        for P in H.DEEP_PACKINGS[seed]:
            y, _ = p.run_block(xd, variant=F.make_variant(P, 0))
            assert ndiff(y.cpu().numpy(), want) == 0, f"seed {seed} P={P}: {g}"
        ya, st = p.run_block(xd[:419].contiguous())
        yb, st = p.run_block(xd[419:].contiguous(), state=st)
        assert ndiff(torch.cat([ya, yb]).cpu().numpy(), want) == 0, f"seed {seed} chained"
        if p.max_delay <= D.LDS_MAX and (T * n_in) % 4 == 0 and (T * n_out) % 4 == 0:
            xs = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (1, 0, 2)))).cuda()
            ys, _ = p.run_block_stream_major(xs)
            assert ndiff(ys.permute(1, 0, 2).contiguous().cpu().numpy(), want) == 0, f"seed {seed} stream-major"
        n += 1
    assert n >= H.DEEP_GPU_MIN
