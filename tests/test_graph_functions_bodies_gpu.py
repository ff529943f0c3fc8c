"""Graph functions on every kernel body the planner sends them to (tests/fn_bodies.py): each cell asserts the kernel name of its body,
compares every stream with the IR evaluator of tests/fn_ref.py (NaNs of any payload equal) and, for the workloads, with their hand-written
recurrences; the state after the block equals the plain kernel's; two chained blocks, cut off every chunk and phase boundary and the second
run by another body, give the same output and state.  Then the library's own choice at the smallest shapes that reach each default body,
and a flags-only lockstep request at a stream count the wave-split kernels would otherwise take."""
import numpy as np
import pytest

import fn_bodies as B
import fn_ref as R
from oracle import flowz_oracle as O
from test_graph_functions_gpu import ndiff
from zignal_amd import workloads as W

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


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


_CACHE = {}


def case(name, ns, T):
    """(program, frames, params, modulator rows, the evaluator's output and state) of one graph at one shape, computed once"""
    key = (name, ns, T)
    if key not in _CACHE:
        prog = B.graph(name)
        x, params, mod = B.frames(name, prog, ns, T)
        want, st = R.run_ir(prog, x, params=params, mod=mod, out_f64=name in B.OUT_F64)
        _CACHE.clear()                                             # (one shape at a time: the cells of a shape are consecutive)
        _CACHE[key] = (prog, x, params, mod, want, st)
    return _CACHE[key]


def recurrence(name, x, params):
    x = x[..., 0]
    if name == "moog":
        return R.moog_ladder_ref(x, params[0], W.MOOG_RESONANCE)
    if name == "soft":
        return R.soft_clip_cascade_ref(x, [W.SOFT_CLIP] * 4)
    return R.envelope_follower_ref(x, W.ENV_ATTACK, W.ENV_RELEASE)


def run(torch, F, prog, layout, x, v, params, mod, t0, t1, state, tile, out_f64):
    """rows [t0, t1) of the frames x (host, [T, ns, slots]) through variant v in the given layout, from `state` (device); returns the
    output as host [t1 - t0, ns, n_out] and the state"""
    pd = torch.from_numpy(np.ascontiguousarray(params)).cuda() if params is not None else None
    if mod is not None:
        prog.set_modulation(torch.from_numpy(np.ascontiguousarray(mod[:, t0:t1])).cuda())
    var = B.variant(v, layout)
    if layout == "sm":
        xs = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (1, 0, 2)))).cuda()
        out = torch.zeros((x.shape[1], x.shape[0], prog.n_out), dtype=torch.float32, device="cuda")
        y, st = prog.run_block_stream_major(xs, state=state, params=pd, out=out, variant=var, row0=t0, n_samples=t1 - t0)
        return y[:, t0:t1].permute(1, 0, 2).cpu().numpy(), st
    xd = torch.from_numpy(np.ascontiguousarray(x[t0:t1])).cuda()
    if layout == "tiles":
        y, st = prog.run_block(F.to_tiled(xd, tile), state=state, params=pd, variant=var, out_f64=out_f64)
        return F.from_tiled(y).cpu().numpy(), st
    y, st = prog.run_block(xd, state=state, params=pd, variant=var, out_f64=out_f64)
    return y.cpu().numpy(), st


@pytest.mark.parametrize("cell", B.CELLS, ids=lambda c: c[0])
def test_function_graph_on_kernel_body(torch, F, cell):
    cid, name, layout, v, ns, T, tile, kname, cut, after = cell
    prog, x, params, mod, want, st_ir = case(name, ns, T)
    f64 = name in B.OUT_F64
    assert B.cell_name(prog, cell) == kname, cid
    assert prog.kernel_name(B.variant(after, layout), ns, T, tile) != kname                 # the block after the cut: another body
    y, st = run(torch, F, prog, layout, x, v, params, mod, 0, T, None, tile, f64)
    assert ndiff(y, want) == 0, cid
    if name in ("moog", "soft", "env"):
        assert ndiff(y[..., 0], recurrence(name, x, params)) == 0, cid
    # the state: the plain kernel's, bit for bit (NaNs of any payload equal) -- and, where no ring holds it, the evaluator's
    _, st0 = run(torch, F, prog, "rows", x, B.PLAIN, params, mod, 0, T, None, 0, f64)
    st, st0 = st.cpu().numpy(), st0.cpu().numpy()
    assert ndiff(st, st0) == 0, cid
    if prog.n_lds_slots == 0 and name != "far" and prog.n_state:
        assert ndiff(st0, st_ir) == 0, cid
    # two chained blocks: this body up to the cut, another one after it
    y1, s1 = run(torch, F, prog, layout, x, v, params, mod, 0, cut, None, tile, f64)
    y2, s2 = run(torch, F, prog, layout, x, after, params, mod, cut, T, s1, tile, f64)
    assert ndiff(np.concatenate([y1, y2]), want) == 0, cid
    assert ndiff(s2.cpu().numpy(), st0) == 0, cid


# ---- the library's own choice ------------------------------------------------------------------------------------------------
def _sample_ids(ns, k, seed):
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([[0, 1, 63, 64, ns - 2, ns - 1], rng.integers(0, ns, k)]))


DEFAULT_RUNS = [   # (graph, n_streams, n_samples, tile_streams, stream-major, kernel name)
    ("moog", 1 << 19, 256, 0, True, "fz_block_kernel_p2u64b64f384"),
    ("soft", 1 << 19, 1024, 0, False, "fz_block_kernel_p2u2b1024f8912896"),
    ("moog", 1 << 19, 1024, 8192, False, "fz_block_kernel_p2u2b1024f8912896"),
    ("env", (1 << 18) + 515, 1024, 0, False, "fz_block_kernel_p2u4b512f8912896M"),
    ("lds", 1 << 18, 1024, 0, False, "fz_block_kernel_p1u16b256f8912896"),
    ("far", 1 << 18, 1024, 0, False, "fz_block_kernel_p2u4b512f8912896"),
]


@pytest.mark.parametrize("run_", DEFAULT_RUNS, ids=lambda r: f"{r[0]}-{r[1]}x{r[2]}{'-sm' if r[4] else ''}{'-t%d' % r[3] if r[3] else ''}")
def test_default_plan_reaches_the_function_bodies(torch, F, run_, monkeypatch):
    """No variant: the body by name, the whole output and the state equal to the plain kernel's on the GPU, 256 sampled streams against
    the evaluator.  (1 << 18) + 515 streams: whole laps and a remainder launch.  (At most three frame buffers of 2 GiB at a time.)"""
    monkeypatch.setenv("FLOWZ_HIP_AUTOTUNE", "0")
    monkeypatch.setenv("FLOWZ_HIP_NO_PLAN_CACHE", "1")
    name, ns, T, tile, sm, kname = run_
    prog = B.graph(name)
    assert B.default_name(prog, ns, T, tile, sm) == kname
    x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
    F.synth_fill(x, seed=B.SEED + ns + T)
    x.mul_(3)
    pd = torch.from_numpy(B.cutoffs(ns, B.SEED + 5)[None]).cuda() if prog.n_param else None
    ids = _sample_ids(ns, 256, 7)
    idd = torch.as_tensor(ids, device="cuda")
    xh = x[:, idd].cpu().numpy()
    if tile:                                                   # (the plain kernel on the same tiles: no time-major copy of the output)
        x = F.to_tiled(x, tile)
    y0, st0 = prog.run_block(x, params=pd, variant=F.make_variant(*B.PLAIN))
    if sm:
        xs = x[..., 0].t().contiguous()[..., None]
        ys, st = prog.run_block_stream_major(xs, params=pd)
        del xs
        y = ys.permute(1, 0, 2).contiguous()
        del ys
    else:
        y, st = prog.run_block(x, params=pd)
    del x
    assert torch.equal(y.view(torch.int32), y0.view(torch.int32)) and torch.equal(st.view(torch.int32), st0.view(torch.int32))
    del y0
    got = y[idd // tile, :, idd % tile].permute(1, 0, 2).cpu().numpy() if tile else y[:, idd].cpu().numpy()
    want, _ = R.run_ir(prog, xh, params=None if pd is None else pd.cpu().numpy()[:, ids])
    assert ndiff(got, want) == 0


def test_flags_only_lockstep_request_runs_the_lockstep_frame_kernel(torch, F):
    """make_variant(0, 0, 0, LOCKSTEP[ | GRID_SYNC]) at 40 000 streams, where the library's own choice is the wave-split kernel with two
    I/O waves: the lockstep frame kernel (stage-packed), bit for bit against the oracle"""
    g = W.df1_cascade(6)
    prog = F.compile(F.from_sexpr(g))
    ns, T = 40000, 1100
    assert "f%d" % B.L not in prog.kernel_name(None, ns, T)
    x = O.synth_input(B.SEED + 77, np.arange(ns), T)
    want = O.compile(g, ns).run(x)
    xd = torch.from_numpy(x).cuda()
    for flags, kname in ((B.L, "fz_block_kernel_p1u16b256s6f%d" % (B.L | F.C.FZ_VF_STAGE_PACK)),
                         (B.L | B.GS, "fz_block_kernel_p1u16b256s6f%d" % (B.L | B.GS | F.C.FZ_VF_STAGE_PACK))):
        assert prog.kernel_name(F.make_variant(0, 0, 0, flags), ns, T) == kname
        y, _ = prog.run_block(xd, variant=F.make_variant(0, 0, 0, flags))
        assert ndiff(y.cpu().numpy(), want) == 0, kname
