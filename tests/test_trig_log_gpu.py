"""sin, cos and log on the MI355X: every cell of tests/trig_cells.py bit for bit against fn_ref.run_ir with the functions of
tests/fn_ref_trig.py registered (NaNs of any payload equal), the workloads against their recurrences, two chained blocks across a cut;
16-bit PCM frames in both layouts; both adjoint kernels against tests/adjoint_ref_trig.py and against each other."""
import numpy as np
import pytest

import adjoint_ref_trig as AT
import fn_ref as R
import grad_harness as H
import pcm16_ref as PR
import trig_cells as TC
from grad_harness import dev, make_inputs, on_gpu, on_gpu_sm
from test_graph_functions_bodies_gpu import run
from test_graph_functions_gpu import ndiff

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    from zignal_amd import flowz
    return flowz


_CACHE = {}


def case(name, ns, T):
    """(program, frames, params, the evaluator's output and state) of one graph at one shape, computed once"""
    key = (name, ns, T)
    if key not in _CACHE:
        prog = TC.graph(name)
        x, params = TC.frames(name, prog, ns, T)
        want, st = R.run_ir(prog, x, params=params, out_f64=name in TC.OUT_F64)
        _CACHE[key] = (prog, x, params, want, st)
    return _CACHE[key]


@pytest.mark.parametrize("cell", TC.CELLS, ids=lambda c: c[0])
def test_graph_on_kernel_body(F, cell):
    cid, name, layout, v, ns, T, tile, kname, cut, after = cell
    prog, x, params, want, st_ir = case(name, ns, T)
    f64 = name in TC.OUT_F64
    assert TC.cell_name(prog, cell) == kname, cid
    y, st = run(torch, F, prog, layout, x, v, params, None, 0, T, None, tile, f64)
    assert ndiff(y, want) == 0, cid
    if name in TC.WORKLOADS:
        assert ndiff(y[..., 0], TC.recurrence(name, x, params)) == 0, cid
    if prog.n_state and prog.n_lds_slots == 0:
        assert ndiff(st.cpu().numpy()[:st_ir.shape[0]], st_ir) == 0, cid
    # two chained blocks: this body up to the cut, another one after it
    y1, s1 = run(torch, F, prog, layout, x, v, params, None, 0, cut, None, tile, f64)
    y2, s2 = run(torch, F, prog, layout, x, after, params, None, cut, T, s1, tile, f64)
    assert ndiff(np.concatenate([y1, y2]), want) == 0, cid
    if prog.n_state:
        assert ndiff(s2.cpu().numpy(), st.cpu().numpy()) == 0, cid


# ---- 16-bit PCM frames ---------------------------------------------------------------------------------------------------------
def pcm_input(ns, T, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(-32768, 32768, (T, ns, 1)).astype(np.int16)
    q[0, :4, 0] = (-32768, 32767, 0, -1)
    return q


@pytest.mark.parametrize("out", ["int16", "float32"])
def test_pcm16_frames_wavefolder(F, out):
    prog = TC.graph("fold")
    ns, T = TC.PCM_SHAPES["rows"]
    q = pcm_input(ns, T, 5)
    xf = PR.to_float(q)
    yf, stf = prog.run_block(torch.from_numpy(xf).cuda(), variant=F.make_variant(*TC.PLAIN))
    yf = yf.cpu().numpy()
    assert ndiff(yf, R.run_ir(prog, xf)[0]) == 0
    y, st = prog.run_block_pcm16(torch.from_numpy(q).cuda(), out_dtype=getattr(torch, out))
    if out == "float32":
        assert ndiff(y.cpu().numpy(), yf) == 0
    else:
        assert np.array_equal(y.cpu().numpy(), PR.from_float(yf))
    assert ndiff(st.cpu().numpy(), stf.cpu().numpy()) == 0


def test_pcm16_stream_major_window_wavefolder(F):
    prog = TC.graph("fold")
    ns, rows, row0 = TC.PCM_SHAPES["sm"]
    q = pcm_input(ns, rows, 6)                                   # [rows, ns, 1]
    xf = PR.to_float(q[row0:])
    want = PR.from_float(R.run_ir(prog, xf)[0])
    qs = torch.from_numpy(np.ascontiguousarray(q.transpose(1, 0, 2))).cuda()
    y, _ = prog.run_block_pcm16_stream_major(qs, out_dtype=torch.int16, row0=row0, n_samples=rows - row0)
    assert np.array_equal(y.cpu().numpy()[:, row0:].transpose(1, 0, 2), want)
    yf, _ = prog.run_block_stream_major(torch.from_numpy(np.ascontiguousarray(PR.to_float(q).transpose(1, 0, 2))).cuda(), row0=row0, n_samples=rows - row0)
    assert np.array_equal(PR.from_float(yf.cpu().numpy()[:, row0:].transpose(1, 0, 2)), want)


# ---- backward ------------------------------------------------------------------------------------------------------------------
def check(p, got, want, what):
    H.check(p, got, want, what, H.GRAD_KEYS)


def grad_inputs(p, ns, T, seed):
    return make_inputs(p, "trig", ns, T, seed, ties=False, draw_params=lambda p_, n, rng: rng.uniform(0.01, 0.5, (p_.n_param, n)).astype(F32))


@pytest.mark.parametrize("name", TC.GRAD_GRAPHS)
@pytest.mark.parametrize("C", [0, 4])
def test_both_adjoint_kernels_match_the_restatement_and_each_other(F, name, C):
    p = TC.graph(name)
    ns, T = 130, 37
    x, s0, par, yb, sb, ap, ac = grad_inputs(p, ns, T, 21)
    want = AT.grad(p, x, yb, s0, par, sb, ap, ac)
    tm = on_gpu(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=C)
    check(p, tm, want, f"{name} time-major C={C}")
    sm = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=C)
    check(p, sm, want, f"{name} stream-major C={C}")
    check(p, sm, tm, f"{name} stream-major against time-major C={C}")
    win = on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=C, row0=4)
    check(p, win, want, f"{name} stream-major window at row 4, C={C}")


@pytest.mark.parametrize("name", TC.GRAD_GRAPHS)
def test_two_chained_blocks_give_one_block_of_2T(F, name):
    p = TC.graph(name)
    ns, T = 130, 37
    x, s0, par, yb, sb, ap, ac = grad_inputs(p, ns, 2 * T, 23)
    whole = on_gpu(p, x, s0, par, yb, sb, ap, ac)
    check(p, whole, AT.grad(p, x, yb, s0, par, sb, ap, ac), f"{name} 2T")
    _, s_mid = p.run_block(dev(x[:T]), dev(s0), dev(par), variant=p_plain(F))
    second = on_gpu(p, x[T:], s_mid.cpu().numpy(), par, yb[T:], sb, ap, ac)
    first = on_gpu(p, x[:T], s0, par, yb[:T], second["state"], second["params"], second["consts"])
    chained = {"x": np.concatenate([first["x"], second["x"]]), "state": first["state"], "params": first["params"], "consts": first["consts"]}
    check(p, chained, whole, f"{name} chained")


def p_plain(F):
    return F.make_variant(*TC.PLAIN)
