"""Graph functions (abs, sqrt, exp, tanh, min, max) on the MI355X: the kernels' bits against the numpy restatement of tests/fn_ref.py
(NaNs of any payload equal), the three nonlinear workloads against their hand-written recurrences on every launch path, and a hard
clipper spelled with min / max against the existing oracle."""
import numpy as np
import pytest

import fn_ref as R
from oracle import flowz_oracle as O
from zignal_amd import workloads as W

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SEED = 20161207


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


def ndiff(a, b):
    """differing bit patterns, NaNs of any payload equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    I = np.uint32 if a.dtype == F32 else np.uint64
    return int(((a.view(I) != b.view(I)) & ~(np.isnan(a) & np.isnan(b))).sum())


def edge_values(T):
    f = np.finfo(T)
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, f.tiny, -f.tiny, f.smallest_subnormal, -f.smallest_subnormal, f.max, -f.max, 1.0, -1.0,
         0.55, -0.55, 10.0, -10.0, 20.0, -20.0, 9.0, 19.0, 88.72283172607422, 88.72283935546875, -103.97, -104.0, 709.782712893383973096,
         709.7827128933841, -745.13, -746.0, 2.0 ** -12, 2.0 ** -27, 0.5, -0.5]
    return np.array(v, T)


def random_bits(T, shape, seed):
    """bit patterns over the whole range of T (every exponent, NaNs included), plus the special values and thresholds"""
    rng = np.random.default_rng(seed)
    I = np.uint32 if T == F32 else np.uint64
    x = rng.integers(0, np.iinfo(I).max, size=shape, dtype=I, endpoint=True).view(T)
    # a third of the samples in the range where the functions do their work (|x| < 2^8, every exponent down to the subnormals)
    n = x.size // 3
    e = rng.integers(-30, 8, n)
    x.reshape(-1)[:n] = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.ldexp(rng.random(n) + 1, e)).astype(T)
    ev = edge_values(T)
    x.reshape(-1)[n:n + 4 * len(ev)] = np.tile(ev, 4)
    return x


NAMES = ["abs", "sqrt", "exp", "tanh", "min", "max"]


def function_bank(F):
    """the six functions of (_1, _2) side by side: outputs abs(_1), sqrt(_1), exp(_1), tanh(_1), min(_1, _2), max(_1, _2)"""
    _1, _2 = F.placeholder(1), F.placeholder(2)
    return F.chan(F.abs(_1), F.sqrt(_1), F.exp(_1), F.tanh(_1), F.min(_1, _2), F.max(_1, _2))


def want_bank(a, b):
    return [R.fabs(a), R.sqrt(a), R.exp(a), R.tanh(a), R.fmin(a, b), R.fmax(a, b)]


@pytest.mark.parametrize("P", [1, 2, 4])
def test_every_function_float_bits(torch, F, P):
    prog = F.compile(function_bank(F))
    T, ns = 64, 4096
    x = random_bits(F32, (T, ns, 2), SEED + P)
    y, _ = prog.run_block(torch.from_numpy(x).cuda(), variant=F.make_variant(P, 8))
    y = y.cpu().numpy()
    for k, (name, w) in enumerate(zip(NAMES, want_bank(x[..., 0], x[..., 1]))):
        assert ndiff(y[..., k], w) == 0, name


@pytest.mark.parametrize("P", [1, 2, 4])
def test_every_function_double_bits_on_a_typed_f64_graph(torch, F, P):
    """fz_compile_typed with FZ_DT_F64 input wires: the functions in double, the double results leave the frame unrounded"""
    dts = ["f64", "f64"]
    prog = F.compile(function_bank(F), in_dtypes=dts)
    T, ns = 32, 2048
    a, b = random_bits(F64, (T, ns), SEED + 10 + P), random_bits(F64, (T, ns), SEED + 20 + P)
    frames = F.pack_typed([a, b], dts)
    y, _ = prog.run_block(torch.from_numpy(frames).cuda(), variant=F.make_variant(P, 8))
    outs = F.unpack_typed(y.cpu().numpy(), ["f64"] * 6)
    for name, got, w in zip(NAMES, outs, want_bank(a, b)):
        assert ndiff(got, w) == 0, name


def test_double_operands_in_an_untyped_graph(torch, F):
    """tanh(0.5 * _1) with the C++ double literal: a double tanh, narrowed to the float frame once"""
    _1 = F.placeholder(1)
    prog = F.compile(F.chan(F.tanh(F.lit64(0.5) * _1), F.exp(F.lit64(1.0) * _1), F.min(_1, F.lit64(0.25)), F.sqrt(F.lit64(1.0) * _1)))
    x = random_bits(F32, (32, 1024, 1), SEED + 30)
    y, _ = prog.run_block(torch.from_numpy(x).cuda())
    xd = x[..., 0].astype(F64)
    want = [R.tanh(F64(0.5) * xd), R.exp(xd), R.fmin(xd, np.full_like(xd, 0.25)), R.sqrt(xd)]
    y = y.cpu().numpy()
    for k, w in enumerate(want):
        assert ndiff(y[..., k], w.astype(F32)) == 0, k


# ---- the workloads ---------------------------------------------------------------------------------------------------------
def workload(name):
    return {"moog_ladder": W.moog_ladder, "soft_clip_cascade": W.soft_clip_cascade, "envelope_follower": W.envelope_follower}[name]()


def reference(name, x, g):
    if name == "moog_ladder":
        return R.moog_ladder_ref(x, g, W.MOOG_RESONANCE)
    if name == "soft_clip_cascade":
        return R.soft_clip_cascade_ref(x, [W.SOFT_CLIP] * 4)
    return R.envelope_follower_ref(x, W.ENV_ATTACK, W.ENV_RELEASE)


def cutoffs(ns, seed=SEED):
    return (0.05 + 0.6 * np.random.default_rng(seed).random(ns)).astype(F32)


@pytest.mark.parametrize("name", ["moog_ladder", "soft_clip_cascade", "envelope_follower"])
def test_workloads_on_every_launch_path(torch, F, name):
    """run_block, two chained blocks, stream-major buffers, stream tiles and run_window against the recurrence written from the equations"""
    prog = F.compile(F.from_sexpr(workload(name)))
    ns, T = 2048, 256
    x = (O.synth_input(SEED + 1, np.arange(ns), T)[..., 0] * 3).astype(F32)
    g = cutoffs(ns)
    want = reference(name, x, g)
    xd = torch.from_numpy(x[..., None]).cuda()
    pd = torch.from_numpy(g[None]).cuda() if prog.n_param else None
    y, _ = prog.run_block(xd, params=pd)
    assert ndiff(y.cpu().numpy()[..., 0], want) == 0, "run_block"
    y1, st = prog.run_block(xd[:100].contiguous(), params=pd)
    y2, _ = prog.run_block(xd[100:].contiguous(), state=st, params=pd)
    assert ndiff(torch.cat([y1, y2]).cpu().numpy()[..., 0], want) == 0, "chained blocks"
    xs = xd[..., 0].t().contiguous()[..., None]
    ysm, _ = prog.run_block_stream_major(xs, params=pd)
    assert ndiff(ysm.cpu().numpy()[..., 0].T, want) == 0, "stream-major"
    yt, _ = prog.run_block(F.to_tiled(xd, 512), params=pd)
    assert ndiff(F.from_tiled(yt).cpu().numpy()[..., 0], want) == 0, "tiles"
    out = torch.empty_like(xd)
    st = torch.zeros((prog.n_state, ns), dtype=torch.float32, device="cuda")
    prog.run_window(xd, out, st, 0, 96, params=pd)
    prog.run_window(xd, out, st, 96, T - 96, params=pd)
    assert ndiff(out.cpu().numpy()[..., 0], want) == 0, "run_window"


def test_moog_ladder_default_plan_at_the_headline_shape(torch, F):
    """1 048 576 x 4096 on the library's default plan, 2048 sampled streams checked; then every stream of 65 536 x 1024"""
    prog = F.compile(F.from_sexpr(W.moog_ladder()))
    ns, T = 1 << 20, 4096
    x = torch.empty((T, ns, 1), dtype=torch.float32, device="cuda")
    F.synth_fill(x, seed=SEED + 2)
    g = cutoffs(ns, SEED + 3)
    y, _ = prog.run_block(x, params=torch.from_numpy(g[None]).cuda())
    ids = np.unique(np.concatenate([np.arange(8), np.random.default_rng(9).integers(0, ns, 2040), np.arange(ns - 8, ns)]))
    idd = torch.as_tensor(ids, device="cuda")
    got = y[:, idd, 0].cpu().numpy()
    xh = x[:, idd, 0].cpu().numpy()
    del x, y
    assert np.array_equal(xh, O.synth_input(SEED + 2, ids, T)[..., 0])
    assert ndiff(got, R.moog_ladder_ref(xh, g[ids], W.MOOG_RESONANCE)) == 0
    ns, T = 65536, 1024
    x = (O.synth_input(SEED + 4, np.arange(ns), T)[..., 0] * 2).astype(F32)
    g = cutoffs(ns, SEED + 5)
    y, _ = prog.run_block(torch.from_numpy(x[..., None]).cuda(), params=torch.from_numpy(g[None]).cuda())
    assert ndiff(y.cpu().numpy()[..., 0], R.moog_ladder_ref(x, g, W.MOOG_RESONANCE)) == 0


def test_min_max_clipper_equals_the_comparison_clipper_of_the_oracle(torch, F):
    """min(max(x, lo), hi) and workloads.hard_clipper give the same bits where neither -0, NaN nor an infinity occurs (the comparison
    spelling multiplies x by 0 outside [lo, hi]: inf * 0 is NaN); the comparison clipper is checked against the existing oracle, so this
    check does not rest on tests/fn_ref.py"""
    lo, hi = -0.5, 0.5
    _1 = F.placeholder(1)
    prog = F.compile(F.min(F.max(_1, lo), hi))
    ns, T = 1024, 128
    x = (O.synth_input(SEED + 6, np.arange(ns), T) * 2).astype(F32)
    x[~np.isfinite(x) | ((x == 0) & np.signbit(x))] = 0.0
    x.reshape(-1)[:8] = [lo, hi, 1e30, -1e30, 1e-40, -1e-40, np.nextafter(F32(hi), F32(1)), np.nextafter(F32(lo), F32(-1))]
    y, _ = prog.run_block(torch.from_numpy(x).cuda())
    with np.errstate(all="ignore"):
        want = O.compile(W.hard_clipper(lo, hi), ns).run(x)
    assert ndiff(y.cpu().numpy(), np.asarray(want, F32).reshape(y.shape)) == 0


# ---- random graphs ---------------------------------------------------------------------------------------------------------
def random_graph(rng, depth=4):
    """a one-in one-out graph mixing the functions with the operators, delays and (sometimes) a feedback loop"""
    def leaf(fb):
        r = rng.random()
        if r < 0.35:
            return W.IN(2 if fb else 1)
        if r < 0.55:
            return W.DEL(1, int(rng.integers(1, 3)))
        if r < 0.65:
            return W.lit64(float(rng.uniform(-2, 2)))
        return W.lit(float(rng.uniform(-2, 2)))

    def node(d, fb):
        if d == 0:
            return leaf(fb)
        r = rng.random()
        if r < 0.4:                                          # (sqrt of |a| and exp of a bounded value: fewer NaN and inf to carry around)
            f = str(rng.choice(["abs", "sqrt", "exp", "tanh"]))
            c = node(d - 1, fb)
            return ("sqrt", ("abs", c)) if f == "sqrt" else ("exp", ("mul", W.lit(3.0), ("tanh", c))) if f == "exp" else (f, c)
        if r < 0.55:
            return (str(rng.choice(["min", "max"])), node(d - 1, fb), node(d - 1, fb))
        if r < 0.6:
            return ("lt", node(d - 1, fb), node(d - 1, fb))
        if r < 0.65:
            return ("neg", node(d - 1, fb))
        return (str(rng.choice(["add", "sub", "mul", "div"])), node(d - 1, fb), node(d - 1, fb))

    if rng.random() < 0.4:                                   # a loop: ~f(_1[_n], _2)
        return W.fb(("tanh", node(depth, True)))
    return node(depth, False)


def test_one_hundred_random_graphs(torch, F):
    """100 random graphs, ten side by side per program (10 kernels, unroll 1: the JIT dominates this test), against the IR evaluator of
    tests/fn_ref.py"""
    rng = np.random.default_rng(SEED + 7)
    ns, T = 256, 48
    checked = 0
    for k in range(10):
        gs = [random_graph(rng) for _ in range(10)]
        e = W.par(*gs)
        prog = F.compile(F.from_sexpr(e))
        x = (O.synth_input(SEED + 100 + k, np.arange(ns), T, n_wires=max(prog.n_in, 1)) * 4).astype(F32)
        x.reshape(-1)[:16] = edge_values(F32)[:16]
        y, _ = prog.run_block(torch.from_numpy(x).cuda(), variant=F.make_variant([1, 2, 4][k % 3], 1, 256))
        want, _ = R.run_ir(prog, x)
        assert ndiff(y.cpu().numpy(), want) == 0, (k, gs)
        checked += len(gs)
    assert checked == 100
