"""What the GPU tests of the backward family share: bitwise comparison, device copies, sentinel-guarded buffers, the transposition
between the two layouts, the input draws, one check() and ONE launch() through the C ABI for every corner of the family (plain or ring,
dL/dy or loss, time-major block or stream-major window, one block or a whole recording), plus the calls through the Python front doors
that more than one test file makes.  Imports without torch and without a GPU: torch is imported inside the functions that need it.
tests/test_grad_harness_host.py holds the primitives to their word on CPU tensors."""
import ctypes

import numpy as np

F32 = np.float32
SENTINEL = np.float32(-1234.5)
PAD = 64                                                          # floats of sentinel on either side (the middle stays 16-byte aligned)
FILL = 7.0                                                        # what x, dL/dy and the target hold outside a window: it must not matter
GRAD_KEYS = ("x", "state", "params", "consts")
LOSS_KEYS = GRAD_KEYS + ("loss", "out")
OUT = {"x": "in_grad", "state": "state0_grad", "params": "param_grad", "consts": "const_grad", "loss": "loss", "out": "out"}


def gpu_flowz():
    """zignal_amd.flowz for the module-scoped F fixture of a GPU test file; skips without an MI355X"""
    import pytest
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from zignal_amd import flowz
    return flowz


def same(a, b):
    """bit for bit, a NaN of any payload equal to a NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def dev(a, device="cuda"):
    import torch
    return torch.from_numpy(np.array(a, F32, order="C")).to(device) if a is not None else None     # (a copy: the cases are read-only)


# ---- transposition ---------------------------------------------------------------------------------------------------------------------
def up4(n):
    return (n + 3) // 4 * 4


def to_sm(a, rows=None, row0=0, fill=0.0):
    """time-major [T][ns][w] -> stream-major [ns][rows][w] with the block at rows [row0, row0 + T), `fill` around it"""
    T, ns, w = a.shape
    rows = up4(row0 + T) if rows is None else rows
    out = np.full((ns, rows, w), fill, F32)
    out[:, row0:row0 + T] = a.transpose(1, 0, 2)
    return out


def from_sm(a, T, row0=0):
    """the window's rows of a stream-major buffer, time-major"""
    return np.ascontiguousarray(a[:, row0:row0 + T].transpose(1, 0, 2))


def grid(p, n):
    """the next row count whose frames of both widths lie on the float4 grid (rows_total and row0 of a stream-major window)"""
    while (n * p.n_in) % 4 or (n * p.n_out) % 4:
        n += 1
    return n


def outside_keeps_sentinel(buf, row0, T):
    keep = np.ones(buf.shape[1], bool)
    keep[row0:row0 + T] = False
    return bool(np.all(buf[:, keep].view(np.uint32) == SENTINEL.view(np.uint32)))


class Guarded:
    """a buffer of `shape` floats between two runs of PAD sentinels; init: what the middle starts from (None: sentinels too)"""

    def __init__(self, shape, init=None, device="cuda"):
        import torch
        self.n = int(np.prod(shape))
        self.buf = torch.full((2 * PAD + self.n,), float(SENTINEL), device=device)
        self.mid = self.buf[PAD:PAD + self.n].view(*shape)
        if init is not None:
            self.mid.copy_(dev(init, device).view(*shape))
        self.before = self.buf.clone()

    def guards_kept(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())

    def untouched(self):
        import torch
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


def check(p, got, want, what, keys, require=False):
    """every key of `keys` that `got` holds equals `want`'s bit for bit, the per-stream rows cut to the graph's counts.  A key `got` holds
    and `want` does not fails.  require: a key of `keys` that `got` lacks fails too (a result that went missing does not pass unseen)"""
    n = {"state": p.n_state, "params": p.n_param, "consts": p.n_const, "state_out": p.n_state}
    for key in keys:
        if key not in got and not require:
            continue
        assert key in got and key in want, f"{what}: {key} is missing ({sorted(got)} against {sorted(want)})"
        g, w = np.asarray(got[key], F32), np.asarray(want[key], F32)
        if key in n:
            g, w = g[:n[key]], w[:n[key]]
        assert same(g, w), f"{what}: {key} differs in {int((~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))).sum()) if g.shape == w.shape else 'shape'} of {g.size}"


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def make_inputs(p, name, ns, T, seed, ties=None, draw_params=None, special_every=1):
    """x, state, params, dL/dy, dL/d(state after) and the two accumulators, none of them zero.  ties (default: by name): the ties and
    specials below mixed into x -- special_every = k: only into every k-th stream, the others stay finite (behind a feedback a NaN
    never leaves its stream); draw_params(p, ns, rng): the per-stream coefficients of a graph that is none of the named ones"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ns, p.n_in)) * 0.5).astype(F32)
    if name == "div_sqrt_exp":
        x = np.abs(x)
    if name in ("rules", "envelope_follower", "clipped_biquad") if ties is None else ties:
        # ties of MIN / MAX (equal values, +0 against -0), +-0 under ABS, NaN and inf through the comparisons
        special = np.array([0.0, -0.0, 1.0, 0.5, np.nan, np.inf, -np.inf, 0.75], F32)
        m = rng.random(x.shape) < 0.2
        m[:, np.arange(ns) % special_every != 0] = False
        x[m] = special[rng.integers(0, special.size, int(m.sum()))]
        if p.n_in >= 2:
            tie = rng.random((T, ns)) < 0.2
            x[:, :, 1][tie] = x[:, :, 0][tie]
    s0 = (rng.standard_normal((p.n_state, ns)) * 0.1).astype(F32)
    par = None
    if p.n_param:
        if draw_params is not None:
            par = draw_params(p, ns, rng)
        elif name == "moog_ladder":
            par = rng.uniform(0.05, 0.5, (1, ns)).astype(F32)
        elif name == "osc_chain6":
            import graphs as G
            par = np.asarray(G.osc_chain_params(G.SEED, np.arange(ns)), F32)
        else:
            import graphs as G
            par = np.empty((p.n_param, ns), F32)
            for j in range(p.n_param // 5):
                par[5 * j:5 * j + 5] = np.asarray(G.STABLE, F32)[:, None] * rng.uniform(0.9, 1.0, (5, ns)).astype(F32)
    yb = rng.standard_normal((T, ns, p.n_out)).astype(F32)
    sb = rng.standard_normal((p.n_state, ns)).astype(F32)
    ap = rng.standard_normal((p.n_param, ns)).astype(F32)
    ac = rng.standard_normal((p.n_const, ns)).astype(F32)
    return x, s0, par, yb, sb, ap, ac


# ---- one launch through the C ABI ------------------------------------------------------------------------------------------------------
# (ring, loss, window, recording) -> the entry point.  Spelled out here, not taken from zignal_amd.flowz: a test that picks the function
# through the code under test says less.
ENTRY = {
    (False, False, False, False): "fz_run_block_grad",
    (False, True, False, False): "fz_run_block_loss_grad",
    (False, False, True, False): "fz_run_block_grad_stream_major",
    (False, True, True, False): "fz_run_block_loss_grad_stream_major",
    (True, False, False, False): "fz_run_block_ring_grad",
    (True, True, False, False): "fz_run_block_ring_loss_grad",
    (True, False, True, False): "fz_run_block_ring_grad_stream_major",
    (True, True, True, False): "fz_run_block_ring_loss_grad_stream_major",
    (False, False, False, True): "fz_run_recording_grad",
    (False, True, False, True): "fz_run_recording_loss_grad",
    (False, False, True, True): "fz_run_recording_grad",
    (False, True, True, True): "fz_run_recording_loss_grad",
    (True, False, False, True): "fz_run_recording_ring_grad",
    (True, True, False, True): "fz_run_recording_ring_loss_grad",
    (True, False, True, True): "fz_run_recording_ring_grad_stream_major",
    (True, True, True, True): "fz_run_recording_ring_loss_grad_stream_major",
}


def launch(p, d, ring=False, loss=False, window=None, recording=None, c=0, state_grad=True, alias=False, leave_out=(), k=1.0, frames=None):
    """One call through the C ABI on the time-major draw d = (x, s0, par, dL/dy, sb, ap, ac) or, under the loss, (x, s0, par, target, sb,
    ap, ac, al): dict of the outputs asked for (numpy).  param_grad, const_grad and loss start from ap / ac / al.
    ring: the ring family's entry point and workspace.  loss: the squared-error call, grad_scale = k.
    window: None (time-major frames), or (rows, row0): stream-major buffers of `rows` rows (None: up4(row0 + T)) with the block at
    [row0, row0 + T), FILL around it in x, dL/dy and the target; "x" and "out" come back as the window's rows, time-major, and
    "x_buffer" / "out_buffer" are the whole buffers.  frames: a dict that keeps the in_grad / out buffers from one launch to the next
    (consecutive windows fill one buffer).
    recording: None (one block), or the block_rows of the call over a whole recording (0: the library's choice); "starts" (the head of
    the workspace) and "state_out" come back too.
    c: checkpoint_rows.  alias: state0_grad is the state_grad buffer.  leave_out: C names of outputs passed as null.
    Afterwards: every input kept its bits (state_grad excepted when aliased); the workspace is exactly the queried bytes and its
    surroundings and those of every output kept their sentinels; an output that is left out, has zero rows or is aliased away was not
    written at all; the rows of in_grad / out outside a window hold what they held before the launch."""
    import torch
    from zignal_amd import _capi as CA
    x, s0, par, yt, sb, ap, ac = d[:7]
    T, ns, _ = x.shape
    rec = recording is not None
    rows, row0 = (None, 0) if window is None else window
    if window is not None and rows is None:
        rows = up4(row0 + T)
    frame = (lambda a: dev(a)) if window is None else (lambda a: dev(to_sm(a, rows, row0, FILL)))
    fshape = (lambda w: (T, ns, max(w, 1))) if window is None else (lambda w: (ns, rows, max(w, 1)))
    ins = {"in_": frame(x), "state": dev(s0), "params": dev(par), "target" if loss else "out_grad": frame(yt),
           "state_grad": dev(sb) if state_grad else None}
    before = {key: v.clone() for key, v in ins.items() if v is not None}
    n = {"in_grad": p.n_in, "state0_grad": p.n_state, "param_grad": p.n_param, "const_grad": p.n_const, "loss": 1, "out": p.n_out,
         "state_out": p.n_state}
    frames = {} if frames is None else frames
    frames.setdefault("in_grad", Guarded(fshape(p.n_in)))
    outs = {"in_grad": frames["in_grad"], "state0_grad": Guarded((max(p.n_state, 1), ns)),
            "param_grad": Guarded((max(p.n_param, 1), ns), ap if p.n_param else None),
            "const_grad": Guarded((max(p.n_const, 1), ns), ac if p.n_const else None)}
    if loss:
        frames.setdefault("out", Guarded(fshape(p.n_out)))
        outs.update(loss=Guarded((ns,), d[7]), out=frames["out"])
    if rec:
        outs["state_out"] = Guarded((max(p.n_state, 1), ns))
    for g in outs.values():
        g.before = g.buf.clone()                                  # (a buffer kept in `frames` holds the earlier window's rows)
    if rec:
        wsb = p.ring_recording_workspace_bytes(ns, T, recording, c) if ring else p.recording_workspace_bytes(ns, T, recording, c, window is not None)
        assert wsb % 4 == 0
    else:
        wsb = (p.ring_grad_workspace_bytes if ring else p.grad_workspace_bytes)(ns, T, c)
    ws = Guarded(((wsb + 3) // 4,))
    a = CA.LossGradArgs() if loss else CA.GradArgs()
    a.struct_size, a.checkpoint_rows = ctypes.sizeof(a), c
    if loss:
        a.grad_scale = k
    for key, t in ins.items():
        setattr(a, key, t.data_ptr() if t is not None and t.numel() else None)
    for key, g in outs.items():
        if key != "state_out":
            setattr(a, key, g.mid.data_ptr() if n[key] and key not in leave_out else None)
    if alias:
        a.state0_grad = ins["state_grad"].data_ptr()
    a.workspace, a.workspace_bytes = ws.mid.data_ptr(), wsb
    fn = getattr(CA.lib, ENTRY[(bool(ring), bool(loss), window is not None, rec)])
    hs = torch.cuda.current_stream().cuda_stream
    so = outs["state_out"].mid.data_ptr() if rec and "state_out" not in leave_out else None
    if rec and ring and window is not None:
        CA.check(fn(p._h, ctypes.byref(a), ns, rows, row0, T, recording, so, hs))
    elif rec and ring:
        CA.check(fn(p._h, ctypes.byref(a), ns, T, recording, so, hs))
    elif rec:
        CA.check(fn(p._h, ctypes.byref(a), int(window is not None), ns, rows or 0, row0, T, recording, so, hs))
    elif window is None:
        CA.check(fn(p._h, ctypes.byref(a), ns, T, hs))
    else:
        CA.check(fn(p._h, ctypes.byref(a), ns, rows, row0, T, hs))
    torch.cuda.synchronize()
    for key, t in before.items():
        if not (alias and key == "state_grad"):
            assert torch.equal(ins[key].view(torch.int32), t.view(torch.int32)), f"input {key} was written"
    assert ws.guards_kept(), "the workspace's surroundings were written"
    gone = {key for key in outs if key in leave_out or not n[key] or (alias and key == "state0_grad")}
    for key, g in outs.items():
        assert g.guards_kept(), f"the surroundings of {key} were written"
        if key in gone:
            assert g.untouched(), f"{key} was left out and written"
    got = {}
    for key, b in OUT.items():
        if b not in outs or b in gone:
            continue
        h = outs[b].mid.cpu().numpy()
        if window is not None and b in ("in_grad", "out"):
            before_rows = outs[b].before[PAD:PAD + outs[b].n].view(*h.shape).cpu().numpy()
            keep = np.ones(rows, bool)
            keep[row0:row0 + T] = False
            assert same(h[:, keep], before_rows[:, keep]), f"rows of {b} outside [{row0}, {row0 + T}) were written"
            got[key + "_buffer"] = h
            h = from_sm(h, T, row0)
        got[key] = h
    if alias and "state0_grad" not in leave_out:
        got["state"] = ins["state_grad"].cpu().numpy()
    if rec:
        if "state_out" not in leave_out:
            got["state_out"] = outs["state_out"].mid.cpu().numpy()
        Be = (p.ring_recording_block_rows if ring else p.recording_block_rows)(T, recording, c)
        nb = -(-T // Be)
        got["starts"] = ws.mid[:nb * p.n_state * ns].view(nb, p.n_state, ns).cpu().numpy()
    return got


# ---- calls through the Python front doors that more than one test file makes -----------------------------------------------------------
def accumulators(p, want, ap, ac, al=None):
    """the accum dict of a Python call: device copies of the accumulators the graph has and `want` names"""
    return {key: dev(v) for key, v, n in (("params", ap, p.n_param), ("consts", ac, p.n_const), ("loss", al, int(al is not None))) if n and key in want}


def to_numpy(r, window=None):
    """the dict a Python call returned, on the host; window = (row0, T) of a stream-major call: "x" and "out" become the window's rows,
    time-major, and "x_buffer" / "out_buffer" the whole buffers"""
    import torch
    torch.cuda.synchronize()
    res = {key: v.cpu().numpy() for key, v in r.items()}
    if window is not None:
        for key in ("x", "out"):
            if key in res:
                res[key + "_buffer"] = res[key]
                res[key] = from_sm(res[key], window[1], window[0])
    return res


def on_gpu(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=0, want=GRAD_KEYS):
    """run_block_grad of time-major numpy inputs"""
    return to_numpy(p.run_block_grad(dev(x), dev(yb), dev(s0) if p.n_state else None, dev(par), dev(sb) if p.n_state else None, want=want,
                                     accum=accumulators(p, want, ap, ac), checkpoint_rows=checkpoint_rows))


def on_gpu_sm(p, x, s0, par, yb, sb, ap, ac, checkpoint_rows=0, want=GRAD_KEYS, rows=None, row0=0, in_grad=None, pad=FILL):
    """run_block_grad_stream_major of time-major numpy inputs; "x" comes back time-major (the window's rows), "x_buffer" is the whole
    in_grad buffer.  Rows outside the window hold `pad` in x and dL/dy: they must not matter."""
    import torch
    T = x.shape[0]
    rows = up4(row0 + T) if rows is None else rows
    if in_grad is None and "x" in want:
        in_grad = torch.full((x.shape[1], rows, p.n_in), float(SENTINEL), device="cuda")
    r = p.run_block_grad_stream_major(dev(to_sm(x, rows, row0, pad)), dev(to_sm(yb, rows, row0, pad)), dev(s0) if p.n_state else None, dev(par),
                                      dev(sb) if p.n_state else None, want=want, accum=accumulators(p, want, ap, ac),
                                      checkpoint_rows=checkpoint_rows, row0=row0, n_samples=T, in_grad=in_grad if "x" in want else None)
    return to_numpy(r, (row0, T))


K = 0.37                                                          # grad_scale of the plain family's loss calls: no power of two, so e * k rounds


def on_gpu_loss(p, sm, x, s0, par, tg, sb, ap, ac, al, checkpoint_rows=0, want=LOSS_KEYS, rows=None, row0=0, in_grad=None, out=None):
    """run_block_loss_grad on time-major numpy inputs; sm: run_block_loss_grad_stream_major through stream-major buffers of `rows` rows with
    the block at row0, "x" and "out" come back time-major (the window's rows), "x_buffer" / "out_buffer" are the whole buffers, SENTINEL
    outside the window -- or in_grad / out, the buffers consecutive windows fill; "target_sent" / "target_after": the target buffer as it
    went in and as the launch left it"""
    import torch
    T, ns = x.shape[:2]
    accum = accumulators(p, want, ap, ac, al)
    args = (dev(s0) if p.n_state else None, dev(par), dev(sb) if p.n_state else None)
    if not sm:
        return to_numpy(p.run_block_loss_grad(dev(x), dev(tg), *args, grad_scale=K, want=want, accum=accum, checkpoint_rows=checkpoint_rows))
    rows = up4(row0 + T) if rows is None else rows
    full = lambda w: torch.full((ns, rows, w), float(SENTINEL), device="cuda")   # noqa: E731
    sent = to_sm(tg, rows, row0, FILL)
    tgd = dev(sent)
    r = p.run_block_loss_grad_stream_major(dev(to_sm(x, rows, row0, FILL)), tgd, *args, grad_scale=K, want=want,
                                           accum=accum, checkpoint_rows=checkpoint_rows, row0=row0, n_samples=T,
                                           in_grad=(full(p.n_in) if in_grad is None else in_grad) if "x" in want else None,
                                           out=(full(p.n_out) if out is None else out) if "out" in want else None)
    return dict(to_numpy(r, (row0, T)), target_sent=sent, target_after=tgd.cpu().numpy())


ROW0 = 8                                                          # where on_gpu_recording puts a stream-major window by default


def rows_of(T):
    """the buffer rows on_gpu_recording gives a stream-major window of T rows at ROW0: sentinel rows on both sides of it"""
    return up4(T + 9) + 4


def keys_of(loss, state_out=False):
    """the results a call returns: every gradient, "loss" and "out" of a loss call, "state_out" of a recording call or the restatement"""
    return tuple(k for k in LOSS_KEYS if loss or k not in ("loss", "out")) + (("state_out",) if state_out else ())


def on_gpu_recording(p, loss, sm, B, x, s0, par, tg, sb, ap, ac, al, row0=ROW0, rows=None):
    """one Python call on time-major numpy inputs.  B None: the one-launch call; else the recording call with block_rows = B, its workspace
    inside a larger sentinel-filled buffer.  sm: through stream-major buffers of `rows` rows (default rows_of(T)) with the window at
    row0 (default ROW0); "x" and "out" come back time-major, "x_buffer" / "out_buffer" are the whole buffers.  "inputs_kept": in, target /
    dL/dy and state as the call left them equal what went in; "starts": the head of the workspace; "ws_kept": nothing outside the queried
    workspace bytes was written"""
    import torch
    T, ns = x.shape[:2]
    want = keys_of(loss, B is not None)
    accum = accumulators(p, want, ap, ac, al if loss else None)
    rows = rows_of(T) if rows is None else rows
    xin, tin = (dev(to_sm(x, rows, row0, FILL)), dev(to_sm(tg, rows, row0, FILL))) if sm else (dev(x), dev(tg))
    sin = dev(s0) if p.n_state else None
    sent = [t.clone() for t in (xin, tin, sin) if t is not None]
    kw = dict(want=want, accum=accum)
    if sm:
        full = lambda w: torch.full((ns, rows, w), float(SENTINEL), device="cuda")   # noqa: E731
        kw.update(row0=row0, n_samples=T, in_grad=full(p.n_in))
        if loss:
            kw["out"] = full(p.n_out)
    if loss:
        kw["grad_scale"] = K
    ws = None
    if B is not None:
        n = p.recording_workspace_bytes(ns, T, B, stream_major=sm) // 4
        ws = Guarded((max(n, 4),))
        kw.update(block_rows=B, stream_major=sm, workspace=ws.mid)
        fn = p.run_recording_loss_grad if loss else p.run_recording_grad
    else:
        fn = {(False, False): p.run_block_grad, (False, True): p.run_block_grad_stream_major, (True, False): p.run_block_loss_grad,
              (True, True): p.run_block_loss_grad_stream_major}[(loss, sm)]
    res = to_numpy(fn(xin, tin, sin, dev(par), dev(sb) if p.n_state else None, **kw), (row0, T) if sm else None)
    # (bit for bit: the inputs of a cell with ties hold NaNs)
    res["inputs_kept"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sent, [t for t in (xin, tin, sin) if t is not None]))
    if ws is not None:
        nb = -(-T // p.recording_block_rows(T, B))                 # (B = 0: the library's choice)
        res["starts"] = ws.mid[:nb * p.n_state * ns].view(nb, p.n_state, ns).cpu().numpy()
        res["ws_kept"] = ws.guards_kept() and bool((ws.mid[n:] == SENTINEL).all())
    return res
