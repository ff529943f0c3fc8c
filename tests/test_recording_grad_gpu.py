"""The backward of a whole recording on the MI355X (fz_run_recording_grad, fz_run_recording_loss_grad): every output bit for bit the
one-launch call's over the same rows and tests/recording_ref.py's, in both layouts; state_out and the block-start states the forward's;
non-zero accumulators; nothing written outside the window or the queried workspace; autograd.mse_recording.

Shapes: 1, 63, 65 and 257 streams (the masked tail, a wave boundary, a second workgroup); T = 37 in blocks of 8 and 12 (a partial last
block, chunk tails at C = 4 and C = 8, B no multiple of C), of 40 (a single block), T = 8 in one block of 8.

The stream-major window.  The issue asks for rows_total = T + 9 with row0 = 5.  fz_run_block_grad_stream_major -- the one-launch call
this is compared with, and the call every block launch is -- refuses that window for a graph with a wire count that is no multiple of
4: rows_total * n and row0 * n must be multiples of 4 floats (tests/test_recording_grad_host.py holds the recording call to the same
refusal, with that very window).  So the window here is the nearest one the ABI takes: row0 = 8 (5 rounded up to the grid) in
up4(T + 9) + 4 rows, sentinel rows on both sides of it."""
import numpy as np
import pytest

import adjoint_ref as A
import grad_fuzz_cells as GC
import loss_grad_ref as LR
import recording_ref as RR
import grad_harness as H
from grad_harness import F32, K, ROW0, dev, gpu_flowz, keys_of, make_inputs, outside_keeps_sentinel, rows_of, same, to_sm
from grad_harness import on_gpu_recording as launch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = RR.GPU_GRAPHS + RR.GPU_CELLS
MSE_TOL = 1e-6                                                    # the bound of test_loss_grad_gpu.test_mse_equals_run_then_torch_mse
SHAPES = RR.GPU_SHAPES


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


_progs = {}


def prog(F, name):
    if not _progs:
        _progs.update(RR.programs())
    return _progs[name]


def draw(p, name, ns, T, seed):
    """x, state, params, target (also dL/dy), dL/d(state after) and three accumulators, none of them zero"""
    kw = dict(draw_params=GC.draw_params, ties=GC.has_ties(p), special_every=GC.SPECIAL_EVERY) if name in GC.CELLS else {}
    x, s0, par, tg, sb, ap, ac = make_inputs(p, name, ns, T, seed, **kw)
    al = np.random.default_rng(seed + 1).standard_normal(ns).astype(F32)
    return x, s0, par, tg, sb, ap, ac, al


def check(p, got, want, what, keys):
    """every key of `keys` is there on both sides (a result that went missing fails, it does not pass unseen) and equal bit for bit"""
    H.check(p, got, want, what, keys, require=True)


def forward_state(p, x, s0, par, rows):
    """run_block's state after the first `rows` rows (the forward kernel's bits)"""
    if rows == 0 or not p.n_state:
        return s0
    _, s = p.run_block(dev(x[:rows]), dev(s0).clone(), dev(par))
    return s.cpu().numpy()[:p.n_state]


@pytest.mark.parametrize("loss", [False, True], ids=["grad", "loss_grad"])
@pytest.mark.parametrize("name", NAMES)
def test_a_recording_is_the_one_launch_call_bitwise_in_both_layouts(F, name, loss):
    p = prog(F, name)
    for i, (ns, T, B) in enumerate(SHAPES):
        d = draw(p, name, ns, T, 700 + i)
        x, s0, par, tg, sb, ap, ac, al = d
        what = f"{name} ns={ns} T={T} B={B} {'loss' if loss else 'plain'}"
        one = launch(p, loss, False, None, *d)
        ref = RR.grad(p, x, B, target=tg, k=K, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac, accum_loss=al) if loss else \
            RR.grad(p, x, B, out_grad=tg, state=s0, params=par, state_grad=sb, accum_params=ap, accum_consts=ac)
        nb = -(-T // min(B, T))
        fwd = [forward_state(p, x, s0, par, k * B) for k in range(nb)] + [forward_state(p, x, s0, par, T)]
        assert same(ref["state_out"], fwd[-1]) and all(same(ref["starts"][k], fwd[k]) for k in range(nb)), what + ": the restated states are not run_block's"
        got = {}
        for sm in (False, True):
            g = got[sm] = launch(p, loss, sm, B, *d)
            lay = what + (" stream-major" if sm else " time-major")
            check(p, g, one, lay + " against the one-launch call", keys_of(loss))
            check(p, g, ref, lay + " against the restatement", keys_of(loss, True))
            assert same(g["starts"], ref["starts"]), lay + ": the block-start states are not the forward's"
            assert same(g["state_out"][:p.n_state], fwd[-1]), lay + ": state_out is not run_block's"
            assert g["inputs_kept"], lay + ": in, target or state were written"
            assert g["ws_kept"], lay + ": the workspace was written beyond the queried size"
            if sm:
                assert outside_keeps_sentinel(g["x_buffer"], ROW0, T), lay + ": rows of in_grad outside the window were written"
                assert not loss or outside_keeps_sentinel(g["out_buffer"], ROW0, T), lay + ": rows of out outside the window were written"
        one_sm = launch(p, loss, True, None, *d)                  # (the stream-major one-launch call on the same window)
        check(p, got[True], one_sm, what + " stream-major against its one-launch call", keys_of(loss))
        check(p, got[True], got[False], what + ": the two layouts", keys_of(loss, True))


@pytest.mark.parametrize("sm", [False, True], ids=["time_major", "stream_major"])
def test_the_library_block_rule_and_other_strides_give_the_same_bits(F, sm):
    """block_rows = 0 (the library's choice), and a checkpoint stride of 8 under blocks of 12 rows"""
    name = "df1_cascade_params6"
    p = prog(F, name)
    d = draw(p, name, 130, 100, 31)
    one = launch(p, True, sm, None, *d)
    check(p, launch(p, True, sm, 0, *d), one, "block_rows = 0", keys_of(True))
    x, s0, par, tg, sb, ap, ac, al = d
    rows = rows_of(100)
    args = (dev(to_sm(x, rows, ROW0, 7.0)), dev(to_sm(tg, rows, ROW0, 7.0))) if sm else (dev(x), dev(tg))
    kw = dict(row0=ROW0, n_samples=100) if sm else {}
    r = p.run_recording_loss_grad(*args, dev(s0), dev(par), dev(sb), grad_scale=K, accum={"params": dev(ap), "consts": dev(ac), "loss": dev(al)},
                                  checkpoint_rows=8, block_rows=12, stream_major=sm, **kw)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in r.items()}
    if sm:
        got.update({k: np.ascontiguousarray(got[k][:, ROW0:ROW0 + 100].transpose(1, 0, 2)) for k in ("x", "out")})
    check(p, got, one, "C = 8, B = 12", keys_of(True))


# ---- autograd.mse_recording ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [False, True], ids=["time_major", "stream_major"])
def test_mse_recording_equals_run_then_torch_mse(F, sm):
    """value and gradients against AG.run, ((y - target) ** 2).mean(), backward(), within the bound test_loss_grad_gpu.py holds
    autograd.mse to against the same route; and bit for bit autograd.mse's own over the same rows"""
    from zignal_amd import autograd as AG
    name = "moog_ladder"
    p = prog(F, name)
    ns, T = 500, 40
    x, s0, par, tg, sb, ap, ac, al = draw(p, name, ns, T, 23)
    xin, tgd = (dev(to_sm(x, T)), dev(to_sm(tg, T))) if sm else (dev(x), dev(tg))

    def route(which):
        xt, st, pt = xin.clone().requires_grad_(), dev(s0).requires_grad_(), dev(par).requires_grad_()
        ct = torch.tensor(p.consts(), dtype=torch.float32).requires_grad_()
        s_out = None
        if which == "recording":
            loss, s_out = AG.mse_recording(p, xt, tgd, st, pt, ct, block_rows=12, stream_major=sm)
            assert not s_out.requires_grad
        elif which == "mse":
            loss = AG.mse(p, xt, tgd, st, pt, ct, stream_major=sm)
        else:
            y, s_out = AG.run(p, xt, st, pt, ct, stream_major=sm)
            loss = ((y - tgd) ** 2).mean()
        (loss * 3.0).backward()                                       # (an upstream scalar that is not 1)
        return (loss.item(), xt.grad.cpu().numpy(), st.grad.cpu().numpy(), pt.grad.cpu().numpy(), ct.grad.numpy()), s_out
    (got, s_got), (want, s_want), (fused, _) = route("recording"), route("torch"), route("mse")
    errs = [abs(got[0] - want[0]) / abs(want[0])] + [A.rel_err(g, w) for g, w in zip(got[1:], want[1:])]
    print("mse_recording vs run + torch: relative errors of value, x, state, params, consts:", errs)
    assert tuple(got[1].shape) == tuple(xin.shape)
    assert all(e <= MSE_TOL for e in errs), errs
    assert got[0] == fused[0] and all(same(g, w) for g, w in zip(got[1:], fused[1:]))
    assert same(s_got.cpu().numpy(), s_want.detach().cpu().numpy())


def test_two_calls_passing_state_out_on_equal_one_call_over_the_concatenation(F):
    from zignal_amd import autograd as AG
    name = "df1_cascade_params6"
    p = prog(F, name)
    ns, T = 257, 72
    x, s0, par, tg, sb, ap, ac, al = draw(p, name, ns, T, 29)
    _, whole = AG.mse_recording(p, dev(x), dev(tg), dev(s0), dev(par), block_rows=16)
    _, mid = AG.mse_recording(p, dev(x[:36]), dev(tg[:36]), dev(s0), dev(par), block_rows=8)
    _, end = AG.mse_recording(p, dev(x[36:]), dev(tg[36:]), mid, dev(par), block_rows=0)
    assert same(end.cpu().numpy(), whole.cpu().numpy())
    assert same(whole.cpu().numpy(), forward_state(p, x, s0, par, T))
    x2, t2 = dev(to_sm(x, T)[:, :, 0]), dev(to_sm(tg, T)[:, :, 0])            # [batch, time]
    pt = dev(par).requires_grad_()
    loss, s_sm = AG.mse_recording(p, x2, t2, dev(s0), pt, block_rows=12, stream_major=True)
    loss.backward()
    assert same(s_sm.cpu().numpy(), whole.cpu().numpy())
    assert same(pt.grad.cpu().numpy(), LR.loss_grad(p, x, tg, 2.0 / (T * ns), s0, par)["params"])
