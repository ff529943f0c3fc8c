"""The backward of a whole recording on the MI355X over every graph of tests/recording_fuzz.py -- the 48 cells of
tests/grad_fuzz_cells.py, the sin / cos / log graphs, six graphs with wide input frames: every class of the two block-start-states
kernels -- at the shapes its rule builds from the graph's own strides (T = 1, T < U, around U, R and 2 R_adj, blocks of 4 rows, blocks
that are no multiple of the checkpoint stride, one block; 1, 64, 65 and 321 streams).

Per triple and layout, all bit for bit, a NaN of any payload equal to a NaN: every result of the recording call against the
one-launch call of the same layout, against tests/recording_ref.py, and the two layouts against each other; the block-start states
and state_out against the restatement, state_out once per graph against run_block's (the forward planner's own kernel); the inputs
untouched, sentinels behind the queried workspace and in every row outside the stream-major window, accumulators that are not zero.
wide4x4 and wide8x2 also run stream-major in blocks of 5 and 6 rows, whose windows lie off the 4-row grid.  The 40-wire graph runs
time-major only (test_recording_fuzz_host.py pins the refusal)."""
import numpy as np
import pytest

import recording_fuzz as RF
import grad_harness as H
from grad_harness import ROW0, dev, gpu_flowz, keys_of, outside_keeps_sentinel, same
from grad_harness import on_gpu_recording as launch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    return gpu_flowz()


def check(p, got, want, what, keys):
    H.check(p, got, want, what, keys, require=True)


def run_blocks_state(p, x, s0, par):
    """run_block's state after all rows of x"""
    _, s = p.run_block(dev(x), dev(s0).clone(), dev(par))
    torch.cuda.synchronize()
    return s.cpu().numpy()[:p.n_state]


def hold(p, name, loss, d, B, sms, what, row0=None, rows=None, forward=False):
    """one draw through the recording call in the layouts `sms`, held to everything the module's docstring lists.  row0 / rows: the
    stream-major window and buffer rows (default: grad_harness.on_gpu_recording's)"""
    x, s0, par, tg, sb, ap, ac, al = d
    T = x.shape[0]
    assert all(np.all(a != 0) for a in (sb, ap, ac, al) if a.size), what + ": an accumulator is zero"
    win = {} if row0 is None else dict(row0=row0, rows=rows)
    ref = RF.restated(name, d, B, loss)
    one = launch(p, loss, False, None, *d)
    fwd = run_blocks_state(p, x, s0, par) if forward and p.n_state else None
    check(p, one, ref, what + " the time-major one-launch call against the restatement", keys_of(loss))
    got = {}
    for sm in sms:
        g = got[sm] = launch(p, loss, sm, B, *d, **(win if sm else {}))
        lay = what + (" stream-major" if sm else " time-major")
        check(p, g, launch(p, loss, True, None, *d, **win) if sm else one, lay + " against its one-launch call", keys_of(loss))
        check(p, g, one, lay + " against the time-major one-launch call", keys_of(loss))
        check(p, g, ref, lay + " against the restatement", keys_of(loss, True))
        assert same(g["starts"], ref["starts"]), lay + ": the block-start states are not the forward's"
        if fwd is not None:
            assert same(g["state_out"][:p.n_state], fwd), lay + ": state_out is not run_block's"
        assert g["inputs_kept"], lay + ": in, target or state were written"
        assert g["ws_kept"], lay + ": the workspace was written beyond the queried size"
        if sm:
            r0 = ROW0 if row0 is None else row0
            assert outside_keeps_sentinel(g["x_buffer"], r0, T), lay + ": rows of in_grad outside the window were written"
            assert not loss or outside_keeps_sentinel(g["out_buffer"], r0, T), lay + ": rows of out outside the window were written"
    if len(got) == 2:
        check(p, got[True], got[False], what + ": the two layouts", keys_of(loss, True))
        assert same(got[True]["starts"], got[False]["starts"]), what + ": the block-start states of the two layouts"


@pytest.mark.parametrize("loss", [False, True], ids=["grad", "loss_grad"])
@pytest.mark.parametrize("name", RF.NAMES)
def test_a_recording_is_the_one_launch_call_bitwise_on_every_graph(F, name, loss):
    p = RF.prog(name)
    s = RF.strides(name)
    sh = RF.shapes(name)
    tag = f"{name} ({p.n_in} in, U={s['u_tm']}/{s['u_sm']}, R={s['r']}, C={s['c']}, R_adj={s['r_adj']}) {'loss' if loss else 'plain'}"
    for i, (ns, T, B) in enumerate(sh):
        hold(p, name, loss, RF.draw(name, ns, T, RF.BASE + i), B, RF.layouts(name), f"{tag} ns={ns} T={T} B={B}", forward=i == RF.longest(name)[0])
    if name in RF.SM_ONLY:
        ns, T, B, row0 = RF.SM_ONLY[name]
        hold(p, name, loss, RF.draw(name, ns, T, RF.BASE + len(sh)), B, (True,), f"{tag} ns={ns} T={T} B={B} row0={row0}", row0=row0,
             rows=RF.up4(row0 + T + 9) + 4)
