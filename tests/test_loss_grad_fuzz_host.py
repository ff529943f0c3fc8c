"""The fuzz of the two loss-gradient kernels without a GPU (tests/loss_grad_fuzz.py, test_loss_grad_fuzz_gpu.py): both loss kernels of
every cell of tests/grad_fuzz_cells.py compile for gfx950 without scratch or VGPR spills, with the plain adjoint kernel's LDS, stride
and name; the cells reach what the named one-output graphs leave out; the GPU test's inputs tell a loss summed in another order from
the documented one; tests/loss_grad_ref.py agrees with float64 autograd of the mean squared error on multi-output cells and on a
sin / cos / log graph; and the recorded manifest holds exactly the loss kernels the GPU test launches."""
import gzip
import os

import numpy as np
import pytest

import adjoint_ref as A
import adjoint_ref_trig as AT
import grad_fuzz_cells as GC
import loss_grad_fuzz as LF
import loss_grad_ref as LR
import trig_cells as TC
from grad_harness import same
from grad_host_harness import ADJOINT, ADJOINT_LOSS, ADJOINT_SM, inputs as smooth_inputs
from zignal_amd import _capi as C
from zignal_amd import flowz as F

F32 = np.float32


# ---- the loss kernels for gfx950 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(LF.N_CHUNKS))
def test_both_loss_kernels_jit_compile_without_scratch_or_vgpr_spills(part, capsys):
    """what test_grad_fuzz_host.py asserts of the plain kernels -- scratch_bytes == 0, vgpr_spills == 0, unroll == C, the LDS bytes of the
    patch -- and that name, LDS bytes and stride are the plain kernel's.  No bound on vgprs + agprs: `vgprs` is .vgpr_count of the code
    object's notes, which on gfx950 counts the unified register file the kernel is allocated (architectural registers and, behind
    them, accumulation registers) and `agprs` is the accumulation registers among them, so the sum counts those twice -- 284 for
    cascade9_depth8's stream-major kernel, which spills nothing.  SGPR spills are printed, not asserted (correct, slower)."""
    lines = []
    for cell in GC.CELLS[part::LF.N_CHUNKS]:
        p = GC.prog(cell)
        c, r = GC.strides(p)
        for sm in (False, True):
            if sm and r is None:
                with pytest.raises(F.FlowzError) as ei:
                    p.loss_grad_resources(stream_major=True)
                assert ei.value.code == C.FZ_E_UNSUPPORTED and "does not fit the LDS" in str(ei.value)
                continue
            res, plain = p.loss_grad_resources(stream_major=sm), p.grad_resources(stream_major=sm)
            sym, psym = p.loss_grad_kernel_symbol(stream_major=sm), p.grad_kernel_symbol(stream_major=sm)
            assert sym != psym and sym == psym.replace("fz_adjoint_", "fz_adjoint_loss_", 1), (cell, sym, psym)
            assert res["scratch_bytes"] == 0 and res["vgpr_spills"] == 0 and res["unroll"] == c, (cell, sm, res)
            assert res["lds_bytes"] == plain["lds_bytes"] and res["unroll"] == plain["unroll"], (cell, sm, res, plain)
            assert res["agprs"] <= res["vgprs"] <= 512 and res["vgprs"] - res["agprs"] <= 256, (cell, sm, res)
            if sm:
                assert res["lds_bytes"] == 4 * 64 * (r * (p.n_in + p.n_out) + 4) * 4 <= 160 * 1024
            lines.append(f"  {cell:32} {'stream' if sm else 'time  '}-major C={c:<2} R={r!s:<4} vgprs {res['vgprs']:3} (plain {plain['vgprs']:3}) agprs {res['agprs']:3} "
                         f"sgpr_spills {res['sgpr_spills']:3} (plain {plain['sgpr_spills']:3})")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_cells_reach_what_the_one_output_graphs_leave_out():
    """one cell per feature (loss_grad_fuzz.REACHES), and the classes as a whole: n_out 1 .. 6, n_in 0 .. 3, every C, R = 8, 16 and 32"""
    import grad_graphs as GG
    named = [F.compile(F.from_sexpr(GG.SUPPORTED[n]())) for n in LR.GPU_GRAPHS]
    assert all(p.n_out == 1 for p in named)
    for what, (cell, has) in LF.REACHES.items():
        p = GC.prog(cell)
        assert has(p, *GC.strides(p)), (what, cell)
        assert not any(has(q, *GC.strides(q)) for q in named), what
    progs = [GC.prog(c) for c in GC.CELLS]
    assert {p.n_out for p in progs} == set(range(1, 7)) and {p.n_in for p in progs} == set(range(4))
    assert {GC.strides(p)[0] for p in progs} == {1, 2, 4, 8, 16} and {GC.strides(p)[1] for p in progs} == {8, 16, 32}
    assert all({"sin", "cos", "log"} & GC.kinds(TC.graph(n)) for n in TC.GRAD_GRAPHS)
    for cell in (LF.SUBSET_CELL, LF.EDGE_CELLS[0]) + LF.AUTOGRAD_CELLS:
        assert GC.prog(cell).n_out >= 2 and GC.prog(cell).n_out != GC.prog(cell).n_in, cell
    assert not any(GC.has_ties(GC.prog(c)) for c in LF.AUTOGRAD_CELLS)


# ---- the inputs of the GPU test tell the documented order from the others --------------------------------------------------------------
@pytest.mark.parametrize("part", range(LF.N_CHUNKS))
def test_the_gpu_tests_inputs_tell_a_loss_summed_in_another_order(part, capsys):
    """with the inputs test_loss_grad_fuzz_gpu.py draws for a cell's longest block at 65 streams, the loss with the rows ascending, with
    the slots descending (two outputs and more) or with e * e added unrounded differs in bits from the documented one in at least one
    stream whose loss is finite: a kernel that sums in one of these orders cannot pass"""
    lines = []
    for cell in GC.CELLS[part::LF.N_CHUNKS]:
        p = GC.prog(cell)
        i, T = LF.longest_65(cell)
        x, s0, par, tg, sb, ap, ac, al = LF.draw(cell, 65, T, GC.GPU_SEED + i)
        y, _ = A.forward(p, x, s0, par)
        ls = LF.losses(y, tg, al)
        assert same(ls["documented"], LR.loss_grad(p, x, tg, LF.K, s0, par, sb, ap, ac, al)["loss"])
        finite = np.isfinite(ls["documented"])
        n = {k: int(((v.view(np.uint32) != ls["documented"].view(np.uint32)) & finite).sum()) for k, v in ls.items() if k != "documented"}
        lines.append(f"  {cell:32} T={T:3} finite streams {int(finite.sum()):2}, streams that differ: {n}")
        for k, v in n.items():
            assert v >= 1 or (k == "slots descending" and p.n_out < 2), (cell, k)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_edge_targets_are_what_they_are_for():
    """loss_grad_fuzz.edge_case on the cells and shape of the GPU test: every kind in a stream of its own, and the restated e * e is +0
    where the target is y, infinite where it must overflow (with a finite dL/dy), and denormal in the multi-output cell's scaled streams"""
    for cell in LF.EDGE_CELLS:
        p = GC.prog(cell)
        T = GC.strides(p)[1] + 3
        (x, s0, par, tg, sb, ap, ac, al), kinds = LF.edge_case(cell, 65, T, 900)
        assert set(LF.EDGE_KINDS) <= set(kinds) and kinds.count(None) >= 30
        y, _ = A.forward(p, x, s0, par)
        with np.errstate(all="ignore"):
            e = y - tg
            sq, yb = e * e, e * F32(LF.K)
        first = {k: kinds.index(k) for k in LF.EDGE_KINDS}            # (the streams the value fills)
        assert np.all(e[:, first["y"]].view(np.uint32) == 0) and same(tg[:, first["y"]], y[:, first["y"]])
        assert np.all(np.isnan(sq[:, first["nan"]])) and np.all(np.isinf(sq[:, first["+inf"]])) and np.all(np.isinf(sq[:, first["-inf"]]))
        assert np.all(np.isinf(sq[:, first["overflow"]])) and np.all(np.isfinite(yb[:, first["overflow"]]))
        z = tg[:, first["zeros"]]
        assert np.all(z == 0) and np.any(np.signbit(z)) and not np.all(np.signbit(z))
        den = sq[:, first["denormal"]]
        if cell == LF.EDGE_CELLS[0]:
            assert ((den > 0) & (den < np.finfo(F32).tiny)).sum() >= den.size // 2, cell
        else:
            assert np.all(den > 0) and np.all(den < F32(1e-12))


# ---- the restatement against float64 autograd of the mean squared error -------------------------------------------------------------
@pytest.mark.parametrize("name", LF.AUTOGRAD_CELLS + ("all3",))
def test_restatement_matches_float64_autograd_of_the_mse(name):
    """test_loss_grad_host.test_restatement_matches_float64_autograd_of_the_mse on graphs with more than one output wire and on one with
    sin, cos and log (restated by tests/adjoint_ref_trig.py); the bound is that test's, 1e-4"""
    import torch

    trig = name not in GC.CELLS
    p, ref = (TC.graph(name), AT) if trig else (GC.prog(name), A)
    assert trig or p.n_out >= 2
    ns, T = 8, 32
    x, s0, _, _, _ = smooth_inputs(p, ns, T, 11)
    par = GC.draw_params(p, ns, np.random.default_rng(7))
    target = (np.random.default_rng(5).standard_normal((T, ns, p.n_out)) * 0.5).astype(F32)
    n = T * ns * p.n_out
    got = LR.loss_grad(p, x, target, 2.0 / n, s0, par, None, ref=ref)
    L = A.Layout(p)
    t = lambda a, shape: torch.tensor(np.asarray(a, np.float64).reshape(shape), dtype=torch.float64, requires_grad=True)   # noqa: E731
    xt, st = t(x, x.shape), t(s0, (L.n_state, ns))
    pt = t(par if par is not None else np.zeros((L.n_param, ns)), (L.n_param, ns))
    ct = t(np.repeat(L.consts.astype(np.float64)[:, None], ns, 1), (L.n_const, ns))
    y, _ = ref.torch_forward(L, xt, st, pt, ct)
    mse = ((y - torch.tensor(target, dtype=torch.float64)) ** 2).mean()
    grads = torch.autograd.grad(mse, (xt, st, pt, ct), allow_unused=True)
    bound = 1e-4
    mean = float(got["loss"].astype(np.float64).sum() / n)
    assert abs(mean - mse.item()) <= bound * mse.item(), (mean, mse.item())
    assert A.rel_err(got["out"], y.detach().numpy()) <= bound
    seen = 0
    for k, g in zip(("x", "state", "params", "consts"), grads):
        if g is None or g.numel() == 0:
            continue
        e = A.rel_err(got[k], g.numpy())
        print(f"{name}: {k} relative error {e:.2e}")
        assert e <= bound, (k, e)
        seen += 1
    assert seen >= 3


def test_the_restatement_of_a_graph_without_trig_does_not_depend_on_the_module():
    """loss_grad(ref=adjoint_ref_trig) gives loss_grad()'s bits where no sin, cos or log is: the argument changes no existing caller's"""
    for cell in ("make11", "cmp21", "generator_without_input"):
        p = GC.prog(cell)
        d = LF.draw(cell, 65, 11, 3)
        x, s0, par, tg, sb, ap, ac, al = d
        a, b = LR.loss_grad(p, x, tg, LF.K, s0, par, sb, ap, ac, al), LR.loss_grad(p, x, tg, LF.K, s0, par, sb, ap, ac, al, ref=AT)
        assert all(same(a[k], b[k]) for k in a), cell


# ---- the manifest ---------------------------------------------------------------------------------------------------------------
def test_the_recorded_manifest_holds_the_loss_kernels_of_the_gpu_test(tmp_path):
    """tests/golden/loss_grad_fuzz_kernels.fzm.gz: every record a loss variant, none refused, and record for record what a process that
    resolves loss_grad_fuzz.kernel_requests() writes now"""
    raw = gzip.open(LF.MANIFEST, "rb").read()
    have = LF.records(raw)
    flags = [r[3] for r in have]
    assert flags and all(f & ADJOINT and f & ADJOINT_LOSS and not f & ~(ADJOINT | ADJOINT_SM | ADJOINT_LOSS) for f in flags)
    n_req = len(LF.kernel_requests())
    assert n_req == 2 * len(GC.CELLS) + 4 * len(GC.STRIDE_CELLS) + 2 * len(LF.TRIG_STRIDES) * len(TC.GRAD_GRAPHS)
    assert sum(1 for f in flags if f & ADJOINT_SM) * 2 == len(flags) <= n_req
    r = F.manifest_build(LF.MANIFEST)
    assert r["failed"] == 0 and r["at_hand"] + r["built"] == r["records"] == len(have), r
    assert LF.records(LF.record(str(tmp_path / "now.fzm"))) == have
