"""tests/grad_host_harness.py is what the host tests of the backward family lean on: its fake call, invalid() and the no-contraction
rule, held to their word; needs no GPU."""
import ctypes

import pytest

import grad_graphs as GG
import grad_harness as H
import grad_host_harness as HH
import ring_loss_graphs as RL
from grad_host_harness import FakeCall, assert_no_contraction, empty_args, invalid
from zignal_amd import _capi as C
from zignal_amd import flowz as F

PLAIN = ["s_load_dwordx2", "v_mul_f32_e32", "global_load_dword", "v_add_f32_e32", "v_mul_f32_e32", "global_store_dword", "s_endpgm"]
DIVISION = ["v_div_scale_f32", "v_div_scale_f32", "v_rcp_f32_e32", "v_fma_f32", "v_fmac_f32_e32", "v_fma_f32", "v_fma_f32", "v_fma_f32",
            "v_div_fmas_f32", "v_div_fixup_f32"]                  # the five fused steps of the correctly rounded division
ROOT_ = ["v_sqrt_f32_e32", "v_fma_f32", "v_fma_f32"]              # the two of the square root
LDS = ["ds_write_b32", "ds_read_b32"]


def test_the_harness_imports_without_torch_at_module_level():
    assert "torch" not in vars(HH)


@pytest.mark.parametrize("corner", sorted(H.ENTRY), ids=lambda c: "".join("RLWB"[i] if on else "-" for i, on in enumerate(c)))
def test_the_fake_calls_buffers_are_the_corners_distinct_aligned_and_apart(corner):
    ring, loss, window, rec = corner
    p = RL.prog("lds_ring_comb") if ring else F.compile(F.from_sexpr(GG.SUPPORTED["moog_ladder"]()))
    b = FakeCall(p, 100, 13, ring, loss, (24, 4) if window else None, 4 if rec else None)
    assert b.fn is getattr(C.lib, H.ENTRY[corner]) and b.ws > 0
    want = {"in_", "state", "params", "target" if loss else "out_grad", "state_grad", "in_grad", "state0_grad", "param_grad", "const_grad", "workspace"}
    want |= ({"loss", "out"} if loss else set()) | ({"state_out"} if rec else set())
    assert set(b.addr) == set(b.size) == want
    assert b.size["in_"] == b.size["in_grad"] == (24 if window else 13) * 100 * 4 * p.n_in and b.size["workspace"] == b.ws
    spans = sorted((b.addr[k], b.addr[k] + b.size[k]) for k in b.addr)
    assert all(lo % 16 == 0 for lo, _ in spans) and len({lo for lo, _ in spans}) == len(spans)
    assert all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:]))
    a = b.args(checkpoint_rows=4)
    assert a.struct_size == ctypes.sizeof(a) == ctypes.sizeof(C.LossGradArgs if loss else C.GradArgs)
    assert a.workspace_bytes == b.ws and a.checkpoint_rows == 4
    for k, n in b.size.items():
        if k != "state_out":
            assert getattr(a, k) == (b.addr[k] if n else None), k
    if ring:                                                      # (the comb has no per-stream coefficient: both buffers are null)
        assert p.n_param == 0 and a.params is None and a.param_grad is None
    if C.lib.fz_device_count() == 0:                              # the corner's call shape: it passes every check
        assert b.run(b.args()) == C.FZ_E_NO_DEVICE, C.last_error()


def test_invalid_wants_the_code_and_the_word():
    p = F.compile(F.from_sexpr(GG.SUPPORTED["moog_ladder"]()))
    b = FakeCall(p, 100, 13)
    rc = b.run(b.args(checkpoint_rows=3))
    assert invalid(rc, "checkpoint_rows") and not invalid(rc, "struct_size")
    assert not invalid(C.FZ_OK, "checkpoint_rows") and not invalid(C.FZ_E_UNSUPPORTED, "checkpoint_rows")      # (the word is still there)
    assert b.run(empty_args(), ns=0) == C.FZ_OK and not invalid(C.FZ_OK, "")


def test_the_no_contraction_rule_passes_what_it_allows():
    assert_no_contraction(PLAIN, divides=False)
    assert_no_contraction(PLAIN + DIVISION)
    assert_no_contraction(PLAIN + DIVISION + ROOT_ + DIVISION)
    assert_no_contraction(PLAIN + LDS, divides=False, lds=True)
    assert_no_contraction(PLAIN + LDS + DIVISION, lds=True)


@pytest.mark.parametrize("every,kw", [
    (PLAIN + ["v_fma_f32"], {}),                                  # one stray fused multiply-add
    (PLAIN + ["v_fmac_f32_e32"], {}),                             # ... without a division
    (PLAIN + DIVISION + ["v_fma_f32"], {}),                       # ... next to one
    (PLAIN + DIVISION + ["v_pk_fma_f32"], {}),
    (PLAIN + ["v_mad_f32"], {}),
    (PLAIN + DIVISION[:-2] + ["v_div_fixup_f32"], {}),            # a division without its v_div_fmas
    (PLAIN + DIVISION, {"divides": False}),
    (PLAIN + ROOT_, {"divides": False}),
    (PLAIN + LDS + ["s_barrier"], {"lds": True}),
    (PLAIN + LDS + ["global_atomic_add_f32"], {"lds": True}),
    (PLAIN + LDS + ["ds_add_rtn_f32", "buffer_atomic_add_f32"], {"lds": True}),
    (PLAIN, {"lds": True}),                                       # no ds_ op at all
    (PLAIN + LDS[:1], {"lds": True}),                             # written, never read
], ids=lambda v: None if isinstance(v, dict) else v[-1])
def test_the_no_contraction_rule_fails_what_it_forbids(every, kw):
    with pytest.raises(AssertionError):
        assert_no_contraction(every, **kw)


def test_symbol_shape_reads_both_layouts():
    assert HH.symbol_shape("fz_adjoint_kernel_c16b256_g0123abcd", "c") == (16, 256)
    assert HH.symbol_shape("fz_adjoint_ring_loss_sm_kernel_c4r32b128_g0123abcd", "c") == (4, 32, 128)
    assert HH.symbol_shape("fz_states_ring_kernel_u8b64_g0123abcd", "u") == (8, 64)
    with pytest.raises(AssertionError):
        HH.symbol_shape("fz_states_ring_kernel_u8b64_g0123abcd", "c")


def test_a_written_manifest_is_what_the_parser_reads(tmp_path):
    import gzip
    recipe = HH.recipe_of(GG.SUPPORTED["integrator"]())
    assert recipe.startswith(b"typed 0\n") and HH.recipe_of(GG.SUPPORTED["integrator"](), 1).startswith(b"typed 1\n")
    records = [(1, 16, 256, HH.ADJOINT, recipe), (32, 8, 64, HH.ADJOINT | HH.ADJOINT_SM | HH.STATES, recipe)]
    HH.write_manifest(tmp_path / "m.fzm", records)
    raw = open(tmp_path / "m.fzm", "rb").read()
    assert raw.startswith(b"FZM1 1 16 256 %d %d\n" % (HH.ADJOINT, len(recipe)) + recipe + b"FZM1 32 8 64 ")
    with gzip.open(tmp_path / "m.fzm.gz", "wb") as f:
        f.write(raw)
    assert RL.manifest_variants(tmp_path / "m.fzm.gz") == records
