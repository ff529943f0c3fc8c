"""Every kernel of the adjoint family compiles to the machine code it had before the loss kernels were folded into their siblings and the
stream-major patch mover was stated once (tests/adjoint_code_pins.py; tests/golden/adjoint_code_pins.json); needs no GPU."""
import re

import pytest

import adjoint_code_pins as P
import far_grad_graphs as FG
import grad_graphs as GG
import ring_sm_graphs as RS
from grad_host_harness import code_pins

WANT = code_pins()


@pytest.fixture(scope="module")
def now():
    return P.pins()


def test_the_elf_reader_reads_sections(tmp_path):
    import struct
    names = b"\0.shstrtab\0.text\0.bss\0"
    body = b"\x90" * 5
    heads = [(0, 0, 0, 0), (1, 3, 64, len(names)), (11, 1, 64 + len(names), len(body)), (17, 8, 0, 99)]
    shoff = 64 + len(names) + len(body)
    elf = b"\x7fELF\x02\x01\x01" + b"\0" * 9 + struct.pack("<HHIQQQIHHHHHH", 3, 224, 1, 0, 0, shoff, 0, 64, 0, 0, 64, len(heads), 1)
    elf += names + body + b"".join(struct.pack("<IIQQQQIIQQ", n, k, 0, 0, off, size, 0, 0, 1, 0) for n, k, off, size in heads)
    assert P.elf_sections(elf) == {"": b"", ".shstrtab": names, ".text": body}
    with pytest.raises(AssertionError):
        P.elf_sections(b"\x7fELF\x01\x01" + elf[6:])


def test_the_pins_cover_every_graph_kernel_layout_and_stride():
    labels = [r[0] for r in P.requests()]
    assert sorted(labels) == sorted(WANT) and len(set(labels)) == len(labels)
    for name in GG.SUPPORTED:
        for kind in ("adjoint", "loss", "states"):
            assert {f"{kind}/tm/{name}", f"{kind}/sm/{name}"} <= set(WANT)
    for name in RS.GRAPHS:
        assert {f"ring_states/tm/{name}", f"ring_states/sm/{name}"} <= set(WANT)
        for c in RS.STRIDES:
            assert {f"{kind}/{layout}/c{c}/{name}" for kind in ("ring", "ring_loss") for layout in ("tm", "sm")} <= set(WANT)
    for name in FG.FARS:
        assert f"far_states/tm/{name}" in WANT
        for c in (0, 1, 32) if name in FG.STRIDES else (0,):
            assert {f"{kind}/{layout}/c{c}/{name}" for kind in ("far", "far_loss") for layout in ("tm", "sm")} <= set(WANT)
    for label, pin in WANT.items():
        assert set(pin) in ({"refused"}, {"symbol"} | set(P.SECTIONS)), label
        if "symbol" in pin:
            assert all(re.fullmatch(r"[0-9a-f]{64}", pin[s]) for s in P.SECTIONS) and P.variant_of(pin["symbol"])


def test_every_kernel_of_the_family_has_the_parents_code(now):
    """entry for entry, none skipped and none missing on either side: symbol, instructions, kernel descriptor and metadata (registers, LDS,
    kernarg layout) -- or the refusal's text"""
    assert sorted(now) == sorted(WANT)
    differ = [label for label in sorted(WANT) if now[label] != WANT[label]]
    assert not differ, differ


def test_the_loss_kernel_is_not_the_plain_kernel(now):
    """the compile-time switch selects code: a loss kernel shares no .text, no descriptor's metadata and no symbol with its sibling"""
    for label, pin in now.items():
        kind, rest = label.split("/", 1)
        if kind in ("loss", "ring_loss", "far_loss") and "symbol" in pin:
            plain = now[{"loss": "adjoint", "ring_loss": "ring", "far_loss": "far"}[kind] + "/" + rest]
            assert pin[".text"] != plain[".text"] and pin[".note"] != plain[".note"] and pin["symbol"] == plain["symbol"].replace("_kernel_", "_loss_kernel_", 1) \
                .replace("_sm_loss_kernel_", "_loss_sm_kernel_"), label
