"""The machine code of every kernel of the adjoint family, pinned (tests/golden/adjoint_code_pins.json): per kernel the sha256 of the code
object's .text (the instructions), .rodata (the kernel descriptor) and .note (the metadata: registers, LDS, kernarg layout).  Not the
whole file: its string table carries names -- of argument structs, of functions -- that say nothing about what runs.  The pins depend
on the compiler, like the code ids of tests/golden/graph_pins.json.

The kernels: for every graph of grad_graphs.SUPPORTED the adjoint, loss and states kernel in both layouts at the default stride; for every
ring graph (ring_sm_graphs.GRAPHS, which holds those of ring_grad_graphs, ring_loss_graphs and ring_recording_graphs) at every stride of
ring_sm_graphs.STRIDES the ring and ring loss kernel in both layouts -- where the geometry rule refuses, the pin is the refusal's text --
and the ring states kernel in both layouts; for every far graph (far_grad_graphs.FARS) the far and far loss kernel in both layouts at
the default stride, for those of far_grad_graphs.STRIDES at C = 1 and C = 32 as well -- the strides the GPU tests launch; a refusal is
pinned as for the ring entries -- and the time-major far states kernel.

The committed file was written by pins() from the parent commit of the change that folded the loss kernels into their siblings, in a
checkout of its own:
    PYTHONPATH=<parent checkout>:tests python tests/adjoint_code_pins.py > tests/golden/adjoint_code_pins.json
The ring_states/sm/* entries are younger than that kernel: they were written the same way from the parent commit of the change that
folded the four block-start-states texts into one per layout (the commit that added the stream-major ring states kernel), with the
requests() of this file; the 214 entries the file held before came out of that tree byte for byte as they stood.
The far/*, far_loss/* and far_states/* entries are younger still: they were written the same way from the parent commit of the change
that folded the three far texts into their ring siblings (FZ_FAR next to FZ_RING), before any text was merged, with the requests() of
this file; the 224 entries the file held before came out of that tree byte for byte as they stood, so the file only gained lines."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

from grad_host_harness import ADJOINT, ADJOINT_FAR, ADJOINT_LOSS, ADJOINT_RING, ADJOINT_SM, STATES

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "adjoint_code_pins.json")
SECTIONS = (".text", ".rodata", ".note")
SYMBOL = re.compile(r"fz_(adjoint|states)(_ring|_far)?(_loss)?(_sm)?_kernel_[cu](\d+)(?:r(\d+))?b(\d+)_g[0-9a-f]{8}")


def elf_sections(data):
    """{name: contents} of the sections of an ELF64 little-endian file"""
    assert data[:6] == b"\x7fELF\x02\x01", "not an ELF64 little-endian file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    heads = [struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = data[heads[shstrndx][4]:heads[shstrndx][4] + heads[shstrndx][5]]
    out = {}
    for name, kind, _, _, offset, size in heads:
        if kind != 8:                                             # (SHT_NOBITS holds no bytes)
            out[names[name:names.index(b"\0", name)].decode()] = data[offset:offset + size]
    return out


def variant_of(symbol):
    """(P, U, block, flags) of the Variant a kernel symbol of the family names"""
    m = SYMBOL.fullmatch(symbol)
    assert m, symbol
    rings = {None: 0, "_ring": ADJOINT_RING, "_far": ADJOINT_RING | ADJOINT_FAR}[m.group(2)]
    flags = ADJOINT | (STATES if m.group(1) == "states" else 0) | rings | (ADJOINT_LOSS if m.group(3) else 0) | (ADJOINT_SM if m.group(4) else 0)
    return int(m.group(6) or 1), int(m.group(5)), int(m.group(7)), flags


def requests():
    """(label, s-expression of the graph, name of the Program method that answers the symbol, its arguments)"""
    import far_grad_graphs as FG
    import grad_graphs as GG
    import ring_grad_graphs as RG
    import ring_loss_graphs as RL
    import ring_recording_graphs as RR
    import ring_sm_graphs as RS
    assert set(RG.RINGS) | set(RL.GRAPHS) | set(RR.GRAPHS) <= set(RS.GRAPHS)
    out = []
    for name in sorted(GG.SUPPORTED):
        for sm in (False, True):
            layout = "sm" if sm else "tm"
            out.append((f"adjoint/{layout}/{name}", GG.SUPPORTED[name](), "grad_kernel_symbol", (0, sm)))
            out.append((f"loss/{layout}/{name}", GG.SUPPORTED[name](), "loss_grad_kernel_symbol", (0, sm)))
            out.append((f"states/{layout}/{name}", GG.SUPPORTED[name](), "states_kernel_symbol", (sm,)))
    for name in sorted(RS.GRAPHS):
        out.append((f"ring_states/tm/{name}", RS.GRAPHS[name](), "ring_states_kernel_symbol", ()))
        out.append((f"ring_states/sm/{name}", RS.GRAPHS[name](), "ring_states_kernel_symbol", (True,)))
        for c in RS.STRIDES:
            for sm in (False, True):
                layout = "sm" if sm else "tm"
                out.append((f"ring/{layout}/c{c}/{name}", RS.GRAPHS[name](), "ring_grad_kernel_symbol", (c, sm)))
                out.append((f"ring_loss/{layout}/c{c}/{name}", RS.GRAPHS[name](), "ring_loss_grad_kernel_symbol", (c, sm)))
    for name in sorted(FG.FARS):
        out.append((f"far_states/tm/{name}", FG.FARS[name](), "far_states_kernel_symbol", ()))
        for c in (0, 1, 32) if name in FG.STRIDES else (0,):
            for sm in (False, True):
                layout = "sm" if sm else "tm"
                out.append((f"far/{layout}/c{c}/{name}", FG.FARS[name](), "far_grad_kernel_symbol", (c, sm)))
                out.append((f"far_loss/{layout}/c{c}/{name}", FG.FARS[name](), "far_loss_grad_kernel_symbol", (c, sm)))
    return out


def _child(cache):
    """in a process of its own, FLOWZ_HIP_CACHE a fresh directory: name every kernel, build them all through a manifest, hash the objects"""
    import ctypes
    from zignal_amd import _capi as C
    from zignal_amd import flowz as F
    pins, records = {}, []
    for label, sexpr, method, args in requests():
        expr = F.from_sexpr(sexpr)
        try:
            symbol = getattr(F.compile(expr), method)(*args)
        except F.FlowzError as er:
            pins[label] = {"refused": str(er)}
            continue
        pins[label] = {"symbol": symbol}
        buf = ctypes.create_string_buffer(1 << 16)
        n = C.lib.fz_expr_recipe(expr._h, buf, 1 << 16)
        assert 0 < n < 1 << 16
        recipe = b"typed 0\n" + buf.raw[:n]
        records.append(b"FZM1 %d %d %d %d %d\n" % (variant_of(symbol) + (len(recipe),)) + recipe)
    manifest = os.path.join(cache, "kernels.fzm")
    with open(manifest, "wb") as f:
        f.write(b"".join(records))
    counts = F.manifest_build(manifest, min(16, len(os.sched_getaffinity(0))))
    assert counts["failed"] == 0, counts
    built = {}
    for name in os.listdir(cache):
        if name.endswith(".hsaco"):
            sec = elf_sections(open(os.path.join(cache, name), "rb").read())
            symbol, = set(re.findall(rb"fz_\w+_g[0-9a-f]{8}", sec[".strtab"]))
            built[symbol.decode()] = {s: hashlib.sha256(sec[s]).hexdigest() for s in SECTIONS}
    assert set(built) == {p["symbol"] for p in pins.values() if "symbol" in p}
    for p in pins.values():
        if "symbol" in p:
            p.update(built[p["symbol"]])
    return pins


def pins():
    """{label: {"symbol", ".text", ".rodata", ".note"} or {"refused": the refusal's text}} with the library that is imported; needs no GPU"""
    import zignal_amd
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport json, adjoint_code_pins as P\nprint(json.dumps(P._child(%%r)))\n" % (os.path.dirname(os.path.dirname(zignal_amd.__file__)), HERE)
    env = {k: v for k, v in os.environ.items() if k != "FLOWZ_HIP_MANIFEST"}
    with tempfile.TemporaryDirectory() as cache:
        out = subprocess.check_output([sys.executable, "-c", code % cache], env=dict(env, FLOWZ_HIP_CACHE=cache), text=True)
    return json.loads(out.strip().splitlines()[-1])


if __name__ == "__main__":
    print(json.dumps(pins(), indent=1, sort_keys=True))
