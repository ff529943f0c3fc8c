#!/usr/bin/env python3
"""Dev tool: JIT a graph variant (no GPU needed) and print instruction histogram + resources.

usage: tools/isa_stats.py [graph] [P] [U] [block] [flags]   (graph: cascade6|par4|par4f|osc|df1|ring)
       tools/isa_stats.py lossgrad [graph] [tm|sm]         the kernel of fz_run_block_loss_grad (sm: _stream_major) next to the plain
                                                           adjoint kernel: registers, spills, LDS (graph: also cascade_params6)
       tools/isa_stats.py states [graph] [tm|sm]           the block-start-states kernel of fz_run_recording_grad: registers, spills, LDS
       tools/isa_stats.py ringgrad [graph] [--layout stream-major]
                                                           the kernel of fz_run_block_ring_grad: registers, spills, scratch, LDS bytes, and
                                                           its LDS (ds_*) and vector-memory instructions per row (graph: ldsring, comb256,
                                                           or a name of tests/ring_grad_graphs.py); --layout stream-major: the kernel of
                                                           fz_run_block_ring_grad_stream_major, with its patch rows R and lanes
       tools/isa_stats.py ringlossgrad [graph] [--layout stream-major]
                                                           the same line for the kernel of fz_run_block_ring_loss_grad, next to the plain
                                                           ring kernel's figures (graph: also a name of tests/ring_loss_graphs.py)
       tools/isa_stats.py fargrad [graph] [--layout stream-major]
                                                           the same lines for the kernel of fz_run_block_far_grad (delay lines deeper than
                                                           256 samples, rings in HBM), with the path its static rule picks (graph: a name
                                                           of tests/far_grad_graphs.py, comb2000, or any ringgrad graph); --layout
                                                           stream-major: the kernel of fz_run_block_far_grad_stream_major
       tools/isa_stats.py farlossgrad [graph] [--layout stream-major]
                                                           the same for the kernel of fz_run_block_far_loss_grad, next to the plain far kernel
       tools/isa_stats.py ringstates [graph] [--layout stream-major]
                                                           the block-start-states kernel of fz_run_recording_ring_grad next to the ring
                                                           adjoint kernel: registers, spills, scratch, LDS bytes, and the ds_* and
                                                           vector-memory instructions in the kernel (graph: as for ringlossgrad, or `all`:
                                                           the ten of tests/ring_loss_graphs.py); --layout stream-major: the kernel of
                                                           fz_run_recording_ring_grad_stream_major, with its patch rows R and lanes
       tools/isa_stats.py farstates [graph] [--layout stream-major]
                                                           the same lines for the block-start-states kernel of fz_run_recording_far_grad next
                                                           to the far adjoint kernel, with its prefetch table (graph: as for fargrad, or
                                                           `all`: the eight of tests/far_grad_graphs.py); --layout stream-major: the kernel
                                                           of fz_run_recording_far_grad_for with FZ_GRAD_STREAM_MAJOR, with its patch rows R
                                                           and lanes
"""
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graphs as G  # noqa: E402
from zignal_amd import flowz as F  # noqa: E402

GRAPHS = {"cascade6": lambda: G.df1_cascade(6), "par4": G.par4_sum, "par4f": G.par4_sum_fanout,
          "osc": lambda: G.osc_chain(6), "gain": lambda: G.mul(G.lit(0.5), G.IN(1)), "cascade2": lambda: G.df1_cascade(2), "cascade4": lambda: G.df1_cascade(4), "df1": G.df1, "integrator": G.integrator,
          "mod6": lambda: G.df1_cascade_modulated(6), "ldsring": G.lds_ring_comb,
          "ring": lambda: G.seq(G.add(G.IN(1), G.mul(G.lit(0.5), G.DEL(1, 40))), G.fb(G.add(G.mul(G.lit(0.7), G.DEL(1, 23)), G.IN(2)))),
          "moog": G.moog_ladder, "softclip": G.soft_clip_cascade, "envelope": G.envelope_follower,
          "tanh": lambda: ("tanh", G.IN(1)), "exp": lambda: ("exp", G.IN(1)), "sqrt": lambda: ("sqrt", G.IN(1)), "min": lambda: ("min", G.IN(1), G.lit(0.5)),
          "sin": lambda: ("sin", G.IN(1)), "cos": lambda: ("cos", G.IN(1)), "log": lambda: ("log", G.IN(1)),
          "wire": lambda: G.IN(1), "cascade_params6": lambda: G.df1_cascade_params(6),
          "comb256": lambda: G.fb(G.add(G.mul(G.lit(0.5), G.DEL(1, 256)), G.IN(2))),
          "comb2000": lambda: G.fb(G.add(G.mul(G.lit(0.5), G.DEL(1, 2000)), G.IN(2)))}


def valu_count(expr, P, U=1, block=256, flags=0):
    """v_* instructions in the code object of a variant of the graph `expr` (s-expression): JIT into a scratch cache, disassemble"""
    with tempfile.TemporaryDirectory() as td:
        old = os.environ.get("FLOWZ_HIP_CACHE")
        os.environ["FLOWZ_HIP_CACHE"] = td
        try:
            F.compile(F.from_sexpr(expr)).build(F.make_variant(P, U, block, flags))
            f = glob.glob(td + "/*.hsaco")[0]
            dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f], text=True)
        finally:
            if old is None:
                os.environ.pop("FLOWZ_HIP_CACHE", None)
            else:
                os.environ["FLOWZ_HIP_CACHE"] = old
    return sum(1 for line in dis.splitlines() if line.split() and line.split()[0].startswith("v_"))


def valu_per_step(expr, P):
    """VALU instructions per step of the graph in a kernel of P streams per lane, unroll 1: its count minus that of the bare wire _1,
    divided by the copies of the step the kernel holds (measured with a chain of 32 additions, which is 32 instructions a step)"""
    base = valu_count(G.IN(1), P)
    chain = G.IN(1)
    for _ in range(32):
        chain = G.add(chain, G.lit(0.5))
    copies = (valu_count(chain, P) - base) / 32.0
    return (valu_count(expr, P) - base) / copies


def loss_grad_line(name, sm):
    p = F.compile(F.from_sexpr(GRAPHS[name]()))
    r, q = p.loss_grad_resources(stream_major=sm), p.grad_resources(stream_major=sm)
    return (f"{name} {'stream' if sm else 'time'}-major {p.loss_grad_kernel_symbol(stream_major=sm)}: C {r['unroll']}, {r['vgprs'] + r['agprs']} VGPRs "
            f"(plain adjoint {q['vgprs'] + q['agprs']}), {r['vgpr_spills']} VGPR / {r['sgpr_spills']} SGPR spills (plain {q['vgpr_spills']} / {q['sgpr_spills']}), "
            f"{r['scratch_bytes']} B scratch, {r['lds_bytes']} B LDS")


def states_line(name, sm):
    p = F.compile(F.from_sexpr(GRAPHS[name]()))
    r = p.states_resources(sm)
    return (f"{name} {'stream' if sm else 'time'}-major {p.states_kernel_symbol(sm)}: U {r['unroll']}, {r['vgprs'] + r['agprs']} VGPRs, "
            f"{r['vgpr_spills']} VGPR / {r['sgpr_spills']} SGPR spills, {r['scratch_bytes']} B scratch, {r['lds_bytes']} B LDS")


def ring_grad_lines(name, loss=False, sm=False, far=False):
    """the ring adjoint kernel at the default stride C, and its ds_* / vector-memory instructions per row of a chunk: the difference of
    the kernels at C and C / 2 over C / 2 rows -- both sweeps unroll a chunk, everything outside the chunks cancels.
    loss: the kernel of fz_run_block_ring_loss_grad, with the plain ring kernel's registers and spills next to its own.
    sm: the kernels for stream-major buffers (their per-row ds_* include the row's frames read from and written to the LDS patch; the
    patch fetch and flush are outside the chunks and cancel)
    far: the kernels of the far family (fz_run_block_far_grad, fz_run_block_far_loss_grad, sm: their _stream_major twins), with the
    path of sweep 2"""
    import far_grad_graphs as FG
    import ring_loss_graphs as RL
    build = (FG.FARS.get(name) if far else None) or RL.GRAPHS.get(name) or GRAPHS[name]
    p = F.compile(F.from_sexpr(build()))
    if far:
        resources = (lambda q, c=0: q.far_loss_grad_resources(c, stream_major=sm)) if loss else (lambda q, c=0: q.far_grad_resources(c, stream_major=sm))
    else:
        resources = (lambda q, c=0: q.ring_loss_grad_resources(c, stream_major=sm)) if loss else (lambda q, c=0: q.ring_grad_resources(c, stream_major=sm))
    r = resources(p)
    C = r["unroll"]

    def counts(c):
        with tempfile.TemporaryDirectory() as td:
            os.environ["FLOWZ_HIP_CACHE"] = td
            q = F.compile(F.from_sexpr(build()))
            resources(q, c)
            dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", glob.glob(td + "/*.hsaco")[0]], text=True)
        ops = [ln.split()[0] for ln in dis.splitlines() if ln.split()]
        vmem = [o for o in ops if o.startswith(("global_load", "global_store", "buffer_load", "buffer_store", "flat_load", "flat_store"))]
        return {"ds_read": sum(o.startswith("ds_read") for o in ops), "ds_write": sum(o.startswith("ds_write") for o in ops),
                "vmem_load": sum("load" in o for o in vmem), "vmem_store": sum("store" in o for o in vmem), "valu": sum(o.startswith("v_") for o in ops)}
    old = os.environ.get("FLOWZ_HIP_CACHE")
    try:
        whole = counts(C)
        half = counts(C // 2) if C > 1 else None
    finally:
        if old is None:
            os.environ.pop("FLOWZ_HIP_CACHE", None)
        else:
            os.environ["FLOWZ_HIP_CACHE"] = old
    if far:
        plain = p.far_grad_resources(0, stream_major=sm) if loss else None
        sym = p.far_loss_grad_kernel_symbol(0, stream_major=sm) if loss else p.far_grad_kernel_symbol(0, stream_major=sm)
        cfg = p.far_grad_source(0).split("// ==== fz_graph_body.h ====")[0]     # (the generated configuration: one text holds both modes)
        sym += " (" + ("no far line" if "#define FZ_FAR 1 " not in cfg else "fast path" if "#define FZ_FAR_FAST 1 " in cfg else "per-row path") + ")"
    else:
        plain = p.ring_grad_resources(0, stream_major=sm) if loss else None
        sym = p.ring_loss_grad_kernel_symbol(0, stream_major=sm) if loss else p.ring_grad_kernel_symbol(0, stream_major=sm)
    kin = "plain far" if far else "plain ring"
    out = [f"{name} {sym}: C {C}, {r['vgprs'] + r['agprs']} VGPRs"
           + (f" ({kin} {plain['vgprs'] + plain['agprs']})" if loss else "") + f", {r['vgpr_spills']} VGPR / {r['sgpr_spills']} SGPR spills"
           + (f" ({kin} {plain['vgpr_spills']} / {plain['sgpr_spills']})" if loss else "") + f", {r['scratch_bytes']} B scratch, {r['lds_bytes']} B LDS",
           "  in the kernel: " + ", ".join(f"{v} {k}" for k, v in whole.items())]
    if half:
        out.append("  per row (both sweeps): " + ", ".join(f"{(whole[k] - half[k]) / (C - C // 2):.2f} {k}" for k in whole))
    return out


def ring_states_lines(name, sm=False, far=False):
    """the ring states kernel: its resources next to the ring adjoint kernel's, and the instructions of its text -- the unrolled group of
    U rows (U ring-read sets, U ds_write per ring line, the next group's U x loads) plus the two state dumps (block start, state_out).
    sm: the kernel for stream-major buffers (its ds_* include the patch: the fetched pieces parked, the group's own-row reads; its
    vector-memory loads are the patch fetch, the state and the coefficients)
    far: the far states kernel (fz_run_recording_far_grad; with sm fz_run_recording_far_grad_for on stream-major buffers) next to the
    far adjoint kernel of the layout: per row of the group one vector-memory load per far read (those at a delay of at least 2 U with
    the next group's x rows, on stream-major buffers a group ahead of the patch's rows: the table) and one store per far line; the two
    dumps copy a far line's slots in a loop of four"""
    import far_grad_graphs as FG
    import ring_loss_graphs as RL
    build = (FG.FARS.get(name) if far else None) or RL.GRAPHS.get(name) or GRAPHS[name]
    p = F.compile(F.from_sexpr(build()))
    states_resources = (lambda q: q.far_states_resources(stream_major=sm)) if far else (lambda q: q.ring_states_resources(stream_major=sm))
    r, ring = states_resources(p), p.far_grad_resources(0, stream_major=sm) if far else p.ring_grad_resources(0, stream_major=sm)
    old = os.environ.get("FLOWZ_HIP_CACHE")
    try:
        with tempfile.TemporaryDirectory() as td:
            os.environ["FLOWZ_HIP_CACHE"] = td
            states_resources(F.compile(F.from_sexpr(build())))
            dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", glob.glob(td + "/*.hsaco")[0]], text=True)
    finally:
        if old is None:
            os.environ.pop("FLOWZ_HIP_CACHE", None)
        else:
            os.environ["FLOWZ_HIP_CACHE"] = old
    ops = [ln.split()[0] for ln in dis.splitlines() if ln.split()]
    vmem = [o for o in ops if o.startswith(("global_load", "global_store", "buffer_load", "buffer_store", "flat_load", "flat_store"))]
    n = {"ds_read": sum(o.startswith("ds_read") for o in ops), "ds_write": sum(o.startswith("ds_write") for o in ops),
         "vmem_load": sum("load" in o for o in vmem), "vmem_store": sum("store" in o for o in vmem), "valu": sum(o.startswith("v_") for o in ops),
         "s_barrier": ops.count("s_barrier"), "atomic": sum("atomic" in o for o in ops)}
    sym = p.far_states_kernel_symbol(stream_major=sm) if far else p.ring_states_kernel_symbol(stream_major=sm)
    geo = f"R {sym.split('_g')[0].split('r')[-1].split('b')[0]}, {sym.split('_g')[0].split('b')[-1]} lanes, " if sm else ""
    kin = "far adjoint" if far else "ring adjoint"
    out = [f"{name} {sym}: U {r['unroll']}, {geo}{r['vgprs'] + r['agprs']} VGPRs ({kin} {ring['vgprs'] + ring['agprs']}), "
           f"{r['sgprs']} SGPRs, {r['vgpr_spills']} VGPR / {r['sgpr_spills']} SGPR spills ({kin} {ring['vgpr_spills']} / {ring['sgpr_spills']}), "
           f"{r['scratch_bytes']} B scratch, {r['lds_bytes']} B LDS ({kin} {ring['lds_bytes']})",
           "  in the kernel: " + ", ".join(f"{v} {k}" for k, v in n.items())]
    if far:
        import re
        src = p.far_states_source(stream_major=sm)
        table = [re.search(r"%s\[\d+\] = \{([^}]*)\}" % t, src) for t in ("fz_fr_delay", "fz_fr_ahead")]
        if "#define FZ_FAR 1 " in src.split("// ==== fz_graph_body.h ====")[0] and all(table):
            out.append("  far reads at delays {" + table[0].group(1) + "}: with the next group's x rows {" + table[1].group(1) + "}")
        else:
            out.append("  no far line: the ring states kernel")
    return out


def main():
    a = sys.argv[1:]
    sm = False
    if "--layout" in a:
        i = a.index("--layout")
        if a[i + 1:i + 2] not in (["stream-major"], ["time-major"]):
            sys.exit("--layout time-major | stream-major")
        sm = a[i + 1] == "stream-major"
        del a[i:i + 2]
    if a and a[0] == "ringstates":
        names = [a[1] if len(a) > 1 else "ldsring"]
        if names == ["all"]:
            import ring_loss_graphs as RL
            names = sorted(RL.GRAPHS)
        for n in names:
            print("\n".join(ring_states_lines(n, sm)))
        return
    if a and a[0] == "farstates":
        names = [a[1] if len(a) > 1 else "far_comb"]
        if names == ["all"]:
            import far_grad_graphs as FG
            names = sorted(FG.FARS)
        for n in names:
            print("\n".join(ring_states_lines(n, sm, far=True)))
        return
    if a and a[0] == "ringgrad":
        print("\n".join(ring_grad_lines(a[1] if len(a) > 1 else "ldsring", sm=sm)))
        return
    if a and a[0] == "ringlossgrad":
        print("\n".join(ring_grad_lines(a[1] if len(a) > 1 else "ldsring", loss=True, sm=sm)))
        return
    if a and a[0] in ("fargrad", "farlossgrad"):
        print("\n".join(ring_grad_lines(a[1] if len(a) > 1 else "far_comb", loss=a[0] == "farlossgrad", sm=sm, far=True)))
        return
    if a and a[0] == "states":
        print(states_line(a[1] if len(a) > 1 else "cascade_params6", len(a) > 2 and a[2] == "sm"))
        return
    if a and a[0] == "lossgrad":
        print(loss_grad_line(a[1] if len(a) > 1 else "cascade_params6", len(a) > 2 and a[2] == "sm"))
        return
    name = a[0] if a else "cascade6"
    P, U, B, FL = (int(a[i]) if len(a) > i else d for i, d in ((1, 2), (2, 8), (3, 256), (4, 0)))
    with tempfile.TemporaryDirectory() as td:
        os.environ["FLOWZ_HIP_CACHE"] = td
        p = F.compile(F.from_sexpr(GRAPHS[name]()))
        p.build(F.make_variant(P, U, B, FL))
        f = glob.glob(td + "/*.hsaco")[0]
        llvm = "/opt/rocm/lib/llvm/bin/"
        dis = subprocess.check_output([llvm + "llvm-objdump", "-d", f], text=True)
        notes = subprocess.check_output([llvm + "llvm-readelf", "--notes", f], text=True)
        if len(a) > 5:
            open(a[5], "w").write(dis)
    hist = {}
    for line in dis.splitlines():
        t = line.split()
        if len(t) > 1 and t[0][0] in "vsgbd" and "_" in t[0]:
            hist[t[0]] = hist.get(t[0], 0) + 1
    print(f"{name} P={P} U={U} block={B} flags={FL}: ops/sample={p.n_ops} state={p.n_state}")
    for k, v in sorted(hist.items(), key=lambda kv: -kv[1]):
        print(f"  {v:6d} {k}")
    for line in notes.splitlines():
        if any(s in line for s in (".vgpr_count", ".sgpr_count", "spill_count", "private_segment_fixed", "group_segment_fixed", ".agpr_count")):
            print(" ", line.strip())


if __name__ == "__main__":
    main()
