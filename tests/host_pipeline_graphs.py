"""Shapes, graphs and kernels of tests/test_host_pipeline_gpu.py: the pipeline of fz_bank_process_host past its second chunk with
kilobytes.  FLOWZ_HIP_HOST_CHUNK_BYTES (read at every call) sets the bytes of a time chunk on the wider side.  100 streams of a graph
with 1 input and 2 output wires, 167 rows, 32 000 bytes a chunk:

    frames                 input row   output row   rows a chunk                       chunks of 167 rows   bytes of the wider side
    float32 -> float32     400 B       800 B        32000 // 800 = 40                  5 (4 x 40 + 7)       133 600
    float32 -> float64     400 B       1600 B       32000 // 1600 = 20                 9 (8 x 20 + 7)       267 200
    int16 -> int16         200 B       400 B        32000 // 400 = 80 -> 64 (from 64   3 (2 x 64 + 39)       66 800
                                                    rows on: whole multiples of 32)

Every case is past 2 x 32 000 bytes, so none takes the one-round-trip short cut, every slot is used more than once (the waits on the
events of chunk k - 2), the last chunk is ragged and the delay lines carry state across the chunks."""
import os
import subprocess
import sys

import graphs as G

NS, T, CHUNK_BYTES = 100, 167, 32000
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_pipeline_kernels.fzm.gz")


def two_out():
    """1 input, 2 outputs: a two-biquad cascade next to ~(0.9*_1[_1] - 0.8*_1[_2] + _2) -- eight state rows"""
    return G.chan(G.df1_cascade(2), G.one_quad())


def two_out_modulated():
    """the same shape with a sample-rate modulator in the first wire's recursion"""
    return G.chan(G.one_pole_modulated(), G.one_quad())


def chunk_rows(row_bytes):
    """rows of a time chunk of bank_process_host for rows of row_bytes on the wider side (fz_bank.cpp); asserts that T rows take the pipeline"""
    rows = CHUNK_BYTES // row_bytes
    assert T * row_bytes > 2 * CHUNK_BYTES and rows < T
    return rows & ~31 if rows >= 64 else rows


def launch_rows(row_bytes):
    """the rows of every chunk's launch, in order"""
    rows = chunk_rows(row_bytes)
    return [min(rows, T - t0) for t0 in range(0, T, rows)]


def resolve_kernels():
    """Resolve, as the launches do, every kernel the GPU tests run (needs no GPU).  The list is derived from fz_bank.cpp, not from a
    recording on a board: bank_process_host launches every chunk through fz::launch with no variant (float64 output: a variant of
    FZ_VF_OUT_F64 alone) at (NS streams, that chunk's rows) -- what Program.build(variant, NS, rows) resolves, one call per distinct
    chunk length of launch_rows() -- and int16 frames through launch_pcm16, whose plan depends on the stream count alone -- what
    pcm16_resources resolves.  A launch the list misses is built at run time on the GPU machine: seconds, not a failure."""
    from zignal_amd import flowz as F
    p, pm = F.compile(F.from_sexpr(two_out())), F.compile(F.from_sexpr(two_out_modulated()))
    for nt in sorted(set(launch_rows(NS * 2 * 4))):
        p.build(None, NS, nt)
        pm.build(None, NS, nt)
    for nt in sorted(set(launch_rows(NS * 2 * 8))):
        p.build(F.make_variant(0, 0, 0, F.C.FZ_VF_OUT_F64), NS, nt)
    p.pcm16_resources("int16", "int16", NS)


def record(path):
    """resolve_kernels() in a process that records (FLOWZ_HIP_MANIFEST): the raw manifest.  tests/golden/host_pipeline_kernels.fzm.gz,
    which the build replays into the kernel cache, is `gzip -9n` of it"""
    code = "import sys; sys.path[:0] = %r; import host_pipeline_graphs as H; H.resolve_kernels()" % ([os.path.dirname(os.path.dirname(MANIFEST)), os.path.dirname(os.path.dirname(os.path.dirname(MANIFEST)))],)
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, FLOWZ_HIP_MANIFEST=path))
    with open(path, "rb") as f:
        return f.read()
