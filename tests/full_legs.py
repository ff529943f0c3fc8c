"""The legs of the whole-output checks (test_full_output_gpu.py): the BASELINE workloads at the bench's full-size shapes, each leg one
frame layout of one workload under the library's static default, with the kernel that default resolves to.

A group is the legs of one workload, seed and stream range: they run on the device first and then share one oracle pass
(tests/full_check.py).  Groups stay within about 100 GiB of device memory: the kept outputs plus one input at a time.  That is why
config 3's four-wire frames (64 GiB of input per layout) and the complex one-pole's two-slot outputs (32 GiB each) check their
stream-major leg in a group of its own, on another seed.

test_full_output_host.py resolves every leg's kernel name without a GPU, so a planner change that moves a leg to another body fails
on a CPU first."""
import numpy as np

from oracle import coracle
from zignal_amd import flowz as F
from zignal_amd import workloads as W

C = F.C
K = "fz_block_kernel_"
SEED = 20160512
M1, T1 = 1 << 20, 4096
REFC = (W.B0, W.B1, W.B2, W.A1, W.A2)                 # the reference benchmark's coefficients (test/benchmark.cpp:18-23)


def _cascade(n):
    return lambda x, s0, s1, seed: coracle.df1_cascade([W.STABLE] * n, x, stream_major=True)


def _ref(fn):
    if fn == "df1":
        return lambda x, s0, s1, seed: coracle.df1_cascade([REFC], x, stream_major=True)
    return lambda x, s0, s1, seed: getattr(coracle, fn)(REFC, x, stream_major=True)


# workload -> (graph, typed, input wires, drive, oracle(x, s0, s1, seed) on stream-major [k, T, w] frames,
#              per-stream parameters(seed, stream ids) or None)
WORKLOADS = {
    "cascade6": (lambda: W.df1_cascade(6), False, 1, "noise", _cascade(6), None),
    "cascade2": (lambda: W.df1_cascade(2), False, 1, "noise", _cascade(2), None),
    "osc6": (lambda: W.osc_chain(6), False, 1, "dirac",
             lambda x, s0, s1, seed: coracle.osc_chain(W.osc_chain_params(seed, np.arange(s0, s1)), x, stream_major=True), W.osc_chain_params),
    "par4": (W.par4_sum, False, 4, "noise", lambda x, s0, s1, seed: coracle.par4_sum(W.PAR4_SETS, x, stream_major=True), None),
    "par4f": (W.par4_sum_fanout, False, 1, "noise",
              lambda x, s0, s1, seed: coracle.par4_sum(W.PAR4_SETS, x, fanout=True, stream_major=True), None),
    "c32onepole": (W.complex_one_pole, True, 1, "noise", lambda x, s0, s1, seed: coracle.complex_one_pole(x, stream_major=True, std=True), None),
    "df1": (W.df1, False, 1, "noise", _ref("df1"), None),
    "df2": (W.df2, False, 1, "noise", _ref("df2"), None),
    "df1t": (W.df1t, False, 1, "noise", _ref("df1t"), None),
    "df2t": (W.df2t, False, 1, "noise", _ref("df2t_flowz"), None),
}

# the second, explicitly chosen variant each leg's final state is compared with: (P, U, block, flags) -- on stream-major buffers
# without FZ_VF_STREAM_MAJOR, which the launch adds
SECOND = {"rows": (1, 16, 256, C.FZ_VF_NO_STAGE_PACK), "tiles": (1, 16, 256, C.FZ_VF_NO_STAGE_PACK), "sm": (1, 8, 0, 0)}

L, GS, P3, SP = C.FZ_VF_LOCKSTEP, C.FZ_VF_GRID_SYNC, C.FZ_VF_PREFETCH3, C.FZ_VF_STAGE_PACK

# (group, priority a / b / c, workload, seed, n_streams, n_samples, [(layout, tile streams, kernel the static default resolves to)])
GROUPS = [
    # (a) never launched by any test, or never checked beyond sampled streams
    ("cascade6-786432", "a", "cascade6", SEED + 201, 786_432, T1, [("rows", 0, K + "p4u1b768f%d" % (L | GS | P3))]),
    ("cascade6-393216", "a", "cascade6", SEED + 202, 393_216, T1, [("rows", 0, K + "p2u2b768f%d" % (L | GS))]),
    ("cascade6-1M", "a", "cascade6", SEED, M1, T1, [("sm", 0, K + "p2u64b64f384"),
                                                    ("rows", 0, K + "p4u1b1024f%d" % (L | GS | P3)),           # (b)
                                                    ("tiles", 8192, K + "p2u2b1024f%d" % (L | GS))]),          # (b)
    ("osc6-1M", "a", "osc6", SEED + 1, M1, T1, [("rows", 0, K + "p1u4b1024s6f%d" % (L | GS | SP)),
                                            ("tiles", 8192, K + "p2u16b256f%d" % C.FZ_VF_MAX_WG(2)),
                                            ("sm", 0, K + "p2u64b64f384")]),
    ("par4f-1M", "a", "par4f", SEED + 203, M1, T1, [("rows", 0, K + "p4u1b1024f%d" % (L | GS | P3)),
                                                    ("tiles", 8192, K + "p2u2b1024f%d" % (L | GS)),
                                                    ("sm", 0, K + "p1u128b64f384")]),
    ("par4-1M", "a", "par4", SEED + 204, M1, T1, [("rows", 0, K + "p1u3b1024f%d" % (L | GS)),                  # (b)
                                                  ("tiles", 4096, K + "p1u32b256f0")]),
    ("par4-1M-sm", "a", "par4", SEED + 205, M1, T1, [("sm", 0, K + "p1u32b256f128")]),
    ("c32onepole-1M", "a", "c32onepole", SEED + 206, M1, T1, [("rows", 0, K + "p4u1b1024f%dL" % (L | GS | P3)),
                                                              ("tiles", 8192, K + "p2u16b256f%d" % C.FZ_VF_MAX_WG(2))]),
    ("c32onepole-1M-sm", "a", "c32onepole", SEED + 207, M1, T1, [("sm", 0, K + "p1u32b256f128")]),
    ("cascade6-2097152", "a", "cascade6", SEED + 208, 2_097_152, T1, [("rows", 0, K + "p2u2b1024f%d" % (L | GS))]),
    ("cascade6-1048577", "a", "cascade6", SEED + 209, 1_048_577, T1, [("rows", 0, K + "p4u1b1024f%dM" % (L | GS | P3)),
                                                                      ("sm", 0, K + "p1u128b64s6f392")]),
    # (b) bench shapes that rested on another kernel of the library for most streams
    ("cascade6-1000000", "b", "cascade6", SEED + 210, 1_000_000, T1, [("rows", 0, K + "p4u1b1024f%d" % (L | GS | P3))]),
    ("cascade6-65536", "b", "cascade6", SEED + 211, 65_536, T1, [("rows", 0, K + "p1u16b256w1io2f33587200"),        # (wave-split bodies)
                                                                 ("tiles", 8192, K + "p1u16b256w1io2f33587200"),
                                                                 ("sm", 0, K + "p1u128b64s6f392")]),
    ("cascade6-262144", "b", "cascade6", SEED + 212, 262_144, T1, [("sm", 0, K + "p1u128b64s6f392")]),
    ("cascade6-32768", "b", "cascade6", SEED + 213, 32_768, T1, [("rows", 0, K + "p1u32b128w2iof33792")]),
    ("cascade6-16384", "b", "cascade6", SEED + 214, 16_384, T1, [("rows", 0, K + "p1u32b64w3iof34816")]),
    ("cascade2-16M", "b", "cascade2", SEED + 215, 1 << 24, 24, [("rows", 0, K + "p2u16b256f0"),
                                                                ("tiles", 8192, K + "p2u16b256f%d" % C.FZ_VF_MAX_WG(2))]),
    # (c) the reference's four single-biquad topologies (test/benchmark.cpp:157-262)
] + [("%s-1M" % n, "c", n, SEED + 216, M1, T1, [("rows", 0, K + "p4u1b1024f%d" % (L | GS | P3))]) for n in ("df1", "df2", "df1t", "df2t")]


def program(workload):
    graph, typed = WORKLOADS[workload][:2]
    return F.compile(F.from_sexpr(graph()), typed=typed)


def variant(layout, v=None):
    """the launch's variant (None: the library's choice); stream-major buffers add FZ_VF_STREAM_MAJOR for the kernel name"""
    v = v or (0, 0, 0, 0)
    return F.make_variant(v[0], v[1], v[2], v[3] | (C.FZ_VF_STREAM_MAJOR if layout == "sm" else 0))


def kernel_name(prog, layout, ns, T, tile, v=None):
    if layout == "sm":
        return prog.kernel_name(variant(layout, v), ns, T)
    return prog.kernel_name(F.make_variant(*v) if v else None, ns, T, tile)


def host_input(workload, seed, s0, s1, T):
    """the input of streams [s0, s1), stream-major [k, T, w]: the host generator or the dirac drive"""
    n_in, drive = WORKLOADS[workload][2:4]
    if drive == "dirac":
        x = np.zeros((s1 - s0, T, 1), np.float32)
        x[:, 0] = 1.0
        return x
    return coracle.synth_fill(seed, s0, s1 - s0, T, n_in, stream_major=True)


def reference(workload, seed, T):
    """reference(s0, s1) -> (x, want) for full_check.check"""
    orc = WORKLOADS[workload][4]

    def f(s0, s1):
        x = host_input(workload, seed, s0, s1, T)
        return x, orc(x, s0, s1, seed)
    return f
