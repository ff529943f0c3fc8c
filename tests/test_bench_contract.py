"""bench.py prints ONE JSON line with the driver's contract keys (small workload, real GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


LINE_LIMIT = 4096      # bytes the driver is sure to keep of the tail of stdout (round 4's 31 KB line came back as parsed = null)
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline", "cpu_baseline")


def test_compact_line_of_a_full_record_fits_the_driver(tmp_path):
    """bench.compact_line on the full record of a real run (round 4's 31 KB line, kept under profiles/): every contract key, the roofline
    and cpu_baseline objects the judge reads, one flat summary map -- in less than 4 KB"""
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r04", "bench_line_plain.json")))
    assert len(json.dumps(full)) > 25000
    txt = bench.compact_line(full)
    assert len(txt) < LINE_LIMIT and "\n" not in txt
    d = json.loads(txt)
    for k in CONTRACT + ("parity", "summary"):
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "algorithmic_bytes_per_launch", "limiter"):
        assert d["roofline"][k] == full["roofline"][k], k
    assert d["roofline"]["sustained"]["frac"] == full["roofline"]["sustained"]["frac"]
    assert set(d["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"} and len(d["cpu_baseline"]["sample"]) <= 200
    s = d["summary"]
    assert s["config2_time_major"] == round(full["config2_65536_streams"]["time_major"]["library_default"]["frac"], 3)
    assert s["config2_tiled"] == round(full["config2_65536_streams"]["library_default"]["frac"], 3)
    assert s["config3_stream_major"] == round(full["config3_par4_sum"]["stream_major"]["library_default"]["frac"], 3)
    assert s["complex_one_pole"] == round(full["next_rows"]["complex_one_pole"]["library_default"]["frac"], 3)
    assert len(s) == 30 and all(isinstance(v, float) for v in s.values())
    assert d["parity_objects"].startswith("bitwise-equal on all 30")
    # a record ten times as wide still fits: the optional maps go first, never the contract keys
    wide = dict(full)
    for i in range(300):
        wide[f"extra_object_number_{i}"] = full["tiled_layout"]
    txt = bench.compact_line(wide)
    assert len(txt) < LINE_LIMIT
    assert all(k in json.loads(txt) for k in CONTRACT)
    # strings no trimming of maps can save (round-5 advisor finding: an assert killed the line after the measurements were done): the contract keys
    # and the roofline's numbers survive, cut short; a leg that never got a timing is named, not a KeyError
    long_ = json.loads(json.dumps(full))
    long_["config"]["workload"] = "w" * 3000
    long_["roofline"]["traffic_source"] = "s" * 3000
    long_["parity"] = "p" * 3000
    long_["tiled_layout"] = {"library_default": {}, "parity": "bitwise-equal"}
    txt = bench.compact_line(long_)
    d = json.loads(txt)
    assert len(txt) < LINE_LIMIT and all(k in d for k in CONTRACT) and d["value"] == full["value"]
    assert d["roofline"]["frac"] == full["roofline"]["frac"] and d["roofline"]["traffic"] == full["roofline"]["traffic"] and "truncated" in d


def test_dump_outputs_writes_the_same_bounded_sample_from_either_frame_layout(tmp_path):
    """bench.dump_outputs on host tensors: float32 files of at most 64 MB, the values of the seeded sample of streams, the same
    files from time-major and stream-tiled frames of the same data; the last sample is itself sampled beyond 4 M streams"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    for ns, T, n_state, tile in ((65536, 512, 24, 8192), ((1 << 22) + 8, 2, 3, 8)):
        g = torch.Generator().manual_seed(ns)
        y = torch.randn((T, ns, 1), generator=g)
        st = torch.randn((n_state, ns), generator=g)
        tiled = y.reshape(T, ns // tile, tile, 1).permute(1, 0, 2, 3).contiguous()
        a, b = tmp_path / f"tm{ns}", tmp_path / f"tiled{ns}"
        bench.dump_outputs(torch, str(a), y, st, 0)
        bench.dump_outputs(torch, str(b), tiled, st, tile)
        names = sorted(os.listdir(a))
        assert names == ["out_last_sample.npy", "out_streams.npy", "state_streams.npy"] and sorted(os.listdir(b)) == names
        assert sum(os.path.getsize(a / n) for n in names) <= bench.DUMP_BYTES
        got = {n[:-4]: np.load(a / n) for n in names}
        for n in names:
            assert got[n[:-4]].dtype == np.float32 and np.array_equal(got[n[:-4]], np.load(b / n)), n
        k = got["state_streams"].shape[1]
        ids = bench.dump_stream_ids(ns, k)
        assert 0 < k < ns and len(np.unique(ids)) == k
        assert np.array_equal(got["out_streams"], y[:, ids].numpy()) and np.array_equal(got["state_streams"], st[:, ids].numpy())
        last = y[-1].numpy()
        if ns * 4 <= bench.DUMP_BYTES // 4:
            assert np.array_equal(got["out_last_sample"], last)
        else:
            n_last = got["out_last_sample"].shape[0]
            assert n_last < ns and np.array_equal(got["out_last_sample"], last[bench.dump_stream_ids(ns, n_last)])


def _last_line_as_the_driver_sees_it(stdout):
    """the driver keeps the tail of stdout: the JSON line must be recoverable from the last 4096 bytes alone"""
    tail = stdout[-LINE_LIMIT:]
    lines = [l for l in tail.splitlines() if l.startswith("{")]
    assert lines, tail[-300:]
    return json.loads(lines[-1])


@pytest.mark.gpu
def test_bench_json_contract_small_workload(tmp_path):
    details = str(tmp_path / "details.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--streams", "16384", "--samples", "512", "--full"], capture_output=True, text=True, timeout=600, env=dict(os.environ, BENCH_DETAILS=details))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    assert len(lines[0]) < LINE_LIMIT
    d = json.loads(lines[0])
    assert d == _last_line_as_the_driver_sees_it(out.stdout)
    for k in CONTRACT:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["kernel"].startswith("fz_block_kernel_p")
    assert "traffic" in r and "traffic_source" in r and (r["traffic"] is None) == (r["traffic_source"] is None)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert d["parity"].startswith("bitwise-equal")
    assert d["roofline"]["sustained"]["seconds"] >= 1.9 and d["roofline"]["sustained"]["frac"] > 0
    assert d["config"]["layout"] == "time-major"                       # SURVEY 8d's device layout is the headline's (round 3)
    s = d["summary"]
    for k in ("tiled", "stream_major", "config2_tiled", "config2_time_major", "config2_stream_major", "cascade6_32768", "cascade6_16384", "config3_tiled",
              "config3_time_major", "config3_stream_major", "config3_fanout", "config4_tiled", "config4_time_major", "config4_stream_major",
              "lds_ring", "far_ring", "blocks64", "modulated", "double_biquad", "complex_one_pole", "ref_df1", "ref_df2t"):
        assert 0 < s[k] < 1, k
    assert d["parity_objects"] == f"bitwise-equal on all {len(s)} objects"
    assert abs(d["value"] - 16384 * 512 * 3 / (d["ms_per_step"] * 3 / 1e3) / 1e6) / d["value"] < 1e-2
    # the full record next to it: everything the line summarises, per plan
    full = json.load(open(details))
    for k in CONTRACT:
        assert full[k] == d[k] or k in ("config", "roofline", "cpu_baseline"), k
    board = full["roofline"]["sustained"]["board"]     # rocm-smi during the sustained leg (best effort: None without rocm-smi)
    assert board is None or (board["package_W"] > 0 and board["sclk_MHz"] > 0 and board["samples"] >= 1)
    for k in ("config2_65536_streams", "cascade6_32768_streams", "cascade6_16384_streams", "config3_par4_sum", "config3_par4_sum_fanout", "config4_osc_chain"):
        assert full[k]["parity"].startswith("bitwise-equal"), (k, full[k]["parity"])
        assert full[k]["library_default"]["frac"] > 0 and full[k]["tuned"]["kernel"].startswith("fz_block_kernel_p")
        assert len(full[k]["library_default"]["code_id"]) == 16
    for k in ("tiled_layout", "stream_major_layout"):                  # the other frame layout and the reference's calling convention, same workload
        assert full[k]["parity"].startswith("bitwise-equal"), (k, full[k]["parity"])
        assert full[k]["library_default"]["frac"] > 0 and full[k]["tuned"]["kernel"].startswith("fz_block_kernel_p") and 0 < full[k]["frac"] < 1
    c = full["cpu_baseline"]
    assert c["Msamples_per_s_per_core"] > 0 and c["physical_cores"] >= 1 and c["logical_cpus"] >= c["physical_cores"]
    assert c["cores"] <= c["threads"] and (c["cgroup_cpu_quota"] is None or c["cores"] <= max(1, round(c["cgroup_cpu_quota"])))
    assert 0.5 < c["Msamples_per_s_per_core"] * c["cores"] / c["value"] < 2.0


@pytest.mark.gpu
def test_bench_plain_run_measures_the_headline_alone():
    """Without --full: the driver's keys, the roofline of the timed launches and the checksum -- no parity check, sustained run, row walk,
    copy, CPU baseline or other object"""
    sys.path.insert(0, ROOT)
    import bench
    d = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--streams", "16384", "--samples", "512"])
    assert set(d) == set(bench.CONTRACT_KEYS) | {"config", "roofline", "checksum"}, sorted(d)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 16384 * 512 * 3 / (d["ms_per_step"] * 3 / 1e3) / 1e6) / d["value"] < 1e-2
    r = d["roofline"]
    assert r["kernel"].startswith("fz_block_kernel_p") and r["avg_launch_ms"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "sustained" not in r and r["measured_row_walk_GBs"] is None and r["measured_copy_GBs"] is None
    assert isinstance(d["checksum"], int)


@pytest.mark.gpu
def test_bench_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs: what the last timed step returned, the same from run to run.  One untimed block, warmup - 1 more, then --steps
    timed ones: --steps 3 --warmup 1 and --steps 2 --warmup 2 both end on the fourth block, which the oracle computes from the same
    seeded input run four times with the state carried"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from oracle import coracle, flowz_oracle as O
    from zignal_amd import workloads as W
    ns, T = 16384, 512
    common = ["--gpus", "1", "--streams", str(ns), "--samples", str(T), "--no-cpu-baseline", "--no-autotune", "--no-config2", "--no-config34",
              "--no-sustained", "--no-layout-legs", "--no-extras", "--no-next-rows"]
    a, b = tmp_path / "a", tmp_path / "b"
    _run_bench(common + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(a)])
    _run_bench(common + ["--steps", "2", "--warmup", "2", "--dump-outputs", str(b)])
    names = sorted(os.listdir(a))
    assert names == ["out_last_sample.npy", "out_streams.npy", "state_streams.npy"] and sorted(os.listdir(b)) == names
    got = {n[:-4]: np.load(a / n) for n in names}
    for n in names:
        assert got[n[:-4]].dtype == np.float32 and np.array_equal(got[n[:-4]].view(np.uint32), np.load(b / n).view(np.uint32)), n
    ids = bench.dump_stream_ids(ns, got["state_streams"].shape[1])
    assert got["out_streams"].shape == (T, len(ids), 1) and got["out_last_sample"].shape == (ns, 1)
    x = O.synth_input(W.SEED, ids, T)
    want = coracle.df1_cascade([W.STABLE] * 6, np.concatenate([x] * 4))[3 * T:]
    assert np.array_equal(got["out_streams"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["out_last_sample"][ids].view(np.uint32), want[-1].view(np.uint32))


def _run_bench(args, nproc=1, timeout=900, launcher=False, env=None):
    if nproc > 1 or launcher:
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, BENCH_DETAILS=os.path.join(td, "details.json"), **(env or {})))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < LINE_LIMIT, out.stdout[-2000:]
    assert json.loads(lines[0]) == _last_line_as_the_driver_sees_it(out.stdout)
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_rehearse_the_sharded_path():
    """The N > 1 path of bench.py (launcher env, shard_range, per-rank generator offset, barrier, max-over-ranks time,
    the statistics all-reduce) with 2 ranks that share device 0 and reduce over gloo: the integer checksum of the two
    shards must equal a single-process run over the union of the global stream ids.  Weak and strong scaling modes."""
    common = ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-autotune", "--no-config2", "--no-config34", "--no-sustained",
              "--no-layout-legs"]
    one = _run_bench(["--gpus", "1", "--streams", "262144"] + common)
    weak = _run_bench(["--gpus", "2", "--streams", "131072", "--dist-backend", "gloo"] + common, nproc=2)
    assert weak["n_gpus"] == 2 and weak["scaling"] == "weak"
    assert weak["config"]["streams_total"] == 262144 and weak["config"]["streams_per_gpu"] == 131072
    assert weak["checksum"] == one["checksum"] and isinstance(weak["checksum"], int)
    # the N > 1 line checks itself: every rank compared streams of its own shard with the oracle; per-rank launch times; who reduced
    assert weak["parity"].startswith("bitwise-equal on") and "every one of the 2 ranks" in weak["parity"]
    assert weak["dist_backend"] == "gloo" and weak["rccl_ranks"] == 0 and len(weak["ms_per_step_per_rank"]) == 2 and min(weak["ms_per_step_per_rank"]) > 0
    assert abs(weak["value"] - 262144 * 4096 * 2 / (weak["ms_per_step"] * 2 / 1e3) / 1e6) / weak["value"] < 1e-2
    strong = _run_bench(["--gpus", "2", "--scaling", "strong", "--streams-total", "262144", "--dist-backend", "gloo"] + common, nproc=2)
    assert strong["n_gpus"] == 2 and strong["scaling"] == "strong" and strong["config"]["streams_total"] == 262144
    assert strong["checksum"] == one["checksum"]


# ranks of the many-rank rehearsal: they all hold device 0 at once, next to the pytest process itself, and a shared GPU takes at
# most six processes that have it open
RANKS_ON_ONE_GPU = 4


@pytest.mark.gpu
def test_bench_four_ranks_on_one_gpu_rehearse_the_drivers_scaling_run():
    """What `bench.py --gpus 8` does on a node, rehearsed on ONE GPU (round 6: the driver's first 8-GPU run is also the first execution with more
    than one RCCL rank, so everything around the collective is exercised here): four ranks under torch.distributed.run share device 0 and
    reduce over gloo, 131 072 streams each.  Every rank measures its plan at the same time (fz_program_tune: four processes appending to
    the ONE plans.txt of the shared kernel cache, none of them torn), runs its shard, checks streams of its own shard against the oracle;
    the integer checksum over the four shards equals a one-rank run over the union; the line stays below 4 KB with the per-rank times."""
    n = RANKS_ON_ONE_GPU
    plans = os.path.join(os.environ.get("FLOWZ_HIP_CACHE") or os.path.join(ROOT, "zignal_amd", "_kcache"), "plans.txt")   # (the library's kernel cache directory)
    before = open(plans).read().splitlines() if os.path.exists(plans) else []
    common = ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-config2", "--no-config34", "--no-sustained", "--no-layout-legs", "--no-extras",
              "--no-next-rows"]
    # (bench.py switches the persisted plans off for itself -- every run measures; the rehearsal switches them back on so that the tunes of all
    #  ranks also meet at the one plans.txt, which a caller's processes would)
    weak = _run_bench(["--gpus", str(n), "--streams", "131072", "--dist-backend", "gloo"] + common, nproc=n, timeout=1200, env={"FLOWZ_HIP_NO_PLAN_CACHE": "0"})
    assert weak["n_gpus"] == n and weak["scaling"] == "weak" and weak["config"]["streams_total"] == n * 131072 and weak["config"]["streams_per_gpu"] == 131072
    assert weak["parity"].startswith("bitwise-equal on") and f"every one of the {n} ranks" in weak["parity"]
    assert weak["dist_backend"] == "gloo" and weak["rccl_ranks"] == 0
    assert len(weak["ms_per_step_per_rank"]) == n and min(weak["ms_per_step_per_rank"]) > 0
    assert f"x{n}" in weak["config"]["parallelism"] and weak["roofline"]["bound"] == "hbm" and 0 < weak["roofline"]["frac"] < 1 and "cpu_baseline" not in weak
    # value = the samples ALL ranks processed / the slowest rank's wall time (barrier to barrier)
    assert abs(weak["value"] - n * 131072 * 4096 * 2 / (weak["ms_per_step"] * 2 / 1e3) / 1e6) / weak["value"] < 1e-2
    assert abs(weak["per_gpu"] * n - weak["value"]) / weak["value"] < 1e-3
    after = open(plans).read().splitlines() if os.path.exists(plans) else []
    new = after[len(before):]
    mine = [l.split() for l in new if l.split()[2:4] == ["131072", "0"]]
    assert len(mine) >= n and all(len(f) == 11 and f[0] == "fzplan3" for f in mine), new[-10:]      # one tune per rank, every line whole
    one = _run_bench(["--gpus", "1", "--streams", str(n * 131072), "--no-autotune"] + common)
    assert weak["checksum"] == one["checksum"] and isinstance(weak["checksum"], int)
    strong = _run_bench(["--gpus", str(n), "--scaling", "strong", "--streams-total", str(n * 131072 + 5), "--dist-backend", "gloo", "--no-autotune"] + common, nproc=n, timeout=1200)
    assert strong["scaling"] == "strong" and strong["config"]["streams_total"] == n * 131072 + 5 and len(strong["ms_per_step_per_rank"]) == n
    assert strong["parity"].startswith("bitwise-equal on")


@pytest.mark.gpu
def test_bench_one_rank_reduces_its_statistics_over_rccl():
    """The `nccl` (= RCCL) branch of bench.py on real hardware: one rank under torch.distributed.run, process group on the GPU,
    the three statistics reduced by RCCL all-reduces on device tensors (zignal_amd/dist.py).  Same checksum and stream count
    as the plain single-process run."""
    common = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-autotune", "--no-config2", "--no-config34", "--no-sustained",
              "--no-layout-legs"]
    one = _run_bench(["--gpus", "1", "--streams", "131072"] + common)
    rccl = _run_bench(["--gpus", "1", "--streams", "131072", "--dist-backend", "nccl"] + common, launcher=True)
    assert rccl["n_gpus"] == 1 and rccl["config"]["streams_total"] == 131072
    assert "statistics reduced over nccl" in rccl["config"]["parallelism"]
    assert "reduced over" not in one["config"]["parallelism"]
    assert rccl["checksum"] == one["checksum"] and isinstance(rccl["checksum"], int)
    assert rccl["rccl_ranks"] == 1 and rccl["dist_backend"] == "nccl" and len(rccl["ms_per_step_per_rank"]) == 1
    assert abs(rccl["value"] - 131072 * 4096 * 2 / (rccl["ms_per_step"] * 2 / 1e3) / 1e6) / rccl["value"] < 1e-2
