"""The shapes of tests/test_host_pipeline_gpu.py (tests/host_pipeline_graphs.py) and the manifest of its kernels, without a GPU."""
import gzip

import host_pipeline_graphs as H


def test_every_frame_type_takes_the_pipeline_past_its_second_chunk():
    assert H.launch_rows(H.NS * 2 * 4) == [40, 40, 40, 40, 7]             # float32 out: 800-byte rows
    assert H.launch_rows(H.NS * 2 * 8) == [20] * 8 + [7]                  # float64 out: 1600-byte rows
    assert H.launch_rows(H.NS * 2 * 2) == [64, 64, 39]                    # int16 out: 400-byte rows, whole multiples of 32 from 64 rows on


def test_the_recorded_manifest_is_what_the_gpu_tests_resolve_now(tmp_path):
    """tests/golden/host_pipeline_kernels.fzm.gz against a fresh recording: another plan for these shapes, or another shape, needs it recorded again"""
    with open(H.MANIFEST, "rb") as f:
        assert gzip.decompress(f.read()) == H.record(str(tmp_path / "m.fzm"))
