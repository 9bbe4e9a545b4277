"""bench.py's command line: a plain run does the headline only, --full the rest; --dump-outputs writes lossless float arrays of
bounded size, the same on every run of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_skips_everything_but_the_headline(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert a.cpu_slices == 0 and a.cpu_pool == 0 and a.no_prof and not a.stream and a.latency_calls == 0 and not a.side
    assert a.dump_outputs is None


def test_full_run_keeps_every_leg(monkeypatch):
    import bench
    a = _parse(monkeypatch, "--full")
    assert a.cpu_slices == -1 and a.cpu_pool == bench.CPU_POOL and not a.no_prof and a.stream and a.latency_calls == 300 and a.side
    a = _parse(monkeypatch, "--full", "--workload", "w3")
    assert not a.side and not a.stream and not a.no_prof


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_as_float_is_lossless():
    import bench
    from eorb_slam_amd import synth
    kp = np.zeros(3, synth.KP_DTYPE)
    kp["x"] = [1.5, np.float32(1e-7), -3.25]; kp["octave"] = [0, 3, 7]; kp["class_id"] = [-1, 2 ** 31 - 1, 5]
    f = bench._as_float(kp)
    assert f.dtype == np.float64 and f.shape == (3, 7)
    assert np.array_equal(f[:, 0].astype(np.float32), kp["x"]) and np.array_equal(f[:, 6].astype(np.int64), kp["class_id"])
    assert bench._as_float(np.arange(256, dtype=np.uint8)).dtype == np.float32
    i32 = np.array([-2 ** 31, 2 ** 31 - 1], np.int32)
    assert np.array_equal(bench._as_float(i32).astype(np.int64), i32)
    assert bench._as_float(np.ones(2, np.float32)).dtype == np.float32


def test_dump_sample_is_fixed_and_bounded():
    import bench
    assert np.array_equal(bench._sample_units(10, 1000), np.arange(10))
    per = bench.DUMP_BYTES // 100 + 1
    s = bench._sample_units(1000, per)
    assert len(s) == 99 and np.all(np.diff(s) > 0) and np.array_equal(s, bench._sample_units(1000, per))


def test_dump_outputs_writes_float_npy_and_refuses_oversize(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path / "d"), {"a": np.arange(6, dtype=np.int32).reshape(2, 3), "b": np.ones(4, np.uint8)})
    a, b = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert a.dtype == np.float64 and a.tolist() == [[0, 1, 2], [3, 4, 5]] and b.dtype == np.float32
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros(bench.DUMP_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists()


def test_ragged_pads_and_counts():
    import bench
    out, n = bench._ragged([np.array([1, 2], np.int32), None, np.array([3], np.int32)], 3)
    assert out.tolist() == [[1, 2, 0], [0, 0, 0], [3, 0, 0]] and n.tolist() == [2, -1, 1]


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A small plain run twice: one short result line with the headline fields, and the same dumped outputs both times."""
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / ("out%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                            "--events", "30000", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    for line in lines:
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line
        assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert "cpu_baseline" not in line and "roofline" not in line and "side" not in line
    a, b = dumps
    assert set(a) == {"slices", "image", "n_keypoints", "keypoints", "descriptors", "matches12", "n_matches"} and set(a) == set(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["image"].shape == (4, 180, 240) and a["n_keypoints"].min() > 0
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
