"""bench.py --dump-outputs: the last timed step's waveforms as float32 .npy
files, whole below the byte cap and a fixed seeded sample above it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _waves():
    r = np.random.default_rng(3)
    return [r.standard_normal(1920 * 4).astype(np.float32), None, r.standard_normal(1920 * 7).astype(np.float32)]


def test_dump_outputs_whole(tmp_path):
    w = _waves()
    assert bench.dump_outputs(str(tmp_path), 0, w) == 2
    assert sorted(os.listdir(tmp_path)) == ["audio_r0_000.npy", "audio_r0_002.npy"]   # None: another rank's utterance
    for i in (0, 2):
        a = np.load(tmp_path / f"audio_r0_{i:03d}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, w[i])


def test_dump_outputs_sampled_above_cap(tmp_path):
    w = _waves()
    cap = (w[0].nbytes + w[2].nbytes) // 4
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 1, w, cap=cap)
    total = 0
    for i in (0, 2):
        a = np.load(tmp_path / "a" / f"audio_r1_{i:03d}.npy")
        assert a.dtype == np.float32 and a.size == w[i].size // 4
        assert np.array_equal(a, np.load(tmp_path / "b" / f"audio_r1_{i:03d}.npy"))   # the same sample every run
        assert np.isin(a, w[i]).all()
        total += a.nbytes
    assert total <= cap


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(gpu, tiny_dir, tmp_path):
    """A plain `bench.py` run on the tiny model: the line carries ms_per_step
    and none of --full's measurements, and the dumped waveform is the last
    timed step's, identical from run to run."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--preset", "tiny",
                            "--frames", "4", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "first_packet_ms" not in line and "roofline" not in line and line["cpu_baseline"] is None
        assert os.listdir(tmp_path / d) == ["audio_r0_000.npy"]
        outs.append(np.load(tmp_path / d / "audio_r0_000.npy"))
    assert outs[0].dtype == np.float32 and outs[0].shape == (4 * 1920,)
    assert np.array_equal(outs[0], outs[1])
