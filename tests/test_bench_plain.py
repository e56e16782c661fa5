"""bench.py without --full: the headline alone -- set-up, W + K steps, --dump-outputs and the line -- and none of the measurements
and checks that --full adds after the timed region (tests/test_multi_rank_gpu.py runs those)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_is_the_headline_alone(tmp_path):
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(dump)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("decoded Vorbis")
    c = d["config"]
    assert abs(d["value"] - 4096 * c["passes_per_step"] * 3 / c["timed_region_s"]) < 1e-6 * d["value"]
    assert abs(d["ms_per_step"] - c["timed_region_s"] / 3 * 1e3) < 1e-6 * d["ms_per_step"]
    assert not set(d) & {"kernels_ms", "pipeline_ms_events", "roofline", "pcm_digest_ok", "c5", "configs", "end_to_end", "cpu_baseline"}
    # the dump is there as without --full: every resident batch of the three decoder instances, decoded PCM
    files = sorted(os.listdir(dump))
    assert len(files) == c["passes_per_step"] and all(f.startswith("pcm_stream") and f.endswith(".npy") for f in files)
    for f in files:
        a = np.load(dump / f)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all() and np.abs(a).max() > 0
