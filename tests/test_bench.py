"""bench.py's plain run: the headline line alone (the other legs and figures come with --full), and --dump-outputs writing
what the last timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BYTES = 3 * (8 << 20) + 12345          # three blocks and a ragged fourth: both samples are drawn, not complete
NAMES = ("compressed_lengths", "decoded_lengths", "compressed_sample", "decoded_sample")


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MINLZ_BENCH_ONE_GPU", "MINLZ_BENCH_FORCE_DIST")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--bytes", str(BYTES),
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return line, {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


def test_plain_run_dumps_the_last_step(tmp_path):
    import bench
    from minlz_amd import synth
    d, a = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "MB/s" and d["dtype"] == "u8"
    assert d["roofline"] is None and d["cpu_baseline"] is None and "kernel_ms" not in d["config"] and "legs" in d["config"]
    blk = [min(bench.BLOCK, BYTES - o) for o in range(0, BYTES, bench.BLOCK)]
    assert a["compressed_lengths"].dtype == np.float64 and a["decoded_lengths"].dtype == np.float64
    assert a["compressed_sample"].dtype == np.float32 and a["decoded_sample"].dtype == np.float32
    assert a["decoded_lengths"].tolist() == blk
    clen = a["compressed_lengths"]
    assert (clen > 0).all() and (clen <= np.array(blk) + 64).all()
    assert round(clen.sum() / BYTES, 4) == d["config"]["ratio"]
    assert a["compressed_sample"].size == a["decoded_sample"].size == bench.DUMP_SAMPLE
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    # the decoded sample is the input at the same seeded positions
    src = synth.enwik_like(BYTES, seed=1)
    assert np.array_equal(a["decoded_sample"], src[bench._sample_positions(BYTES, seed=2)].astype(np.float32))
    # same arguments, same inputs, same outputs
    _, b = _bench(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
