"""bench.py's command line, the parts that need no GPU: the options a plain and a full run take, and
the --dump-outputs writer (float32 .npy, one file per array)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-1000:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def test_dump_outputs_writes_float32_npy(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    c = np.arange(12, dtype=np.float64) / 7
    bench.dump_outputs(str(tmp_path / "d"), {"C": c})
    got = np.load(tmp_path / "d" / "C.npy")
    assert got.dtype == np.float32 and np.array_equal(got, c.astype(np.float32))
