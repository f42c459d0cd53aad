"""bench.py argument checks that need no GPU."""
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_refuses_a_run_without_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, (r.returncode, r.stderr[-1000:])
