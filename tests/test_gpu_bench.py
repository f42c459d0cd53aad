"""bench.py --dump-outputs: what the timed path computed in its last step, written as float32 .npy files from seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench_dump(out_dir, steps, extra=()):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--size", "64",
                        "--batch", "2", "--no-cpu-baseline", "--no-launch-floor", "--no-other-configs", "--dump-outputs", str(out_dir)] + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_dump_outputs_are_reproducible(tmp_path):
    """The full-width male2female model at 64x64, B=2: the dump holds every loss and equally sized seeded samples of the parameters and
    gradients, float32, under 64 MB.  Deterministic mode: a second run with the same arguments writes the same bits.  Default plan: two
    runs agree to rounding."""
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib as L
    sys.path.insert(0, ROOT)
    import bench
    runs = []
    for i, extra in enumerate((["--deterministic"], ["--deterministic"], [], [])):
        out = _bench_dump(tmp_path / str(i), 3, extra)
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["config"]["losses_finite"] is True
        runs.append({f[:-4]: np.load(tmp_path / str(i) / f) for f in sorted(os.listdir(tmp_path / str(i)))})
    a, b, c, d = runs
    assert set(a) == set(L.LOSS_NAMES) | {"params", "grads"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    assert a["params"].shape == a["grads"].shape == (bench.DUMP_SAMPLE,)      # (the full-width networks hold ~55 M parameters)
    assert np.isfinite(a["grads"]).all() and np.abs(a["grads"]).max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the default plan: fp32 atomics reorder sums from run to run, but every step trains from the same state, so two runs agree to rounding
    assert set(c) == set(d) == set(a)
    for k in c:
        assert np.abs(c[k].astype(np.float64) - d[k]).max() <= 1e-3 * max(np.abs(c[k]).max(), 1e-30), k
