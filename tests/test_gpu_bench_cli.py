"""GPU: bench.py's command line -- a plain run prints only the headline line
and, with --dump-outputs, writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_line_and_dump(tmp_path):
    """--steps sets the timed steps, the line carries ms_per_step and none of
    the --full measurements, and the dump holds the last step's slot
    (steps 5, 8 slots -> slot 4) of the config-2 box QP: float64, every
    instance optimal, |u| <= 1, and z not the same for every instance."""
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5",
                        "--warmup", "1", "--batch", "300", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 5 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(300 * 1e3 / res["ms_per_step"], rel=1e-2)
    assert res["unit"] == "solves/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    for k in ("max_abs_u_err_vs_oracle", "roofline", "cpu_baseline", "host_roundtrip", "kernel_us"):
        assert k not in res
    assert sorted(os.listdir(d)) == ["status.npy", "status_iters.npy", "z.npy"]
    z, st = np.load(os.path.join(d, "z.npy")), np.load(os.path.join(d, "status.npy"))
    assert z.dtype == np.float64 and z.shape == (300, 20) and st.shape == (300,)
    assert (st == 0).all()
    assert np.abs(z).max() <= 1.0 + 1e-12
    assert np.unique(z.round(9), axis=0).shape[0] > 1
    # the same slot through the C oracle (bench.py Config2's plant and x0 seed;
    # 1e-9 as in smoke(): fp64 on both sides, a well-conditioned 20-variable QP)
    from oracle import cbaseline as cbl

    ts = 0.5
    A, B = np.array([[1.0, ts], [0.0, 1.0]]), np.array([[0.0], [-ts]])
    C = np.array([[1.0], [-2.0 / 3.0]])
    Q = C @ C.T + 1e-3 * np.eye(2)
    x0 = np.random.default_rng(20261015 + 2).uniform(-10.0, 10.0, size=(8, 300, 2))[4]
    zr, _ = cbl.mpc_box(A, B, Q, np.array([[0.1]]), Q, 20, x0, -1.0, 1.0, nthreads=1)
    assert np.abs(z - zr).max() < 1e-9
