"""A plain ``bench.py`` run on one GPU: the result line carries the headline keys and nothing that ``--full`` adds, ``--steps`` is
the number of timed steps, and ``--dump-outputs`` writes the FLAME codes of the last timed step - here one tiny-config clip whose
reference golden is committed (tests/golden/tiny_4s_s0.npz: seed 0, 4 s, no style).  Run as a child process, as the driver runs
bench.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FLAME_TOL, load_golden

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "tiny", "--batch", "1", "--seconds", "4",
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert abs(r["config"]["frames_per_clip"] / (r["ms_per_step"] * 1e-3) - r["value"]) / r["value"] < 1e-2     # both rounded in the line
    for k in ("cpu_baseline", "synchronous", "host_io", "f32_mode", "heavy_profile", "batch1_latency_ms", "stream_chunk_ms"):
        assert k not in r, f"a plain run measured `{k}` (that belongs behind --full)"
    assert r["budget_ms"] is None and r["parity"] is None
    codes = np.load(out_dir / "flame_codes.npy")
    assert codes.dtype == np.float32 and codes.shape == (1, 100, 106)
    g = load_golden("tiny_4s_s0")
    err = float(np.abs(codes[0] - g["out"]).max())
    assert err < FLAME_TOL, f"dumped codes differ from the reference golden by {err:.3e}"
