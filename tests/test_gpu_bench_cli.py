"""bench.py as a program on the GPU: a plain run times its steps and prints the headline keys
only; --dump-outputs writes what the last timed step computed; --full adds the roofline loop and
the parity check and leaves the dump unchanged.  Small sizes (2^16 samples), one process each."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
LOG2N = 16
FULL_ONLY = ("roofline", "cpu_baseline", "cpu_baseline_numpy", "cpu_baseline_numpy_threads",
             "cpu_baseline_python_loop", "parity", "configs")


def _bench(*argv):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--log2n", str(LOG2N), *argv],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _expected():
    import bench as b
    from oracle import fir_oracle

    x = np.random.default_rng(b.SEED).integers(-32768, 32768, 1 << LOG2N, dtype=np.int16)
    return b, fir_oracle.fir1d_i16_i32(x, b.SHARPEN5)


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    b, ref = _expected()
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert rec["metric"] == b.METRIC and rec["unit"] == "Gsamples/s" and rec["higher_is_better"] is True
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["dtype"].startswith("int32")
    assert rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps (both are rounded in the line)
    assert abs(rec["value"] - (1 << LOG2N) / (rec["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * rec["value"] + 1e-3
    assert not [k for k in FULL_ONLY if k in rec]
    assert [p.name for p in (tmp_path / "out").iterdir()] == ["y.npy"]
    y = np.load(tmp_path / "out" / "y.npy")
    assert y.dtype == np.float64 and np.array_equal(y, ref.astype(np.float64))


def test_full_run_adds_its_keys_and_the_same_dump(tmp_path):
    _, ref = _expected()
    rec = _bench("--full", "--steps", "3", "--warmup", "1", "--cpu-seconds", "0", "--no-configs",
                 "--roofline-launches", "5", "--roofline-ramp", "0", "--dump-outputs", str(tmp_path / "out"))
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["parity"].startswith("bit-exact") and rec["roofline"]["kernel_avg_us"] > 0
    assert np.array_equal(np.load(tmp_path / "out" / "y.npy"), ref.astype(np.float64))
