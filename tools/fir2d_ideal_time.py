#!/usr/bin/env python3
"""Times the float64 ideal 2-D FIR (fir2d_ideal_frames_dev, 3x3 and 5x5) against the 1-D ideal
kernel (fir1d_ideal_rows_dev, 5 taps) on the same 2^28 samples: 4 frames of 8192^2 per launch,
4 rotated HBM-resident input / output sets (9.7 GB, far past the 256 MiB Infinity Cache), HIP
events around each window of launches, the three kernels alternating window by window inside one
process.  All three move the same 9 bytes per sample (1 in + 8 out), so the 1-D kernel is the
yardstick.

    python tools/fir2d_ideal_time.py [--launches 200] [--windows 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fir2d_ideal_time.py --launches 40 --no-check

Prints one JSON line: per kernel the median / min time per launch over the windows, its bytes over
the 8.0 TB/s HBM3E spec peak, and its ratio to the 1-D kernel.  Fails without a GPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "warmup-fir-filter_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

HBM_PEAK_BPS = 8.0e12  # MI355X HBM3E spec peak
FRAMES, H, W, SETS = 4, 8192, 8192, 4


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="timed launches per kernel (split over the windows)")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--no-check", action="store_true", help="skip the band check against the NumPy checker")
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()

    import torch

    from fir_hip import torch_ops

    if not torch.cuda.is_available():
        sys.exit("fir2d_ideal_time: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261019)
    h3, h5, h1 = rng.uniform(-8, 8, (3, 3)), rng.uniform(-8, 8, (5, 5)), rng.uniform(-8, 8, 5)
    gen = torch.Generator(device=dev).manual_seed(7)
    xs = [torch.randint(0, 256, (FRAMES, H, W), dtype=torch.uint8, device=dev, generator=gen) for _ in range(SETS)]
    ys = [torch.empty((FRAMES, H, W), dtype=torch.float64, device=dev) for _ in range(SETS)]
    kernels = {
        "fir2d_ideal_3x3": lambda i: torch_ops.fir2d_ideal_dev(xs[i], h3, out=ys[i]),
        "fir2d_ideal_5x5": lambda i: torch_ops.fir2d_ideal_dev(xs[i], h5, out=ys[i]),
        "fir1d_ideal_5tap": lambda i: torch_ops.fir1d_ideal_rows_dev(xs[i].view(FRAMES * H, W), h1,
                                                                      out=ys[i].view(FRAMES * H, W)),
    }

    if not a.no_check:  # the timed size computes what the checker does: bands across strip seams
        from ideal2d_ref import ideal2d

        for name, h in (("fir2d_ideal_3x3", h3), ("fir2d_ideal_5x5", h5)):
            kernels[name](0)
            torch.cuda.synchronize()
            for f, lo, hi in ((0, 0, 40), (1, 4090, 4130), (FRAMES - 1, H - 40, H)):
                b0, b1 = max(lo - 4, 0), min(hi + 4, H)
                want = ideal2d(xs[0][f, b0:b1].cpu().numpy(), h)[lo - b0:lo - b0 + (hi - lo)]
                if ys[0][f, lo:hi].cpu().numpy().tobytes() != want.tobytes():
                    sys.exit(f"fir2d_ideal_time: {name} differs from the checker in frame {f} rows {lo}-{hi}")

    per = max(1, a.launches // a.windows)
    for fn in kernels.values():
        for i in range(a.warmup):
            fn(i % SETS)
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for _ in range(a.windows):
        for name, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(per):
                fn(i % SETS)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / per)  # us per launch
    nbytes = 9 * FRAMES * H * W
    base = statistics.median(times["fir1d_ideal_5tap"])
    res = {"samples_per_launch": FRAMES * H * W, "bytes_per_launch": nbytes, "launches_per_kernel": per * a.windows,
           "windows": a.windows, "hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "checked": not a.no_check, "kernels": {}}
    for name, t in times.items():
        med = statistics.median(t)
        res["kernels"][name] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                                "TBps": round(nbytes / med / 1e6, 3),
                                "share_of_hbm_peak": round(nbytes / (med * 1e-6) / HBM_PEAK_BPS, 4),
                                "ratio_to_fir1d_ideal": round(med / base, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
