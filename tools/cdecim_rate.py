#!/usr/bin/env python3
"""Times the decimating complex-tap FIR (fir_cplx_decim_rows_dev) against what a caller had to do
without it.

Three legs alternate window by window inside one process, on the same seeded device-resident
inputs, HIP events around each window, after a warm-up:

    a  fir_cplx_decim_rows_dev                                       (this feature)
    b  fir_cplx_rows_dev alone                                        (full rate, nothing kept back)
    c  leg b, then y.view(rows, width, 2)[:, phase::D].contiguous()   (what a caller does today)

Before any timing leg a is checked bit-equal to leg c, and its route must be the fast kernel.  Per
shape the tool records the three times and their spread over the windows, the algorithmic bytes
(4 + 8 / D per frame) of leg a, the share of the 8 TB/s HBM peak they amount to (next to leg b's
share for its own 12 bytes per frame, same run), and which bound holds for leg a at the peak rates:
memory, or VALU at 2 LP / D v_dot2 per input frame (LP: the tap bucket) against one v_dot2 per lane
and clock (256 CUs x 4 SIMD x 32 lanes x 2.4 GHz).

    python tools/cdecim_rate.py --out profiles/cdecim [--windows 10] [--per 5] [--only NAME]

Needs the built libraries and a GPU only; writes DIR/rate.json and prints it as one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "warmup-fir-filter_amd"):
    sys.path.insert(0, str(p))

HBM_PEAK_BPS = 8.0e12      # the peak the project's other profiles use
VALU_DOT2_PER_S = 256 * 4 * 32 * 2.4e9  # one v_dot2_i32_i16 per lane and clock
# name, rows, width (frames), L, D
SHAPES = [
    ("c16_2p26_L5_D2", 1, 1 << 26, 5, 2),
    ("c16_2p26_L5_D4", 1, 1 << 26, 5, 4),
    ("c16_2p26_L5_D8", 1, 1 << 26, 5, 8),
    ("c16_2p26_L16_D4", 1, 1 << 26, 16, 4),
    ("c16_2p26_L64_D2", 1, 1 << 26, 64, 2),
    ("c16_2p26_L64_D8", 1, 1 << 26, 64, 8),
    ("c16_2p26_L64_D16", 1, 1 << 26, 64, 16),
    ("c16_16384x4096_L16_D4", 16384, 4096, 16, 4),
]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, required=True, help="directory for rate.json")
    ap.add_argument("--name", default="rate.json", help="file name inside --out")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--per", type=int, default=5, help="launches per leg and window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="time one shape by name")
    a = ap.parse_args()

    import torch

    from fir_hip import cdecim, torch_cdecim, torch_cplx

    if not torch.cuda.is_available():
        sys.exit("cdecim_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261021)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "shapes": {}}
    for name, rows, width, L, D in SHAPES:
        if a.only and a.only != name:
            continue
        phase = D - 1
        hq = torch_cplx.CplxTaps(rng.integers(-1500, 1501, (L, 2)))
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.randint(-32768, 32768, (rows, 2 * width), dtype=torch.int16, device=dev, generator=gen)
        ow = cdecim.out_width(width, D, phase)
        ya = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        yb = torch.empty((rows, 2 * width), dtype=torch.int32, device=dev)

        def leg_a():
            torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(x, hq, D, phase, out=ya)

        def leg_b():
            torch_cplx.fir1d_fixed_rows_cplx_dev(x, hq, out=yb)

        def leg_c():
            leg_b()
            return yb.view(rows, width, 2)[:, phase::D].contiguous()

        leg_a()
        route = cdecim.last_launch()
        if route.route != cdecim.ROUTE_FAST:
            sys.exit(f"cdecim_rate: {name}: route {route}, not the fast kernel")
        yc = leg_c()
        torch.cuda.synchronize()
        if not torch.equal(ya.view(rows, ow, 2), yc):
            sys.exit(f"cdecim_rate: {name}: fir_cplx_decim_rows_dev differs from the full-rate result's slice")
        del yc
        legs = {"a_cplx_decim": leg_a, "b_full_rate": leg_b, "c_full_rate_then_gather": leg_c}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.per):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.per)  # us per call
        n = rows * width  # frames
        bytes_a = n * 4 + rows * ow * 8
        bytes_b = n * 12
        bytes_c = bytes_b + n * 8 + rows * ow * 8  # + the gather's strided read (at least) and its write
        t_mem = bytes_a / HBM_PEAK_BPS
        t_valu = n * 2.0 * route.tap_bucket / D / VALU_DOT2_PER_S
        rec = {"rows": rows, "width": width, "taps": L, "tap_bucket": route.tap_bucket, "decim": D, "phase": phase,
               "bytes_a_in_plus_out_over_D": bytes_a, "bytes_b": bytes_b, "bytes_c_at_least": bytes_c,
               "dot2_per_frame": 2.0 * route.tap_bucket / D, "t_mem_at_peak_us": round(t_mem * 1e6, 2),
               "t_valu_at_peak_us": round(t_valu * 1e6, 2), "bound_at_peak": "memory" if t_mem >= t_valu else "VALU",
               "legs": {}}
        for k, t in times.items():
            med = statistics.median(t)
            b = {"a_cplx_decim": bytes_a, "b_full_rate": bytes_b, "c_full_rate_then_gather": bytes_c}[k]
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(b / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lb, lc = (rec["legs"][k] for k in legs)
        rec["a_below_c_beyond_spread"] = la["us_max"] < lc["us_min"]
        rec["a_not_above_b"] = la["us_median"] <= lb["us_median"]
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del x, ya, yb
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.name).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
