#!/usr/bin/env python3
"""Times the interpolating complex-tap FIR (fir_cplx_interp_rows_dev) against what a caller had to do
without it.

The legs alternate window by window inside one process, on the same seeded device-resident inputs,
HIP events around each window, after a warm-up:

    a  fir_cplx_interp_rows_dev                                        (this feature)
    b  fir_cplx_rows_dev alone on an already stuffed tensor            (full rate, stuffing not counted)
    c  torch.zeros + strided copy of x into it, then leg b             (what a caller does today)
    r  fir_interp_rows_dev, the real interpolator, int16 -> int32 of one channel over the same input
       and output bytes (2 N samples, the same U and tap count): the yardstick for the share of peak

Before any timing leg a is checked bit-equal to leg c, and its route must be the fast kernel.  Per
shape the tool records the times and their spread over the windows, the algorithmic bytes
((4 + 8 U) per input frame) of leg a, the share of the 8 TB/s HBM peak they amount to next to leg r's
share for the same bytes in the same run, and which bound holds for leg a at the peak rates: memory,
or VALU at 2 * U * NP v_dot2 per input frame (NP: the window bucket, so U * NP the padded taps)
against one v_dot2 per lane and clock (256 CUs x 4 SIMD x 32 lanes x 2.4 GHz).

    python tools/cinterp_rate.py --out profiles/cinterp [--windows 10] [--per 5] [--only NAME]

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
# name, rows, width (input frames), L, U
SHAPES = [
    ("c16_2p26_L10_U2", 1, 1 << 26, 10, 2),
    ("c16_2p26_L20_U4", 1, 1 << 26, 20, 4),
    ("c16_2p26_L40_U8", 1, 1 << 26, 40, 8),
    ("c16_2p25_L64_U4", 1, 1 << 25, 64, 4),
    ("c16_2p25_L128_U8", 1, 1 << 25, 128, 8),
    ("c16_2p25_L16_U16", 1, 1 << 25, 16, 16),
    ("c16_16384x4096_L32_U2", 16384, 4096, 32, 2),
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

    from fir_hip import cinterp, torch_cinterp, torch_cplx, torch_interp

    if not torch.cuda.is_available():
        sys.exit("cinterp_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261021)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "shapes": {}}
    for name, rows, width, L, U in SHAPES:
        if a.only and a.only != name:
            continue
        h = rng.integers(-1500, 1501, (L, 2))
        hq = torch_cplx.CplxTaps(h)
        hr = h[:, 0].copy()
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.randint(-32768, 32768, (rows, 2 * width), dtype=torch.int16, device=dev, generator=gen)
        ow = cinterp.out_width(width, U)
        ya = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        yb = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        xs = torch.zeros((rows, ow, 2), dtype=torch.int16, device=dev)  # leg b's input: stuffed once, outside the timing
        xs[:, ::U] = x.view(rows, width, 2)

        def leg_a():
            torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(x, hq, U, out=ya)

        def leg_b():
            torch_cplx.fir1d_fixed_rows_cplx_dev(xs.view(rows, 2 * ow), hq, out=yb)

        def leg_c():
            s = torch.zeros((rows, ow, 2), dtype=torch.int16, device=dev)
            s[:, ::U] = x.view(rows, width, 2)
            torch_cplx.fir1d_fixed_rows_cplx_dev(s.view(rows, 2 * ow), hq, out=yb)

        def leg_r():  # 2 N real samples: the same 4 N bytes in and 8 U N bytes out
            torch_interp.fir1d_fixed_rows_interp_dev(x, hr, U, 12, 32, 1, 1, out=ya)

        leg_c()
        leg_a()
        route = cinterp.last_launch()
        if route.route != cinterp.ROUTE_FAST:
            sys.exit(f"cinterp_rate: {name}: route {route}, not the fast kernel")
        torch.cuda.synchronize()
        if not torch.equal(ya, yb):
            sys.exit(f"cinterp_rate: {name}: fir_cplx_interp_rows_dev differs from the full-rate result of the stuffed signal")
        legs = {"a_cplx_interp": leg_a, "b_full_rate_on_stuffed": leg_b, "c_stuff_then_full_rate": leg_c,
                "r_real_interp_same_bytes": leg_r}
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
        n = rows * width  # input frames
        bytes_a = n * (4 + 8 * U)
        bytes_b = n * U * 12
        bytes_c = bytes_b + n * 4 + n * U * 4 * 2  # + the zero fill and the scatter's read and write (at least)
        t_mem = bytes_a / HBM_PEAK_BPS
        dot2 = 2.0 * U * route.window_bucket
        t_valu = n * dot2 / VALU_DOT2_PER_S
        rec = {"rows": rows, "width": width, "taps": L, "up": U, "window_bucket": route.window_bucket,
               "padded_taps": U * route.window_bucket, "bytes_a_in_plus_out": bytes_a, "bytes_b": bytes_b,
               "bytes_c_at_least": bytes_c, "dot2_per_input_frame": dot2, "t_mem_at_peak_us": round(t_mem * 1e6, 2),
               "t_valu_at_peak_us": round(t_valu * 1e6, 2), "bound_at_peak": "memory" if t_mem >= t_valu else "VALU",
               "legs": {}}
        for k, t in times.items():
            med = statistics.median(t)
            b = {"a_cplx_interp": bytes_a, "b_full_rate_on_stuffed": bytes_b, "c_stuff_then_full_rate": bytes_c,
                 "r_real_interp_same_bytes": bytes_a}[k]
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(b / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lc = rec["legs"]["a_cplx_interp"], rec["legs"]["c_stuff_then_full_rate"]
        rec["a_below_c_beyond_spread"] = la["us_max"] < lc["us_min"]
        rec["a_not_above_b"] = la["us_median"] <= rec["legs"]["b_full_rate_on_stuffed"]["us_median"]
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del x, xs, ya, yb
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.name).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
