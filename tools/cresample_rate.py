#!/usr/bin/env python3
"""Times the rational resampling complex-tap FIR (fir_cplx_resample_rows_dev) against what a caller
had to do without it.

The legs alternate window by window inside one process, on the same seeded device-resident inputs,
HIP events around each window, after a warm-up:

    a  fir_cplx_resample_rows_dev                                              (this feature)
    b  fir_cplx_interp_rows_dev into a width * U intermediate, then
       [..., phase::D, :].contiguous()                                         (what a caller does today)
    c  the interpolator alone
    r  fir_resample_rows_dev, the real resampler, int16 -> int32 of one channel over the same input
       and output bytes (2 N samples, the same U, D and tap count): the yardstick for the share of peak

Before any timing leg a is checked bit-equal to leg b, and its route must be the fast kernel.  Per
shape the tool records the times and their spread over the windows, the algorithmic bytes
((4 + 8 U / D) per input frame) of leg a, the share of the 8 TB/s HBM peak they amount to next to leg
r's share for the same bytes in the same run, and which bound holds for leg a at the peak rates:
memory, or VALU at 2 * NP v_dot2 per output frame (NP: the tap bucket) against one v_dot2 per lane and
clock (256 CUs x 4 SIMD x 32 lanes x 2.4 GHz).

    python tools/cresample_rate.py --out profiles/cresample [--windows 10] [--per 5] [--only NAME]

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
# name, rows, width (input frames), L, U, D, phase
SHAPES = [
    ("c16_2p26_L72_U3_D2", 1, 1 << 26, 72, 3, 2, 1),
    ("c16_2p26_L64_U2_D3", 1, 1 << 26, 64, 2, 3, 1),
    ("c16_2p26_L64_U4_D6", 1, 1 << 26, 64, 4, 6, 1),
    ("c16_2p25_L64_U4_D3", 1, 1 << 25, 64, 4, 3, 1),
    ("c16_2p25_L128_U8_D5", 1, 1 << 25, 128, 8, 5, 1),
    ("c16_2p25_L128_U16_D15", 1, 1 << 25, 128, 16, 15, 1),
    ("c16_16384x4096_L32_U3_D2", 16384, 4096, 32, 3, 2, 1),
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

    import fir_hip
    from fir_hip import cresample, torch_cinterp, torch_cplx, torch_cresample, torch_resample

    if not torch.cuda.is_available():
        sys.exit("cresample_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261021)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "shapes": {}}
    for name, rows, width, L, U, D, phase in SHAPES:
        if a.only and a.only != name:
            continue
        h = rng.integers(-1500, 1501, (L, 2))
        hq = torch_cplx.CplxTaps(h)
        hr = h[:, 0].copy()
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.randint(-32768, 32768, (rows, 2 * width), dtype=torch.int16, device=dev, generator=gen)
        ow = cresample.out_width(width, U, D, phase)
        ya = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        mid = torch.empty((rows, 2 * width * U), dtype=torch.int32, device=dev)  # legs b and c: the intermediate
        # leg r's output: the real resampler's row of 2 * width samples
        yr = torch.empty((rows, fir_hip.resample_out_width(2 * width, U, D, phase)), dtype=torch.int32, device=dev)
        kept = {}

        def leg_a():
            torch_cresample.fir1d_fixed_rows_cplx_resample_dev(x, hq, U, D, phase, out=ya)

        def leg_b():
            torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(x, hq, U, out=mid)
            kept["y"] = mid.view(rows, width * U, 2)[:, phase::D, :].contiguous()

        def leg_c():
            torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(x, hq, U, out=mid)

        def leg_r():  # 2 N real samples: the same 4 N bytes in and (within one sample a row) 8 N U / D bytes out
            torch_resample.fir1d_fixed_rows_resample_dev(x, hr, U, D, phase, 12, 32, 1, 1, out=yr)

        leg_b()
        leg_a()
        route = cresample.last_launch()
        if route.route != cresample.ROUTE_FAST:
            sys.exit(f"cresample_rate: {name}: route {route}, not the fast kernel")
        torch.cuda.synchronize()
        if not torch.equal(ya.view(rows, ow, 2), kept["y"]):
            sys.exit(f"cresample_rate: {name}: fir_cplx_resample_rows_dev differs from the interpolator's sliced result")
        legs = {"a_cplx_resample": leg_a, "b_interp_then_slice": leg_b, "c_interp_alone": leg_c, "r_real_resample_same_bytes": leg_r}
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
        n_out = rows * ow
        bytes_a = n * 4 + n_out * 8
        bytes_c = n * 4 + n * U * 8
        bytes_b = bytes_c + 2 * n_out * 8  # + the gather's read (at least the kept frames) and its write
        t_mem = bytes_a / HBM_PEAK_BPS
        dot2 = 2.0 * route.tap_bucket
        t_valu = n_out * dot2 / VALU_DOT2_PER_S
        rec = {"rows": rows, "width": width, "taps": L, "up": U, "decim": D, "phase": phase, "out_width": ow,
               "tap_bucket": route.tap_bucket, "bytes_a_in_plus_out": bytes_a, "bytes_b_at_least": bytes_b, "bytes_c": bytes_c,
               "dot2_per_output_frame": dot2, "t_mem_at_peak_us": round(t_mem * 1e6, 2),
               "t_valu_at_peak_us": round(t_valu * 1e6, 2), "bound_at_peak": "memory" if t_mem >= t_valu else "VALU",
               "legs": {}}
        for k, t in times.items():
            med = statistics.median(t)
            b = {"a_cplx_resample": bytes_a, "b_interp_then_slice": bytes_b, "c_interp_alone": bytes_c,
                 "r_real_resample_same_bytes": bytes_a}[k]
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(b / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lb = rec["legs"]["a_cplx_resample"], rec["legs"]["b_interp_then_slice"]
        rec["a_below_b_beyond_spread"] = la["us_max"] < lb["us_min"]
        rec["b_over_a"] = round(lb["us_median"] / la["us_median"], 2)
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del x, ya, mid, yr
        kept.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.name).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
