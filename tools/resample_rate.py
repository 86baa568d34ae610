#!/usr/bin/env python3
"""Times the resampling FIR (fir_resample_rows_dev) against what a caller had to do without it.

Three legs alternate window by window inside one process, on the same seeded device-resident
inputs, HIP events around each window, after a warm-up:

    a  fir_resample_rows_dev                                                     (this feature)
    b  fir_interp_rows_dev into a width * U intermediate, then [..., phase::D].contiguous()
                                                                                 (what a caller does today)
    c  fir_interp_rows_dev alone into that intermediate                          (a lower bound of b)

Before any timing leg a is checked bit-equal to leg b.  Per shape the tool records the three times
and their spread over the windows, the algorithmic bytes (in + out * U / D) * N of leg a, the share
of the 8 TB/s HBM peak they amount to, and which bound holds for leg a at the peak rates: memory, or
VALU at L / (2 U) v_dot2 per output and channel against one v_dot2 per lane and clock (256 CUs x
4 SIMD x 32 lanes x 2.4 GHz).

    python tools/resample_rate.py --out profiles/resample [--windows 10] [--per 5] [--only NAME]

Needs the built library and a GPU only; writes DIR/rate.json and prints it as one JSON line.
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
PHASE = 1
# name, torch dtype name, rows, width (input frames), channels, L, U, D, out stage
SHAPES = [
    ("i16_2p26_L72_3over2", "int16", 1, 1 << 26, 1, 72, 3, 2, "i32"),
    ("i16_2p26_L72_2over3", "int16", 1, 1 << 26, 1, 72, 2, 3, "i32"),
    ("i16_2p26_L192_8over5", "int16", 1, 1 << 26, 1, 192, 8, 5, "i32"),
    ("i16_2p26_L384_16over15", "int16", 1, 1 << 26, 1, 384, 16, 15, "i32"),
    ("i16_2p26_L64_4over6", "int16", 1, 1 << 26, 1, 64, 4, 6, "i32"),
    ("c16_2p25_L64_4over3", "int16", 1, 1 << 25, 2, 64, 4, 3, "i32"),
    ("u8_16384x4096_L15_3over2", "uint8", 16384, 4096, 1, 15, 3, 2, "u8"),
]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, required=True, help="directory for the result file")
    ap.add_argument("--file", default="rate.json", help="name of the result file in --out")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--per", type=int, default=5, help="launches per leg and window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="time one shape by name")
    a = ap.parse_args()

    import torch

    import fir_hip
    from fir_hip import torch_interp, torch_ops, torch_resample

    if not torch.cuda.is_available():
        sys.exit("resample_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261020)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "phase": PHASE, "shapes": {}}
    for name, dt, rows, width, ch, L, U, D, st in SHAPES:
        if a.only and a.only != name:
            continue
        stage = fir_hip.OUT_I32 if st == "i32" else fir_hip.OUT_U8_SAT
        isz, osz = (2 if dt == "int16" else 1), (4 if st == "i32" else 1)
        hq = torch_ops.Taps(rng.integers(-1500, 1501, L))
        gen = torch.Generator(device=dev).manual_seed(7)
        lo, hi = (-32768, 32768) if dt == "int16" else (0, 256)
        tdt, odt = getattr(torch, dt), (torch.int32 if st == "i32" else torch.uint8)
        x = torch.randint(lo, hi, (rows, width * ch), dtype=tdt, device=dev, generator=gen)
        mid = fir_hip.interp_out_width(width, U)
        ow = fir_hip.resample_out_width(width, U, D, PHASE)
        ya = torch.empty((rows, ow * ch), dtype=odt, device=dev)
        ymid = torch.empty((rows, mid * ch), dtype=odt, device=dev)
        kept = {}

        def leg_a():
            torch_resample.fir1d_fixed_rows_resample_dev(x, hq, U, D, PHASE, 12, 32, stage, ch, out=ya)

        def leg_c():
            torch_interp.fir1d_fixed_rows_interp_dev(x, hq, U, 12, 32, stage, ch, out=ymid)

        def leg_b():
            leg_c()
            kept["y"] = ymid.view(rows, mid, ch)[:, PHASE::D].contiguous()

        leg_a()
        leg_b()
        torch.cuda.synchronize()
        if not torch.equal(ya, kept["y"].view(rows, ow * ch)):
            sys.exit(f"resample_rate: {name}: fir_resample_rows_dev differs from the interpolator's output [phase::D]")
        legs = {"a_resample": leg_a, "b_interp_then_gather": leg_b, "c_interp_alone": leg_c}
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
        n = rows * width * ch  # input samples
        n_out = rows * ow * ch
        bytes_a = n * isz + n_out * osz  # (in + out * U / D) * N
        bytes_c = n * isz + n * U * osz
        bytes_b = bytes_c + n * U * osz + n_out * osz  # + the gather's read of every line of the intermediate and its write
        t_mem = bytes_a / HBM_PEAK_BPS
        t_valu = n_out * (L / (2.0 * U)) / VALU_DOT2_PER_S
        rec = {"rows": rows, "width": width, "channels": ch, "taps": L, "up": U, "decim": D, "in": dt, "out": st,
               "out_width": ow, "bytes_a_in_plus_out_U_over_D": bytes_a, "bytes_b_at_least": bytes_b, "bytes_c": bytes_c,
               "dot2_per_output": L / (2.0 * U), "t_mem_at_peak_us": round(t_mem * 1e6, 2),
               "t_valu_at_peak_us": round(t_valu * 1e6, 2), "bound_at_peak": "memory" if t_mem >= t_valu else "VALU",
               "legs": {}}
        for k, t in times.items():
            med = statistics.median(t)
            b = {"a_resample": bytes_a, "b_interp_then_gather": bytes_b, "c_interp_alone": bytes_c}[k]
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(b / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lb, lc = (rec["legs"][k] for k in legs)
        rec["a_below_b_beyond_spread"] = la["us_max"] < lb["us_min"]
        rec["a_not_above_c"] = la["us_median"] <= lc["us_median"]
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del x, ya, ymid, kept
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.file).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
