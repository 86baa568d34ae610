#!/usr/bin/env python3
"""Times the interpolating FIR (fir_interp_rows_dev) against what a caller had to do without it.

Three legs alternate window by window inside one process, on the same seeded device-resident
inputs, HIP events around each window, after a warm-up:

    a  fir_interp_rows_dev                                              (this feature)
    b  fir1d_fixed_rows_dev alone on an already zero-stuffed tensor     (full rate at the output rate)
    c  torch.zeros + a strided copy of x into it, then leg b on it      (what a caller does today)

Before any timing leg a is checked bit-equal to leg c.  Per shape the tool records the three times
and their spread over the windows, the algorithmic bytes (in + U * out) * N of leg a, the share of
the 8 TB/s HBM peak they amount to (next to leg b's share for its own (in + out) * N * U bytes,
same run), and which bound holds for leg a at the peak rates: memory, or VALU at L / (2 U) v_dot2
per output and channel against one v_dot2 per lane and clock (256 CUs x 4 SIMD x 32 lanes x 2.4 GHz).

    python tools/interp_rate.py --out profiles/interp [--windows 10] [--per 5] [--only NAME]

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
# name, torch dtype name, rows, width (input frames), channels, L, U, out stage
SHAPES = [
    ("i16_2p26_L10_U2", "int16", 1, 1 << 26, 1, 10, 2, "i32"),
    ("i16_2p26_L20_U4", "int16", 1, 1 << 26, 1, 20, 4, "i32"),
    ("i16_2p26_L40_U8", "int16", 1, 1 << 26, 1, 40, 8, "i32"),
    ("i16_2p26_L64_U4", "int16", 1, 1 << 26, 1, 64, 4, "i32"),
    ("c16_2p25_L64_U4", "int16", 1, 1 << 25, 2, 64, 4, "i32"),
    ("u8_16384x4096_L10_U2", "uint8", 16384, 4096, 1, 10, 2, "u8"),
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
    from fir_hip import torch_interp, torch_ops

    if not torch.cuda.is_available():
        sys.exit("interp_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261020)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "shapes": {}}
    for name, dt, rows, width, ch, L, U, st in SHAPES:
        if a.only and a.only != name:
            continue
        stage = fir_hip.OUT_I32 if st == "i32" else fir_hip.OUT_U8_SAT
        isz, osz = (2 if dt == "int16" else 1), (4 if st == "i32" else 1)
        hq = torch_ops.Taps(rng.integers(-1500, 1501, L))
        gen = torch.Generator(device=dev).manual_seed(7)
        lo, hi = (-32768, 32768) if dt == "int16" else (0, 256)
        tdt, odt = getattr(torch, dt), (torch.int32 if st == "i32" else torch.uint8)
        x = torch.randint(lo, hi, (rows, width * ch), dtype=tdt, device=dev, generator=gen)
        ow = fir_hip.interp_out_width(width, U)
        ya = torch.empty((rows, ow * ch), dtype=odt, device=dev)
        yb = torch.empty((rows, ow * ch), dtype=odt, device=dev)

        def stuff():
            xu = torch.zeros((rows, ow, ch), dtype=tdt, device=dev)
            xu[:, ::U] = x.view(rows, width, ch)
            return xu.view(rows, ow * ch)

        xs = stuff()  # leg b's input: stuffed once, outside the timing

        def leg_a():
            torch_interp.fir1d_fixed_rows_interp_dev(x, hq, U, 12, 32, stage, ch, out=ya)

        def leg_b():
            torch_ops.fir1d_fixed_rows_dev(xs, hq, 12, 32, stage, ch, out=yb)

        def leg_c():
            torch_ops.fir1d_fixed_rows_dev(stuff(), hq, 12, 32, stage, ch, out=yb)

        leg_a()
        leg_c()
        torch.cuda.synchronize()
        if not torch.equal(ya, yb):
            sys.exit(f"interp_rate: {name}: fir_interp_rows_dev differs from the full-rate result of the stuffed signal")
        legs = {"a_interp": leg_a, "b_full_rate_on_stuffed": leg_b, "c_stuff_then_full_rate": leg_c}
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
        bytes_a = n * (isz + U * osz)
        bytes_b = n * U * (isz + osz)
        bytes_c = bytes_b + n * isz + 2 * n * U * isz  # + the zero fill, the read of x and its strided write (at least)
        t_mem = bytes_a / HBM_PEAK_BPS
        t_valu = n * U * (L / (2.0 * U)) / VALU_DOT2_PER_S
        rec = {"rows": rows, "width": width, "channels": ch, "taps": L, "up": U, "in": dt, "out": st,
               "bytes_a_in_plus_U_out": bytes_a, "bytes_b": bytes_b, "bytes_c_at_least": bytes_c,
               "dot2_per_output": L / (2.0 * U), "t_mem_at_peak_us": round(t_mem * 1e6, 2),
               "t_valu_at_peak_us": round(t_valu * 1e6, 2), "bound_at_peak": "memory" if t_mem >= t_valu else "VALU",
               "legs": {}}
        for k, t in times.items():
            med = statistics.median(t)
            b = {"a_interp": bytes_a, "b_full_rate_on_stuffed": bytes_b, "c_stuff_then_full_rate": bytes_c}[k]
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(b / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lb, lc = (rec["legs"][k] for k in legs)
        rec["a_below_c_beyond_spread"] = la["us_max"] < lc["us_min"]
        rec["a_not_above_b"] = la["us_median"] <= lb["us_median"]
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del x, xs, ya, yb
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.file).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
