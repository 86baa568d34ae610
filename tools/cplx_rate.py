#!/usr/bin/env python3
"""Times the complex-tap FIR (fir_cplx_rows_dev) against what a caller had to do without it.

Three legs alternate window by window inside one process, on the same seeded device-resident
inputs, HIP events around each window, after a warm-up:

    a  fir_cplx_rows_dev                                                          (this feature)
    b  two fir1d_fixed_rows_dev calls with channels = 1 on the flattened row, with the real tap sets
       g_re / g_im of 4 * (taps // 2) + 3 taps (below), then the even values of the first and the odd
       values of the second copied into one contiguous (re, im) tensor          (what a caller does today)
    c  fir1d_fixed_rows_dev with channels = 2 and the real taps hr on the same buffers: the same
       bytes and half the MACs, the floor leg a is held against

    g_re[2k] = -hi[k]  g_re[2k+1] = hr[k]      g_im[2k+1] = hr[k]  g_im[2k+2] = hi[k]

Before any timing leg a is checked bit-equal to leg b.  Every leg rotates through the same number
of (x, y) buffer sets, enough of them that one round touches more than the 256 MiB Infinity Cache
(1 GiB or more, at most 8 sets), so no leg is handed its input by the previous launch.  Per shape
the tool records the three times and their spread over the windows, leg a's algorithmic bytes (4 in + 8 out = 12 B per frame), the share of the
8 TB/s HBM peak they amount to, which bound holds for leg a at the peak rates -- memory, or VALU at
2 * taps v_dot2 per frame against one v_dot2 per lane and clock (256 CUs x 4 SIMD x 32 lanes x
2.4 GHz) -- and leg a over leg c.

    python tools/cplx_rate.py --out profiles/cplx [--windows 10] [--per 5] [--only NAME]

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
ROUND_BYTES = 1 << 30      # one round of the buffer sets touches at least this much
MAX_SETS = 8
# name, rows, width (frames), taps, path of leg a
SHAPES = [
    ("c16_2p27_L5", 1, 1 << 27, 5, "fast"),
    ("c16_2p27_L16", 1, 1 << 27, 16, "fast"),
    ("c16_2p27_L64", 1, 1 << 27, 64, "fast"),
    ("c16_16384x4096_L16", 16384, 4096, 16, "fast"),
    ("c16_2p22_L65_generic", 1, 1 << 22, 65, "generic"),
]


def real_tap_sets(hq):
    h = np.asarray(hq, dtype=np.int64)
    L = h.shape[0]
    g_re, g_im = np.zeros(4 * (L // 2) + 3, np.int64), np.zeros(4 * (L // 2) + 3, np.int64)
    g_re[0:2 * L:2], g_re[1:2 * L:2] = -h[:, 1], h[:, 0]
    g_im[1:2 * L:2], g_im[2:2 * L + 1:2] = h[:, 0], h[:, 1]
    return g_re, g_im


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
    from fir_hip import torch_cplx, torch_ops

    if not torch.cuda.is_available():
        sys.exit("cplx_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261020)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "shapes": {}}
    for name, rows, width, L, path in SHAPES:
        if a.only and a.only != name:
            continue
        h = rng.integers(-1500, 1501, (L, 2))
        h[L // 2, 1] = 700  # never all real: leg a must not be the forward
        hq = torch_cplx.CplxTaps(h)
        g_re, g_im = (torch_ops.Taps(g) for g in real_tap_sets(h))
        hr = torch_ops.Taps(h[:, 0])
        n = rows * width
        bytes_a = n * 12
        nsets = max(1, min(MAX_SETS, -(-ROUND_BYTES // bytes_a)))
        gen = torch.Generator(device=dev).manual_seed(7)
        xs = [torch.randint(-32768, 32768, (rows, 2 * width), dtype=torch.int16, device=dev, generator=gen)
              for _ in range(nsets)]
        ys = [torch.empty((rows, 2 * width), dtype=torch.int32, device=dev) for _ in range(nsets)]
        yre = torch.empty((rows, 2 * width), dtype=torch.int32, device=dev)  # leg b's two full-rate results
        yim = torch.empty((rows, 2 * width), dtype=torch.int32, device=dev)
        turn = {"a": 0, "b": 0, "c": 0}

        def pick(leg):
            i = turn[leg] % nsets
            turn[leg] += 1
            return xs[i], ys[i]

        def leg_a():
            x, y = pick("a")
            torch_cplx.fir1d_fixed_rows_cplx_dev(x, hq, 12, 32, fir_hip.OUT_I32, out=y)

        def leg_b():
            x, y = pick("b")
            torch_ops.fir1d_fixed_rows_dev(x, g_re, 12, 32, fir_hip.OUT_I32, 1, out=yre)
            torch_ops.fir1d_fixed_rows_dev(x, g_im, 12, 32, fir_hip.OUT_I32, 1, out=yim)
            y3 = y.view(rows, width, 2)
            y3[..., 0].copy_(yre.view(rows, width, 2)[..., 0])
            y3[..., 1].copy_(yim.view(rows, width, 2)[..., 1])

        def leg_c():
            x, y = pick("c")
            torch_ops.fir1d_fixed_rows_dev(x, hr, 12, 32, fir_hip.OUT_I32, 2, out=y)

        leg_a()  # set 0
        torch.cuda.synchronize()
        got = ys[0].clone()
        ys[0].zero_()
        leg_b()  # set 0 again
        torch.cuda.synchronize()
        if not torch.equal(got, ys[0]):
            sys.exit(f"cplx_rate: {name}: fir_cplx_rows_dev differs from the two real filters' interleaved output")
        del got
        turn.update(a=0, b=0, c=0)
        legs = {"a_cplx": leg_a, "b_two_real_then_interleave": leg_b, "c_real_taps_two_channels": leg_c}
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
        t_mem = bytes_a / HBM_PEAK_BPS
        t_valu = n * 2.0 * L / VALU_DOT2_PER_S
        rec = {"rows": rows, "width_frames": width, "taps": L, "real_taps_of_leg_b": int(len(g_re.h)), "leg_a_path": path,
               "buffer_sets": nsets, "bytes_a_12_per_frame": bytes_a, "dot2_per_frame": 2 * L,
               "t_mem_at_peak_us": round(t_mem * 1e6, 2), "t_valu_at_peak_us": round(t_valu * 1e6, 2),
               "bound_at_peak": "memory" if t_mem >= t_valu else "VALU", "legs": {}}
        for k, t in times.items():
            med = statistics.median(t)
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
        la, lb, lc = (rec["legs"][k] for k in legs)
        la["share_of_hbm_peak"] = round(bytes_a / (la["us_median"] * 1e-6) / HBM_PEAK_BPS, 4)
        lc["share_of_hbm_peak"] = round(bytes_a / (lc["us_median"] * 1e-6) / HBM_PEAK_BPS, 4)
        la["over_valu_bound"] = round(la["us_median"] / (t_valu * 1e6), 3)
        rec["a_below_b_beyond_spread"] = la["us_max"] < lb["us_min"]
        rec["a_over_c"] = round(la["us_median"] / lc["us_median"], 3)
        rec["a_over_b"] = round(la["us_median"] / lb["us_median"], 4)
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del xs, ys, yre, yim
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.file).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
