#!/usr/bin/env python3
"""Times one block of the streaming decimating complex-tap FIR (fir_cplx_stream_block_dev) against the
one-shot decimator on the same block and against what a caller had to do without it.

Four legs alternate window by window inside one process, on the same seeded device-resident inputs,
HIP events around each window, after a warm-up, in steady state (a hostile, non-zero history that
ping-pongs between two buffers):

    a  fir_cplx_stream_block_dev: the FIR kernel and the history kernel        (this feature)
    b  fir_cplx_decim_rows_dev on the same x                                    (the floor: no history)
    c  what a caller does today: Z = torch.cat([hist, x], -1); the one-shot decimator over Z with
       phase' = (phase + H - c) mod D; drop the first (phase + H - c) // D kept frames, truncate to
       out_width, .contiguous(); hist = Z[..., -2H:].clone()
    h  the history kernel alone: the same entry with decim = width + 1 and phase = width, which
       keeps no frame, so only the history is written (from the same x and history)

Before any timing leg a is checked bit-equal to leg c (y and the next history), and its route must be
the fast kernel.  Per shape the tool records the four times with their spread over the windows,
a - b next to h, leg a's slowest window against b's slowest + h's slowest (b's own spread is the
noise that comparison is read against), the algorithmic bytes of leg a (4 + 8 / D per frame, plus
rows * H * 8 of history read and written) and the share of the 8 TB/s HBM peak they amount to.

    python tools/cstream_rate.py --out profiles/cstream [--windows 10] [--per 5] [--only NAME]

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
    ("c16_1x2p26_L5_D2", 1, 1 << 26, 5, 2),
    ("c16_1x2p24_L64_D8", 1, 1 << 24, 64, 8),
    ("c16_64x2p16_L64_D8", 64, 1 << 16, 64, 8),   # a 64-channel receiver's block
    ("c16_64x4096_L16_D4", 64, 4096, 16, 4),      # a small block, where the launches show
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

    from fir_hip import cdecim, cstream, torch_cdecim, torch_cplx, torch_cstream

    if not torch.cuda.is_available():
        sys.exit("cstream_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261021)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "valu_dot2_per_s": VALU_DOT2_PER_S, "windows": a.windows,
           "launches_per_window": a.per, "shapes": {}}
    for name, rows, width, L, D in SHAPES:
        if a.only and a.only != name:
            continue
        phase, H, c = D - 1, L - 1, L // 2
        hq = torch_cplx.CplxTaps(rng.integers(-1500, 1501, (L, 2)))
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.randint(-32768, 32768, (rows, 2 * width), dtype=torch.int16, device=dev, generator=gen)
        hist0 = torch.randint(-32768, 32768, (rows, 2 * H), dtype=torch.int16, device=dev, generator=gen)
        ow = cstream.out_width(width, D, phase)
        skip, phase_c = divmod(phase + H - c, D)
        ya = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        yb = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        yh = torch.empty((rows, 0), dtype=torch.int32, device=dev)
        hists = [hist0.clone(), torch.empty_like(hist0)]  # leg a's and leg h's ping-pong pair
        state = {"a": 0, "h": 0, "c": hist0.clone()}

        def leg_a():
            k = state["a"]
            torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(x, hists[k], hists[1 - k], hq, D, phase, out=ya)
            state["a"] = 1 - k

        def leg_b():
            torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(x, hq, D, phase, out=yb)

        def leg_c():
            z = torch.cat([state["c"], x], -1)
            full = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(z, hq, D, phase_c)
            y = full.view(rows, -1, 2)[:, skip:skip + ow].contiguous()
            state["c"] = z[..., z.shape[-1] - 2 * H:].clone()
            return y

        def leg_h():
            k = state["h"]
            torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(x, hists[k], hists[1 - k], hq, width + 1, width, out=yh)
            state["h"] = 1 - k

        leg_a()
        route = cstream.last_launch()
        if route.route != cstream.ROUTE_FAST:
            sys.exit(f"cstream_rate: {name}: route {route}, not the fast kernel")
        yc = leg_c()
        torch.cuda.synchronize()
        if not torch.equal(ya.view(rows, ow, 2), yc) or not torch.equal(hists[1], state["c"]):
            sys.exit(f"cstream_rate: {name}: the stream block differs from cat + the one-shot decimator + slice")
        del yc
        leg_h()
        if cstream.last_launch().route != cstream.ROUTE_NONE:
            sys.exit(f"cstream_rate: {name}: the history-only call launched a FIR kernel")
        leg_b()
        if cdecim.last_launch().route != cdecim.ROUTE_FAST:
            sys.exit(f"cstream_rate: {name}: the one-shot decimator is not on its fast kernel")
        legs = {"a_stream_block": leg_a, "b_one_shot_decim": leg_b, "c_cat_decim_slice_clone": leg_c, "h_history_only": leg_h}
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
        bytes_hist = rows * H * 8  # read and written, 4 bytes a frame each
        bytes_a = n * 4 + rows * ow * 8 + bytes_hist
        bytes_b = n * 4 + rows * ow * 8
        bytes_c = 3 * n * 4 + 3 * rows * ow * 8  # the cat's read and write, the decimator, the slice's read and write, at least
        t_mem = bytes_a / HBM_PEAK_BPS
        t_valu = n * 2.0 * route.tap_bucket / D / VALU_DOT2_PER_S
        rec = {"rows": rows, "width": width, "taps": L, "tap_bucket": route.tap_bucket, "decim": D, "phase": phase,
               "bytes_a_in_plus_out_over_D_plus_history": bytes_a, "bytes_history": bytes_hist, "bytes_b": bytes_b,
               "bytes_c_at_least": bytes_c, "dot2_per_frame": 2.0 * route.tap_bucket / D,
               "t_mem_at_peak_us": round(t_mem * 1e6, 2), "t_valu_at_peak_us": round(t_valu * 1e6, 2),
               "bound_at_peak": "memory" if t_mem >= t_valu else "VALU", "legs": {}}
        nbytes = {"a_stream_block": bytes_a, "b_one_shot_decim": bytes_b, "c_cat_decim_slice_clone": bytes_c,
                  "h_history_only": bytes_hist}
        for k, t in times.items():
            med = statistics.median(t)
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(nbytes[k] / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lb, lc, lh = (rec["legs"][k] for k in legs)
        rec["a_slowest_below_c_fastest"] = la["us_max"] < lc["us_min"]
        rec["a_minus_b_us_median"] = round(la["us_median"] - lb["us_median"], 2)
        rec["h_us_median"] = lh["us_median"]
        rec["a_slowest_us"] = la["us_max"]
        rec["b_slowest_plus_h_slowest_us"] = round(lb["us_max"] + lh["us_max"], 2)
        rec["b_spread_us"] = round(lb["us_max"] - lb["us_min"], 2)
        rec["a_slowest_not_above_b_plus_h"] = la["us_max"] <= lb["us_max"] + lh["us_max"]
        res["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), file=sys.stderr, flush=True)
        del x, ya, yb, hists, hist0
        state.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    a.out.mkdir(parents=True, exist_ok=True)
    (a.out / a.name).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
