#!/usr/bin/env python3
"""Times one block of the streaming U/D resampling complex-tap FIR (fir_cplx_rstream_block_dev) against
the one-shot resampler on the same block and against what a caller had to do without it.

Four legs alternate window by window inside one process, on the same seeded device-resident inputs,
HIP events around each window, after a warm-up, in steady state (a hostile, non-zero history that
ping-pongs between two buffers):

    a  fir_cplx_rstream_block_dev: the FIR kernel and the history kernel       (this feature)
    b  fir_cplx_resample_rows_dev on the same x                                 (the floor: no history)
    c  what a caller does today: Z = torch.cat([one zero frame, hist, x], -1); the one-shot resampler
       over Z with phase' = first mod D, first = phase + (H + 1) U - taps // 2; drop the first
       first // D kept frames, truncate to out_width, .contiguous(); hist = Z[..., -2H:].clone()
    h  the history kernel alone: the same entry with decim = width * U + 1 and phase = width * U,
       which keeps no frame, so only the history is written (from the same x and history)

Before any timing leg a is checked bit-equal to leg c (y and the next history), and its route must be
the fast kernel.  Per shape the tool records the four times with their spread over the windows,
whether a's slowest window is below c's fastest, a - b next to h and b's own spread (the noise that
comparison is read against), the algorithmic bytes of leg a (4 per input frame, 8 per output frame,
plus rows * H * 8 of history read and written) and the share of the 8 TB/s HBM peak they amount to.

    python tools/crstream_rate.py --out profiles/crstream [--windows 10] [--per 5] [--only NAME]

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
# name, rows, width (frames), L, U, D
SHAPES = [
    ("c16_1x2p26_L72_3_2", 1, 1 << 26, 72, 3, 2),
    ("c16_1x2p25_L64_4_3", 1, 1 << 25, 64, 4, 3),
    ("c16_64x2p16_L64_4_3", 64, 1 << 16, 64, 4, 3),   # a 64-channel receiver's block
    ("c16_64x4096_L32_3_2", 64, 4096, 32, 3, 2),      # a small block, where the launches show
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

    from fir_hip import cresample, crstream, torch_cplx, torch_cresample, torch_crstream

    if not torch.cuda.is_available():
        sys.exit("crstream_rate: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20261021)
    res = {"hbm_peak_TBps": HBM_PEAK_BPS / 1e12, "windows": a.windows, "launches_per_window": a.per, "shapes": {}}
    for name, rows, width, L, U, D in SHAPES:
        if a.only and a.only != name:
            continue
        phase, H = D - 1, crstream.hist_frames(L, U)
        hq = torch_cplx.CplxTaps(rng.integers(-1500, 1501, (L, 2)))
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.randint(-32768, 32768, (rows, 2 * width), dtype=torch.int16, device=dev, generator=gen)
        hist0 = torch.randint(-32768, 32768, (rows, 2 * H), dtype=torch.int16, device=dev, generator=gen)
        zero = torch.zeros((rows, 2), dtype=torch.int16, device=dev)
        ow = crstream.out_width(width, U, D, phase)
        skip, phase_c = divmod(phase + (H + 1) * U - L // 2, D)
        ya = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        yb = torch.empty((rows, 2 * ow), dtype=torch.int32, device=dev)
        yh = torch.empty((rows, 0), dtype=torch.int32, device=dev)
        hists = [hist0.clone(), torch.empty_like(hist0)]  # leg a's and leg h's ping-pong pair
        state = {"a": 0, "h": 0, "c": hist0.clone()}

        def leg_a():
            k = state["a"]
            torch_crstream.fir1d_fixed_rows_cplx_resample_block_dev(x, hists[k], hists[1 - k], hq, U, D, phase, out=ya)
            state["a"] = 1 - k

        def leg_b():
            torch_cresample.fir1d_fixed_rows_cplx_resample_dev(x, hq, U, D, phase, out=yb)

        def leg_c():
            z = torch.cat([zero, state["c"], x], -1)
            full = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(z, hq, U, D, phase_c)
            y = full.view(rows, -1, 2)[:, skip:skip + ow].contiguous()
            state["c"] = z[..., z.shape[-1] - 2 * H:].clone()
            return y

        def leg_h():
            k = state["h"]
            torch_crstream.fir1d_fixed_rows_cplx_resample_block_dev(x, hists[k], hists[1 - k], hq, U, width * U + 1,
                                                                    width * U, out=yh)
            state["h"] = 1 - k

        leg_a()
        route = crstream.last_launch()
        if route.route != crstream.ROUTE_FAST:
            sys.exit(f"crstream_rate: {name}: route {route}, not the fast kernel")
        yc = leg_c()
        torch.cuda.synchronize()
        if not torch.equal(ya.view(rows, ow, 2), yc) or not torch.equal(hists[1], state["c"]):
            sys.exit(f"crstream_rate: {name}: the stream block differs from cat + the one-shot resampler + slice")
        del yc
        leg_h()
        if crstream.last_launch().route != crstream.ROUTE_NONE:
            sys.exit(f"crstream_rate: {name}: the history-only call launched a FIR kernel")
        leg_b()
        if cresample.last_launch().route != cresample.ROUTE_FAST:
            sys.exit(f"crstream_rate: {name}: the one-shot resampler is not on its fast kernel")
        legs = {"a_stream_block": leg_a, "b_one_shot_resample": leg_b, "c_cat_resample_slice_clone": leg_c,
                "h_history_only": leg_h}
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
        bytes_c = 3 * n * 4 + 3 * rows * ow * 8  # the cat's read and write, the resampler, the slice's read and write, at least
        rec = {"rows": rows, "width": width, "taps": L, "tap_bucket": route.tap_bucket, "up": U, "decim": D, "phase": phase,
               "hist_frames": H, "bytes_a_in_plus_out_plus_history": bytes_a, "bytes_history": bytes_hist, "bytes_b": bytes_b,
               "bytes_c_at_least": bytes_c, "t_mem_at_peak_us": round(bytes_a / HBM_PEAK_BPS * 1e6, 2), "legs": {}}
        nbytes = {"a_stream_block": bytes_a, "b_one_shot_resample": bytes_b, "c_cat_resample_slice_clone": bytes_c,
                  "h_history_only": bytes_hist}
        for k, t in times.items():
            med = statistics.median(t)
            rec["legs"][k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                              "share_of_hbm_peak": round(nbytes[k] / (med * 1e-6) / HBM_PEAK_BPS, 4)}
        la, lb, lc, lh = (rec["legs"][k] for k in legs)
        rec["a_slowest_below_c_fastest"] = la["us_max"] < lc["us_min"]
        rec["c_median_over_a_median"] = round(lc["us_median"] / la["us_median"], 2)
        rec["a_minus_b_us_median"] = round(la["us_median"] - lb["us_median"], 2)
        rec["h_us_median"] = lh["us_median"]
        rec["b_spread_us"] = round(lb["us_max"] - lb["us_min"], 2)
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
