"""GPU parity of the float64 ideal 2-D FIR (fir2d_ideal*, csrc/ideal2d.hip) and of the 2-D model
layer (fir_2d/model/python/fir_2d_ref.py).

Every comparison is byte equality (``tobytes()``) with the NumPy checker tests/ideal2d_ref.py,
itself proven in tests/test_ideal2d_ref.py.  Taps come from uniform(-8, 8): full mantissas, so a
contracted multiply-add, a reordered sum or a sum seeded with its first product changes bytes.
"""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import torch

import fir_hip
from conftest import IMAGES, same_metrics
from fir_2d.model.python.fir_2d_ref import fir_2d_compare, fir_2d_fixed_golden, fir_2d_ideal
from fir_hip import torch_ops
from guarded import guarded_input, guarded_output
from ideal2d_ref import ideal2d
from oracle import c_oracle, fir_oracle as fo

DEV = torch.device("cuda:0")

# csrc/ideal2d.hip: kIdeal2dStrip (output rows per strip of the register kernel), the wave tile
# (64 lanes x 4 pixels) and kIdeal2dMaxRC (largest R, C of the register kernel)
STRIP = 16
WAVE_TILE = 256
REG_MAX = 5


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _case(shape, R, C, salt=0):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + R * 10 + C + salt)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.uniform(-8, 8, (R, C))


# ---- shapes x kernels: the grid of the fixed 2-D test --------------------------------------
# Both dispatch branches: widths that are / are not whole dwords and whole wave tiles, H < R,
# W < C, 7x7 (generic whatever the frame).
@pytest.mark.parametrize("shape", [(1, 16), (3, 32), (37, 64), (64, 64), (100, 1280), (257, 4096), (5, 16 * 300),
                                   (33, 17), (40, 4499), (1, 1), (7, 3)])
@pytest.mark.parametrize("R,C", [(5, 5), (3, 3), (1, 5), (5, 1), (3, 5), (2, 4), (7, 7)])
def test_ideal2d_vs_checker(shape, R, C):
    x, h = _case(shape, R, C)
    assert fir_hip.fir2d_ideal(x, h).tobytes() == ideal2d(x, h).tobytes()


# ---- strip seams of the register kernel ---------------------------------------------------
@pytest.mark.parametrize("R,C", [(5, 5), (3, 3), (2, 4), (4, 2)])
def test_ideal2d_strip_and_wave_tile_seams(R, C):
    heights = (STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + R - 2)
    widths = [WAVE_TILE * k + d for k in (1, 2) for d in (-4, 4)]
    for H in heights:
        for W in widths:
            x, h = _case((H, W), R, C, salt=7)
            assert fir_hip.fir2d_ideal(x, h).tobytes() == ideal2d(x, h).tobytes(), (H, W)


def test_ideal2d_frame_taller_than_65535_strips():
    """Past 65535 * STRIP rows the launcher grows the strip height (the grid's y limit): 17-row
    strips here, a height the other cases never reach."""
    H = 65535 * STRIP + 5
    x, h = _case((H, 8), 3, 3, salt=11)
    assert fir_hip.fir2d_ideal(x, h).tobytes() == ideal2d(x, h).tobytes()


# ---- the accumulator starts at +0.0 -------------------------------------------------------
@pytest.mark.parametrize("shape,R,C", [((STRIP + 3, 260), 3, 3), ((STRIP + 3, 260), 5, 5),  # register kernel
                                       ((STRIP + 3, 259), 3, 3), ((9, 64), 7, 7)])           # generic kernel
def test_zero_frame_under_negative_taps_is_plus_zero(shape, R, C):
    h = -np.random.default_rng(R * C).uniform(0.5, 8, (R, C))
    y = fir_hip.fir2d_ideal(np.zeros(shape, np.uint8), h)
    assert y.tobytes() == np.zeros(shape, np.float64).tobytes()  # +0.0 everywhere, never -0.0


# ---- the reference's own bytes: one non-zero kernel row / column is its 1-D ideal filter ---
def _image_stems():
    with np.load(IMAGES) as d:  # names only: nothing is decoded at collection time
        return sorted(d.files)


@pytest.mark.parametrize("stem", _image_stems())
def test_centre_row_and_column_pins_on_the_golden_images(stem, images, image_outputs):
    x = images[stem]
    xt = np.ascontiguousarray(x.T)
    seen = 0
    for o in image_outputs["outputs"]:
        if o["tap"] != "5tap" or o["case_stem"] != stem:
            continue
        k = np.zeros((5, 5))
        k[2] = image_outputs["banks"]["5tap"][o["coeff_name"]]
        assert _sha(fir_hip.fir2d_ideal(x, k)) == o["ideal_f64_sha256"], o["coeff_name"]
        assert _sha(fir_hip.fir2d_ideal(xt, np.ascontiguousarray(k.T)).T) == o["ideal_f64_sha256"], o["coeff_name"]
        seen += 1
    assert seen == len(image_outputs["banks"]["5tap"])


# ---- frames -------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(3, 3), (5, 5), (7, 7)])
def test_frame_batch_equals_single_frames_host_and_device(R, C):
    x, h = _case((3, 37, 260), R, C)
    got = fir_hip.fir2d_ideal(x, h)
    dev = torch_ops.fir2d_ideal_dev(torch.from_numpy(x).to(DEV), h)
    torch.cuda.synchronize()
    assert got.shape == x.shape and got.dtype == np.float64
    assert dev.cpu().numpy().tobytes() == got.tobytes()
    for f in range(3):
        assert got[f].tobytes() == fir_hip.fir2d_ideal(x[f], h).tobytes(), f
        one = torch_ops.fir2d_ideal_dev(torch.from_numpy(x[f]).to(DEV), h)
        torch.cuda.synchronize()
        assert one.cpu().numpy().tobytes() == got[f].tobytes(), f
        assert got[f].tobytes() == ideal2d(x[f], h).tobytes(), f


# ---- guard bands: nothing outside the input is used, nothing outside the output is written ---
GUARD_CASES = [  # (shape, input lead bytes, output lead bytes): lead 0 / 4 keep x 4-byte aligned
    ((19, 260), 0, 0),     # register kernel
    ((19, 260), 4, 0),     # register kernel, x 4 bytes past a 512-byte boundary
    ((19, 260), 1, 8),     # generic kernel (x odd, y 8 bytes off a 16-byte boundary)
    ((2, 9, 36), 0, 0),    # batch, register kernel
    ((2, 9, 36), 1, 8),    # batch, generic kernel
]


@pytest.mark.parametrize("shape,lead_in,lead_out", GUARD_CASES)
@pytest.mark.parametrize("R,C", [(5, 5), (3, 3)])
def test_guard_bands(shape, lead_in, lead_out, R, C):
    x, h = _case(shape, R, C, salt=3)
    xd = guarded_input(torch.from_numpy(x), lead_bytes=lead_in, device=DEV)
    yd, check = guarded_output(shape, torch.float64, lead_bytes=lead_out, device=DEV)
    assert xd.data_ptr() % 4 == lead_in % 4 and yd.data_ptr() % 16 == lead_out
    torch_ops.fir2d_ideal_dev(xd, h, out=yd)
    torch.cuda.synchronize()
    got = yd.cpu().numpy()
    frames = x if x.ndim == 3 else x[None]
    want = np.stack([ideal2d(f, h) for f in frames]).reshape(shape)
    assert got.tobytes() == want.tobytes()
    check(f"fir2d_ideal_dev {shape} {R}x{C}")


# ---- stream order and graph capture -------------------------------------------------------
def test_non_default_stream_and_graph_replay():
    H, W = 41, 516
    rng = np.random.default_rng(99)
    h = rng.uniform(-8, 8, (5, 5))
    s = torch.cuda.Stream(device=DEV)
    xh = rng.integers(0, 256, (H, W), dtype=np.uint8)
    x = torch.from_numpy(xh).to(DEV)
    y = torch.empty((H, W), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # also warms the entry outside the capture
        torch_ops.fir2d_ideal_dev(x, h, out=y)
    s.synchronize()
    assert y.cpu().numpy().tobytes() == ideal2d(xh, h).tobytes()
    y2 = torch.empty_like(y)
    torch_ops.fir2d_ideal_dev(x, h, out=y2, stream=s)  # the explicit stream argument
    s.synchronize()
    assert y2.cpu().numpy().tobytes() == ideal2d(xh, h).tobytes()

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        torch_ops.fir2d_ideal_dev(x, h, out=y)
    torch.cuda.synchronize()
    for seed in (1, 2):
        xh = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
        x.copy_(torch.from_numpy(xh))
        y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == ideal2d(xh, h).tobytes(), seed


# ---- model layer --------------------------------------------------------------------------
MODEL_KERNELS = {
    "box3": np.full((3, 3), 1 / 9).tolist(),
    "sharpen3": [[0.0, -1.0, 0.0], [-1.0, 5.0, -1.0], [0.0, -1.0, 0.0]],
    "gauss5": (np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256).tolist(),
}


@pytest.mark.parametrize("name", sorted(MODEL_KERNELS))
def test_model_layer(name):
    h = MODEL_KERNELS[name]
    x = np.random.default_rng(len(name)).integers(0, 256, (64, 96), dtype=np.uint8)
    hq = fo.quantize_h(np.asarray(h).reshape(-1)).reshape(np.asarray(h).shape)
    fixed = fir_2d_fixed_golden(x, h)
    assert fixed.dtype == np.uint8 and np.array_equal(fixed, c_oracle().fir2d(x, hq, 12, 32, 0))
    ideal = fir_2d_ideal(x, h)
    want = ideal2d(x, h)
    assert ideal.dtype == np.float64 and ideal.tobytes() == want.tobytes()
    got = fir_2d_compare(x, h)
    ref = fo.compute_metrics(want, fixed)
    assert same_metrics(got, ref) == [], (got, ref)
    # float input frames are prepared like the 1-D model's rows: round half up, clamp
    xf = x.astype(np.float64) + 0.25
    xf[0, 0], xf[0, 1] = -3.0, 400.0
    xp = np.clip(np.floor(xf + 0.5), 0, 255).astype(np.uint8)
    assert fir_2d_ideal(xf, h).tobytes() == ideal2d(xp, h).tobytes()
