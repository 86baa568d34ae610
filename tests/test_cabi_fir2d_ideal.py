"""The float64 ideal 2-D entries without a device: the four symbols are exported, structurally
invalid calls get FIR_EINVAL and a message, empty problems are no-ops, and the Python layers
(fir_hip.fir2d_ideal, fir_2d.model.python.fir_2d_ref) refuse bad arguments before any library
or device call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip
from fir_2d.model.python.fir_2d_ref import fir_2d_compare, fir_2d_fixed_golden, fir_2d_ideal

NAMES = ("fir2d_ideal", "fir2d_ideal_dev", "fir2d_ideal_frames", "fir2d_ideal_frames_dev")
BAD_H = r"Invalid h: h must be a non-empty 2-D array of coefficients\."


@pytest.fixture(scope="module")
def lib():
    if not fir_hip.lib_path().exists():
        pytest.fail(f"{fir_hip.lib_path()} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return fir_hip.lib()


def test_the_four_symbols_are_exported(lib):
    raw = ctypes.CDLL(str(fir_hip.lib_path()))
    for name in NAMES:
        assert name in fir_hip.EXPORTS and hasattr(raw, name), name


def _einval(lib, rc, word: bytes):
    assert rc == 1, rc
    assert word in lib.fir_last_error(), lib.fir_last_error()


def test_invalid_arguments_are_rejected_without_device(lib):
    h = (ctypes.c_double * 9)(*([0.5] * 9))
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused first
    for host in (False, True):  # the _dev entries (stream NULL) and the host entries (device 0)
        one = lib.fir2d_ideal if host else lib.fir2d_ideal_dev
        many = lib.fir2d_ideal_frames if host else lib.fir2d_ideal_frames_dev
        last = 0 if host else None
        _einval(lib, one(p, 4, 4, h, 0, 3, p, last), b"tap_rows")
        _einval(lib, one(p, 4, 4, h, 3, 0, p, last), b"tap_cols")
        _einval(lib, one(p, -4, 4, h, 3, 3, p, last), b"height")
        _einval(lib, many(p, 65536, 4, 4, h, 3, 3, p, last), b"65535")
        _einval(lib, many(p, -1, 4, 4, h, 3, 3, p, last), b"frames")
        _einval(lib, one(p, 4, 4, None, 3, 3, p, last), b"h must not be NULL")
        _einval(lib, one(None, 4, 4, h, 3, 3, p, last), b"NULL")
        _einval(lib, one(p, 4, 4, h, 3, 3, None, last), b"NULL")
        # empty problems are valid no-ops, NULL buffers included
        assert one(None, 0, 4, h, 3, 3, None, last) == 0
        assert one(None, 4, 0, h, 3, 3, None, last) == 0
        assert many(None, 0, 4, 4, h, 3, 3, None, last) == 0
        # ... but still check their taps
        _einval(lib, many(None, 0, 4, 4, h, 0, 3, None, last), b"tap_rows")


def test_host_binding_refuses_bad_ranks_and_out_before_any_call():
    x = np.zeros((4, 8), np.uint8)
    k = np.full((3, 3), 0.25)
    for bad_h in ([0.25, 0.5, 0.25], np.zeros((1, 3, 3)), np.zeros((0, 3)), 0.5):
        with pytest.raises(fir_hip.FirHipError, match="h2"):
            fir_hip.fir2d_ideal(x, bad_h)
    for bad_x in (np.zeros(8, np.uint8), np.zeros((1, 2, 4, 8), np.uint8)):
        with pytest.raises(fir_hip.FirHipError, match="x must be"):
            fir_hip.fir2d_ideal(bad_x, k)
    ro = np.zeros((4, 8), np.float64)
    ro.flags.writeable = False
    for out in (np.zeros((4, 8), np.float32), np.zeros((4, 7), np.float64), np.zeros((8, 4), np.float64).T,
                np.zeros((1, 4, 8), np.float64), [[0.0] * 8] * 4, ro):
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            fir_hip.fir2d_ideal(x, k, out=out)
    # an empty frame is a no-op of the library: nothing to compute, no device needed
    assert fir_hip.fir2d_ideal(np.zeros((0, 8), np.uint8), k).shape == (0, 8)
    assert fir_hip.fir2d_ideal(np.zeros((3, 0, 8), np.uint8), k).dtype == np.float64


MODELS = (fir_2d_ideal, fir_2d_fixed_golden, fir_2d_compare)


@pytest.mark.parametrize("model", MODELS)
def test_model_layer_argument_checks(model):
    x = np.zeros((4, 8), np.uint8)
    for empty in ([], [[]], [[], []], np.zeros((0, 3)), np.zeros((3, 0))):
        with pytest.raises(ValueError, match=BAD_H):
            model(x, empty)
    for ragged in ([[0.1, 0.2], [0.3]], [0.1, 0.2, 0.3], 0.5, np.zeros((1, 3, 3)).tolist()):
        with pytest.raises(ValueError, match=BAD_H):
            model(x, ragged)
    # the 1-D validator on the row-major flattened kernel: the index is the flat one
    with pytest.raises(ValueError, match=r"Invalid h\[4\]=nan: h coefficients must be finite\."):
        model(x, [[0.1, 0.2, 0.3], [0.4, float("nan"), 0.6]])
    with pytest.raises(ValueError, match=r"Invalid h\[5\]=-8\.5: \|h\| must be <= 8\.0\."):
        model(x, [[0.1, 0.2, 0.3], [0.4, 0.5, -8.5], [9.0, 0.0, 0.0]])
    # h is checked before x
    with pytest.raises(ValueError, match=BAD_H):
        model(np.zeros(8, np.uint8), [])
    with pytest.raises(ValueError, match=r"Invalid x: x must be a 2-D array"):
        model(np.zeros(8, np.uint8), [[0.25, 0.5, 0.25]])
    with pytest.raises(ValueError, match=r"Invalid x: x must be a 2-D array"):
        model(np.zeros((2, 4, 8), np.uint8), [[0.25, 0.5, 0.25]])
    with pytest.raises(ValueError, match=r"Invalid x\[1\]=inf: x must be finite\."):
        model(np.array([[1.0, 2.0], [3.0, np.inf]]), [[0.25, 0.5, 0.25]])


def test_q_range_is_the_fixed_models_check_only():
    x = np.zeros((0, 8), np.uint8)  # empty frame: every check runs, nothing is computed
    h = [[0.5, 8.0], [0.25, 0.125]]  # 8.0 passes |h| <= 8 and lies beyond Q4.12's 7.999755859375
    assert fir_2d_ideal(x, h).shape == (0, 8) and fir_2d_ideal(x, h).dtype == np.float64
    for model in (fir_2d_fixed_golden, fir_2d_compare):
        with pytest.raises(ValueError, match=r"Invalid h\[1\]=8\.0: out of Q-format real range"):
            model(x, h)
        with pytest.raises(ValueError, match=r"Invalid coeff_bits=12"):
            model(x, [[0.5]], coeff_bits=12)
    # x is prepared before the coefficient stage
    with pytest.raises(ValueError, match=r"Invalid x\[0\]=nan"):
        fir_2d_fixed_golden(np.array([[np.nan, 1.0]]), h)


def test_empty_frames_need_no_device():
    k = [[0.25, 0.5, 0.25]]
    y = fir_2d_fixed_golden(np.zeros((0, 5), np.uint8), k)
    assert y.shape == (0, 5) and y.dtype == np.uint8
    assert fir_2d_ideal(np.zeros((5, 0)), k).shape == (5, 0)
    m = fir_2d_compare(np.zeros((0, 5), np.uint8), k)
    assert m["num_samples"] == 0 and set(m) == {"num_samples", "max_abs_err", "mae", "rmse", "mean_err",
                                                "sat_low_ratio", "sat_high_ratio", "sat_ratio", "clip_needed_ratio"}
