"""The complex-tap FIR's C ABI and host layer, without a GPU: the two fir_cplx_* symbols, the order
and texts of the refusals of both entries, empty problems, and the Python layer's own refusals (each
before any library call)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip

EINVAL, ENODEV = 1, 3
_NO_DEV = 1 << 20  # a device index no machine has: the device lookup itself refuses it
SYMBOLS = ("fir_cplx_rows", "fir_cplx_rows_dev")


@pytest.fixture(scope="module")
def lib():
    if not fir_hip.lib_path().exists():
        pytest.fail(f"{fir_hip.lib_path()} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return fir_hip.lib()


def test_symbols_are_exported_and_bound(lib):
    raw = ctypes.CDLL(str(fir_hip.lib_path()))
    for name in SYMBOLS:
        assert name in fir_hip.EXPORTS, name
        assert hasattr(raw, name), name
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert fir_hip.EXPORTS["fir_cplx_rows"] == (i32, [vp, i64, i64, vp, i32, i32, i32, i32, vp, i32])
    assert fir_hip.EXPORTS["fir_cplx_rows_dev"] == (i32, [vp, i64, i64, vp, i32, i32, i32, i32, vp, vp])
    assert lib.fir_abi_version() == 6  # additive: the ABI number stays
    assert "fir1d_fixed_rows_cplx" in fir_hip.__all__


def _table():
    """(entry, arguments, status, piece of fir_last_error) -- None: the device lookup's text.  A call
    that is wrong in two ways names the check that comes first: check_fir1d's own order (for int16
    of two channels: the stage, rows and width, hq, taps, frac_bits and acc_bits), then the sizes,
    then NULL x or y (only for a problem that is not empty), then, for the host form, the device
    lookup."""
    h = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    buf = np.zeros(1024, np.uint8)
    X = Y = buf.ctypes.data
    sizes = b"must fit in int64"
    t = []
    for fn, tail in (("fir_cplx_rows_dev", None), ("fir_cplx_rows", _NO_DEV)):
        def add(rc, msg, x=None, rows=0, width=16, hq=h, taps=3, frac=12, acc=32, stage=1, y=None, fn=fn, tail=tail):
            t.append((fn, (x, rows, width, hq, taps, frac, acc, stage, y, tail), rc, msg))
        # empty problems: FIR_OK without a device, NULL pointers and all
        add(0, b"")
        add(0, b"", rows=5, width=0)
        add(0, b"", rows=0, width=1 << 40, stage=0)
        add(0, b"", rows=1 << 40, width=0, acc=64, frac=40)
        add(0, b"", rows=0, width=0, taps=1)
        # check_fir1d's checks, in its order, with its texts
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=5, rows=-1, hq=None)
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=-1, taps=0)
        add(EINVAL, b"rows and width must be >= 0", rows=-1, hq=None, taps=0)
        add(EINVAL, b"rows and width must be >= 0", width=-1, frac=0)
        add(EINVAL, b"hq must not be NULL", hq=None, taps=0, frac=0)
        add(EINVAL, b"taps must be in [1, ", taps=0, frac=0)
        add(EINVAL, b"taps must be in [1, ", taps=-3, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", frac=0, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", acc=0, rows=1)
        # then the sizes, with a text of their own
        add(EINVAL, sizes, rows=1 << 40, width=1 << 40)
        add(EINVAL, sizes, rows=1, width=1 << 60)                    # * 2 * 4
        add(EINVAL, sizes, rows=1 << 30, width=1 << 30, x=X, y=Y)
        add(EINVAL, sizes, rows=1 << 62, width=2)
        # then the pointers, only when something would be computed
        add(EINVAL, b"x and y must not be NULL", rows=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, x=X)
        add(EINVAL, b"x and y must not be NULL", rows=1, y=Y, stage=0)
        add(EINVAL, b"x and y must not be NULL", rows=1 << 29, width=1 << 30)  # the largest legal size
        if tail is not None:  # the host form gets as far as the device lookup
            add(ENODEV, None, rows=1, x=X, y=Y)
            add(ENODEV, None, rows=2, x=X, y=Y, stage=0, acc=64)
    return t, buf


def test_refusal_order_of_both_entries(lib):
    count = ctypes.c_int32(-1)
    have = lib.fir_device_count(ctypes.byref(count)) == 0 and count.value > 0
    nodev = b"out of range" if have else b"no HIP device available"
    table, keep = _table()
    assert {fn for fn, *_ in table} == set(SYMBOLS)
    bad = []
    for fn, args, want, msg in table:
        rc = getattr(lib, fn)(*args)
        err = lib.fir_last_error()
        if rc != want or (want and (nodev if msg is None else msg) not in err):
            bad.append((fn, args, want, msg, rc, err))
    assert not bad, "\n".join(f"{fn}{args}: want {want} {msg!r}, got {rc} {err!r}" for fn, args, want, msg, rc, err in bad)
    del keep


def test_empty_problems_need_no_device(lib):
    h = (ctypes.c_int32 * 10)(-256, 3, -1024, 0, 6656, -7, -1024, 0, -256, 1)
    for stage in (0, 1):
        for rows, width in ((0, 0), (0, 4096), (7, 0), (0, 1)):
            for acc, frac in ((32, 12), (64, 40), (8, 1)):
                rc = lib.fir_cplx_rows_dev(None, rows, width, h, 5, frac, acc, stage, None, None)
                assert rc == 0, (stage, rows, width, lib.fir_last_error())
                rc = lib.fir_cplx_rows(None, rows, width, h, 5, frac, acc, stage, None, _NO_DEV)
                assert rc == 0, (stage, rows, width, lib.fir_last_error())


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a call the host layer must refuse")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(fir_hip, "lib", lambda: _NoLibrary())
    x = np.zeros((4, 16), np.int16)
    h = [[1, 2], [3, 4], [5, 6]]
    f = fir_hip.fir1d_fixed_rows_cplx
    for bad in (x.astype(np.uint8), x.astype(np.int32), x.astype(np.float32), x.astype(np.complex64), x.tolist()):
        with pytest.raises(fir_hip.FirHipError, match="x must be an int16 array"):
            f(bad, h)
    with pytest.raises(fir_hip.FirHipError, match="at least one axis"):
        f(np.zeros((), np.int16), h)
    for odd in (np.zeros((4, 15), np.int16), np.zeros(1, np.int16), np.zeros((2, 3, 7), np.int16)):
        with pytest.raises(fir_hip.FirHipError, match="even number of values"):
            f(odd, h)
    shape = r"non-empty \(taps, 2\) array"
    for taps in ([1, 2, 3], [[1, 2, 3]], np.zeros((0, 2), np.int64), np.zeros((2, 2, 2), np.int64), [], 7, [[1], [2]]):
        with pytest.raises(fir_hip.FirHipError, match=shape):
            f(x, taps)
    for taps in ([[1.0, 2.0]], np.ones((3, 2), np.float32), np.ones((3, 2), bool), np.ones((3, 2), np.complex64),
                 [[1, None]], [[2**70, 1.5]]):
        with pytest.raises(fir_hip.FirHipError, match="hq must be an integer array"):
            f(x, taps)
    for taps in ([[1, 2**31]], [[-2**31 - 1, 0]], [[0, 1], [2**40, 0]], [[2**70, 0]], np.array([[2**63, 0]], np.uint64)):
        with pytest.raises(fir_hip.FirHipError, match="must fit in int32"):
            f(x, taps)
    monkeypatch.setattr(fir_hip, "MAX_TAPS", 4)
    with pytest.raises(fir_hip.FirHipError, match="exceed the library limit of 4"):
        f(x, np.ones((5, 2), np.int64))
    monkeypatch.undo()
    monkeypatch.setattr(fir_hip, "lib", lambda: _NoLibrary())
    # out=: x's shape, int32 (uint8 for the u8 stage); wrong dtype, shape, layout, not an array, read-only, overlap
    ro = np.zeros((4, 16), np.int32)
    ro.flags.writeable = False
    for out in (np.zeros((4, 16), np.uint8), np.zeros((4, 8), np.int32), np.zeros((4, 32), np.int32),
                np.zeros((16, 4), np.int32).T, [[0] * 16] * 4, ro):
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            f(x, h, out=out)
    with pytest.raises(fir_hip.FirHipError, match="out must be uint8"):
        f(x, h, out_stage=fir_hip.OUT_U8_SAT, out=np.zeros((4, 16), np.int32))
    big = np.zeros(256, np.int16)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):
        f(big[:32], h, out=big.view(np.int32)[8:40])
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # u8 in place is refused too
        f(big[:32], h, out_stage=fir_hip.OUT_U8_SAT, out=big.view(np.uint8)[:32])


def test_python_layer_passes_the_call_on(monkeypatch):
    """An accepted call reaches fir_cplx_rows once, with rows, width in FRAMES, the taps and the
    scalars; int32's ends are accepted."""
    calls = []

    class Rec:
        def fir_cplx_rows(self, *a):
            taps = tuple((ctypes.c_int32 * (2 * a[4])).from_address(a[3].value))
            calls.append((a[1], a[2], taps) + tuple(a[4:8]) + (a[9],))
            return 0

    monkeypatch.setattr(fir_hip, "lib", lambda: Rec())
    x = np.zeros((3, 5, 16), np.int16)
    y = fir_hip.fir1d_fixed_rows_cplx(x, [[2**31 - 1, -2**31], [3, -4]], 7, 24, device=2)
    assert y.shape == x.shape and y.dtype == np.int32
    assert calls == [(15, 8, (2**31 - 1, -2**31, 3, -4), 2, 7, 24, fir_hip.OUT_I32, 2)]
    y = fir_hip.fir1d_fixed_rows_cplx(x[..., :0], np.array([[1, 2]], np.int8), out_stage=fir_hip.OUT_U8_SAT)
    assert y.shape == (3, 5, 0) and y.dtype == np.uint8 and calls[-1][:2] == (0, 0)
    import inspect
    sig = inspect.signature(fir_hip.fir1d_fixed_rows_cplx)
    assert list(sig.parameters) == ["x", "hq", "frac_bits", "acc_bits", "out_stage", "device", "out"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, device=0, out=None)
