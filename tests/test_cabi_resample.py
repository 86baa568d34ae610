"""The resampling FIR's C ABI and host layer, without a GPU: the three fir_resample_* symbols, the
out_width rule, the order and texts of the refusals of both entries, empty problems, and the
Python layer's own refusals (each before any library call)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip

EINVAL, ENODEV = 1, 3
_NO_DEV = 1 << 20  # a device index no machine has: the device lookup itself refuses it
SYMBOLS = ("fir_resample_out_width", "fir_resample_rows", "fir_resample_rows_dev")
I64_MAX = 2**63 - 1


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
    assert fir_hip.EXPORTS["fir_resample_out_width"] == (ctypes.c_int64, [ctypes.c_int64] + [ctypes.c_int] * 3)
    assert len(fir_hip.EXPORTS["fir_resample_rows"][1]) == len(fir_hip.EXPORTS["fir_resample_rows_dev"][1]) == 15
    assert lib.fir_abi_version() == 6  # additive: the ABI number stays
    assert {"resample_out_width", "fir1d_fixed_rows_resample"} <= set(fir_hip.__all__)


OUT_WIDTH = [
    # width, up, decim, phase, out_width
    # width 0, and phase >= width * up: nothing is kept
    (0, 1, 1, 0, 0), (0, 16, 3, 2, 0), (0, 2**31 - 1, 2**31 - 1, 2**31 - 2, 0), (1, 2, 3, 2, 0), (1, 3, 8, 3, 0),
    (1, 3, 8, 7, 0), (5, 2, 16, 10, 0), (5, 2, 16, 15, 0), (1, 1, 2, 1, 0),
    # the last kept frame is the row's last, one short of it, one past it
    (1, 2, 3, 1, 1), (1, 2, 3, 0, 1), (1, 1, 1, 0, 1), (17, 1, 1, 0, 17),
    (6, 2, 3, 0, 4), (6, 2, 3, 1, 4), (6, 2, 3, 2, 4),        # width * up = 12: exact multiples of D
    (7, 2, 3, 0, 5), (7, 2, 3, 1, 5), (7, 2, 3, 2, 4),        # 14: one past
    (4, 5, 7, 0, 3), (4, 5, 7, 5, 3), (4, 5, 7, 6, 2),        # 20 = 3 * 7 - 1: one short
    (23, 3, 2, 0, 35), (23, 3, 2, 1, 34), (23, 16, 15, 0, 25), (23, 16, 15, 14, 24), (23, 15, 16, 9, 21),
    (100, 1, 4, 3, 25), (100, 4, 1, 0, 400), (5, 1000, 17, 16, 294), (1, 2**31 - 1, 2**31 - 1, 0, 1),
    (1, 2**31 - 1, 2**31 - 1, 2**31 - 2, 1), (3, 2**31 - 1, 2**31 - 1, 1, 3),
    # products at int64's edge ...
    (I64_MAX, 1, 1, 0, I64_MAX), (I64_MAX, 1, 2, 0, 1 << 62), (I64_MAX, 1, 2, 1, (1 << 62) - 1),
    ((1 << 62) - 1, 2, 2, 0, (1 << 62) - 1), (I64_MAX // 3, 3, 3, 2, I64_MAX // 3), (1 << 32, 2**31 - 1, 2**31 - 1, 0, 1 << 32),
    (1 << 61, 2, 1, 0, 1 << 62),
    # ... and past it
    (1 << 62, 2, 2, 0, -1), ((1 << 62) + 1, 2, 4, 1, -1), (1 << 61, 4, 16, 0, -1), (I64_MAX, 2, 2**31 - 1, 0, -1),
    (I64_MAX // 3 + 1, 3, 3, 0, -1), (1 << 33, 2**31 - 1, 2**31 - 1, 0, -1),
    # each bad argument
    (16, 0, 2, 0, -1), (16, -3, 2, 0, -1), (16, 2, 0, 0, -1), (16, 2, -1, 0, -1), (16, 2, 3, 3, -1), (16, 2, 3, -1, -1),
    (16, 2, 1, 1, -1), (-1, 2, 3, 0, -1), (-1, 0, 0, 0, -1), (0, 0, 1, 0, -1), (0, 1, 0, 0, -1), (0, 1, 1, 1, -1),
]


@pytest.mark.parametrize("width,up,decim,phase,want", OUT_WIDTH)
def test_out_width_table(lib, width, up, decim, phase, want):
    assert lib.fir_resample_out_width(width, up, decim, phase) == want
    if want >= 0:
        assert fir_hip.resample_out_width(width, up, decim, phase) == want == len(range(phase, width * up, decim))
        assert want == fir_hip.decim_out_width(fir_hip.interp_out_width(width, up), decim, phase)
    else:
        with pytest.raises(fir_hip.FirHipError, match="up must be >= 1|decim must be >= 1|phase must be in|"
                                                      "width must be >= 0|does not fit in int64"):
            fir_hip.resample_out_width(width, up, decim, phase)
    if phase == 0 and want >= 0:
        assert fir_hip.resample_out_width(width, up, decim) == want  # phase defaults to 0


def _table():
    """(entry, arguments, status, piece of fir_last_error) -- None: the device lookup's text.  A call
    that is wrong in two ways names the check that comes first: check_fir1d's own order, then up,
    then decim, then phase, then the sizes, then NULL x or y (only for a problem that is not empty),
    then, for the host form, the device lookup."""
    h = (ctypes.c_int32 * 3)(1, 2, 1)
    buf = np.zeros(1024, np.uint8)
    X = Y = buf.ctypes.data
    sizes = b"must fit in int64"
    t = []
    for fn, tail in (("fir_resample_rows_dev", None), ("fir_resample_rows", _NO_DEV)):
        def add(rc, msg, x=None, in_dtype=0, rows=0, width=16, ch=1, hq=h, taps=3, up=3, decim=2, phase=0, frac=12,
                acc=32, stage=0, y=None, fn=fn, tail=tail):
            t.append((fn, (x, in_dtype, rows, width, ch, hq, taps, up, decim, phase, frac, acc, stage, y, tail), rc, msg))
        # empty problems: FIR_OK without a device, NULL pointers and all
        add(0, b"")
        add(0, b"", rows=5, width=0)
        add(0, b"", rows=5, width=0, up=2**31 - 1, decim=2**31 - 1, phase=2**31 - 2)
        add(0, b"", rows=0, width=1 << 40, up=1000, decim=7, phase=6)
        add(0, b"", rows=0, width=1 << 40, up=1, decim=1, ch=3, in_dtype=1, stage=1)
        add(0, b"", rows=5, width=1, up=3, decim=8, phase=3)   # phase >= width * up: nothing is kept
        add(0, b"", rows=1 << 40, width=2, up=2, decim=16, phase=15, in_dtype=1, stage=1)
        # check_fir1d's checks, in its order, with its texts
        add(EINVAL, b"in_dtype must be FIR_IN_U8 or FIR_IN_I16", in_dtype=7, stage=5, up=0)
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=5, rows=-1, decim=0)
        add(EINVAL, b"rows and width must be >= 0", rows=-1, ch=0, up=0)
        add(EINVAL, b"rows and width must be >= 0", width=-1, phase=-1)
        add(EINVAL, b"channels must be >= 1", ch=0, hq=None, up=0)
        add(EINVAL, b"hq must not be NULL", hq=None, taps=0, decim=0)
        add(EINVAL, b"taps must be in [1, ", taps=0, frac=0, up=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", frac=0, up=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", acc=0, phase=9, rows=1)
        # then up, decim, phase, in that order
        add(EINVAL, b"up must be >= 1", up=0, rows=1)
        add(EINVAL, b"up must be >= 1", up=-2, decim=0, phase=-1)
        add(EINVAL, b"up must be >= 1", up=0, rows=1 << 40, width=1 << 40)  # before the sizes
        add(EINVAL, b"decim must be >= 1", decim=0, rows=1)
        add(EINVAL, b"decim must be >= 1", decim=-3, phase=-1)
        add(EINVAL, b"decim must be >= 1", decim=0, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"phase must be in [0, decim)", phase=2, rows=1)
        add(EINVAL, b"phase must be in [0, decim)", phase=-1)
        add(EINVAL, b"phase must be in [0, decim)", decim=1, phase=1, up=1)
        add(EINVAL, b"phase must be in [0, decim)", phase=2, rows=1 << 40, width=1 << 40)  # before the sizes
        # then the sizes, with a text of their own
        add(EINVAL, sizes, rows=1 << 40, width=1 << 40)
        add(EINVAL, sizes, rows=1, width=1 << 62, up=2)                       # width * up
        add(EINVAL, sizes, rows=0, width=1 << 62, up=4, decim=16)             # ... which out_width itself needs
        add(EINVAL, sizes, rows=1, width=1 << 61, up=1, decim=1)              # * 4
        add(EINVAL, sizes, rows=1, width=1 << 60, up=4, decim=2)              # out_width = 2^61, * 4
        add(EINVAL, sizes, rows=1 << 22, width=1 << 20, up=1 << 20, decim=2, ch=2, in_dtype=1)
        add(EINVAL, sizes, rows=1 << 40, width=1 << 21, up=1, decim=1 << 20, ch=2, in_dtype=1)  # the input's own size
        add(EINVAL, sizes, rows=1, width=1 << 59, up=4, decim=2, ch=2, in_dtype=1, x=X, y=Y)
        # then the pointers, only when something would be computed
        add(EINVAL, b"x and y must not be NULL", rows=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, x=X)
        add(EINVAL, b"x and y must not be NULL", rows=1, y=Y, up=16, decim=15, phase=14)
        add(EINVAL, b"x and y must not be NULL", rows=1, up=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, decim=1)
        if tail is not None:  # the host form gets as far as the device lookup
            add(ENODEV, None, rows=1, x=X, y=Y)
            add(ENODEV, None, rows=2, x=X, y=Y, up=16, decim=15, phase=7, in_dtype=1, stage=1)
            add(ENODEV, None, rows=1, x=X, y=Y, up=1, decim=4, phase=3)
            add(ENODEV, None, rows=1, x=X, y=Y, up=4, decim=1)
    return t, buf


def test_refusal_order_of_both_entries(lib):
    count = ctypes.c_int32(-1)
    have = lib.fir_device_count(ctypes.byref(count)) == 0 and count.value > 0
    nodev = b"out of range" if have else b"no HIP device available"
    table, keep = _table()
    assert {fn for fn, *_ in table} == {"fir_resample_rows", "fir_resample_rows_dev"}
    bad = []
    for fn, args, want, msg in table:
        rc = getattr(lib, fn)(*args)
        err = lib.fir_last_error()
        if rc != want or (want and (nodev if msg is None else msg) not in err):
            bad.append((fn, args, want, msg, rc, err))
    assert not bad, "\n".join(f"{fn}{args}: want {want} {msg!r}, got {rc} {err!r}" for fn, args, want, msg, rc, err in bad)
    del keep


def test_empty_problems_need_no_device(lib):
    h = (ctypes.c_int32 * 5)(-256, -1024, 6656, -1024, -256)
    for in_dtype, ch, stage in ((0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1), (1, 2, 1), (1, 3, 1)):
        for rows, width, up, decim, phase in ((0, 0, 1, 1, 0), (0, 4096, 4, 3, 2), (7, 0, 4, 3, 0), (7, 0, 1, 1, 0),
                                              (0, 1, 1000, 999, 5), (7, 1, 3, 8, 3), (7, 2, 2, 16, 4), (7, 1, 1, 2, 1)):
            rc = lib.fir_resample_rows_dev(None, in_dtype, rows, width, ch, h, 5, up, decim, phase, 12, 32, stage, None, None)
            assert rc == 0, (in_dtype, ch, stage, rows, width, up, decim, phase, lib.fir_last_error())
            rc = lib.fir_resample_rows(None, in_dtype, rows, width, ch, h, 5, up, decim, phase, 12, 32, stage, None, _NO_DEV)
            assert rc == 0, (in_dtype, ch, stage, rows, width, up, decim, phase, lib.fir_last_error())


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a call the host layer must refuse")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(fir_hip, "lib", lambda: _NoLibrary())
    x = np.zeros((4, 16), np.uint8)
    h = [1, 2, 1]
    f = fir_hip.fir1d_fixed_rows_resample
    for up in (0, -1, -16):
        with pytest.raises(fir_hip.FirHipError, match="up must be >= 1"):
            f(x, h, up, 2)
    for decim in (0, -1):
        with pytest.raises(fir_hip.FirHipError, match="decim must be >= 1"):
            f(x, h, 3, decim)
    for decim, phase in ((2, 2), (2, -1), (1, 1), (16, 16)):
        with pytest.raises(fir_hip.FirHipError, match=r"phase must be in \[0, decim\)"):
            f(x, h, 3, decim, phase)
    with pytest.raises(fir_hip.FirHipError, match="up must be >= 1"):  # up before decim before phase
        f(x, h, 0, 0, -1)
    with pytest.raises(fir_hip.FirHipError, match="decim must be >= 1"):
        f(x, h, 1, 0, -1)
    with pytest.raises(fir_hip.FirHipError, match="dtype"):
        f(x.astype(np.float32), h, 3, 2)
    with pytest.raises(fir_hip.FirHipError, match="channels"):
        f(np.zeros((4, 15), np.int16), h, 3, 2, channels=2)
    with pytest.raises(fir_hip.FirHipError, match="channels"):
        f(x, h, 3, 2, channels=0)
    for taps, text in (([], "non-empty 1-D"), ([[1, 2]], "non-empty 1-D"), ([1, 2**31], "fit in int32")):
        with pytest.raises(fir_hip.FirHipError, match=text):
            f(x, taps, 3, 2)
    # out=: 16 frames * 3 / 2 = 24.  Wrong dtype, wrong shape, layout, not an array, read-only
    ro = np.zeros((4, 24), np.uint8)
    ro.flags.writeable = False
    bad = [np.zeros((4, 24), np.int32), np.zeros((4, 16), np.uint8), np.zeros((4, 48), np.uint8), np.zeros((4, 23), np.uint8),
           np.zeros((3, 24), np.uint8), np.zeros((24, 4), np.uint8).T, [[0] * 24] * 4, ro]
    for out in bad:
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            f(x, h, 3, 2, out=out)
    with pytest.raises(fir_hip.FirHipError, match="out must"):  # phase 1 of 5 frames * 3 / 2 keeps 7, phase 0 keeps 8
        f(np.zeros((4, 5), np.uint8), h, 3, 2, 1, out=np.zeros((4, 8), np.uint8))
    with pytest.raises(fir_hip.FirHipError, match="out must be int32"):
        f(x, h, 3, 2, out_stage=fir_hip.OUT_I32, out=np.zeros((4, 24), np.uint8))
    big = np.zeros(4 * 24 + 64, np.uint8)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # x inside out
        f(big[16:80].reshape(4, 16), h, 3, 2, out=big[:96].reshape(4, 24))
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # in place is refused even at up = decim = 1
        f(x.reshape(-1), h, 1, 1, out=x.reshape(-1))
    x16 = np.zeros(256, np.int16)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # a partial overlap through a view
        f(x16[:32], h, 3, 2, out_stage=fir_hip.OUT_I32, out=x16.view(np.int32)[8:56])
    # a complex row counts frames: 16 int16 = 8 frames -> 12 frames = 24 values
    with pytest.raises(fir_hip.FirHipError, match=r"shape \(4, 24\)"):
        f(np.zeros((4, 16), np.int16), h, 3, 2, channels=2, out_stage=fir_hip.OUT_I32, out=np.zeros((4, 48), np.int32))
