"""The interpolating FIR's C ABI and host layer, without a GPU: the three fir_interp_* symbols, the
out_width rule, the order and texts of the refusals of both entries, empty problems, and the
Python layer's own refusals (each before any library call)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip

EINVAL, ENODEV = 1, 3
_NO_DEV = 1 << 20  # a device index no machine has: the device lookup itself refuses it
SYMBOLS = ("fir_interp_out_width", "fir_interp_rows", "fir_interp_rows_dev")
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
    assert fir_hip.EXPORTS["fir_interp_out_width"][0] is ctypes.c_int64
    assert len(fir_hip.EXPORTS["fir_interp_rows"][1]) == len(fir_hip.EXPORTS["fir_interp_rows_dev"][1]) == 13
    assert lib.fir_abi_version() == 6  # additive: the ABI number stays
    assert {"interp_out_width", "fir1d_fixed_rows_interp"} <= set(fir_hip.__all__)


OUT_WIDTH = [
    # width, up, out_width
    (0, 1, 0), (0, 16, 0), (0, 2**31 - 1, 0), (1, 1, 1), (17, 1, 17), (1 << 62, 1, 1 << 62), (I64_MAX, 1, I64_MAX),
    (1, 2, 2), (16, 2, 32), (17, 3, 51), (5, 1000, 5000), (1, 2**31 - 1, 2**31 - 1),
    (1 << 61, 2, 1 << 62), ((1 << 62) - 1, 2, (1 << 63) - 2), (1 << 60, 7, 7 << 60), (I64_MAX // 3, 3, I64_MAX // 3 * 3),
    (1 << 32, 2**31 - 1, (1 << 32) * (2**31 - 1)),
    # overflow
    (1 << 62, 2, -1), ((1 << 62) + 1, 2, -1), (1 << 61, 4, -1), (I64_MAX, 2, -1), (I64_MAX // 3 + 1, 3, -1),
    (1 << 33, 2**31 - 1, -1),
    # bad arguments
    (16, 0, -1), (16, -3, -1), (-1, 2, -1), (-1, 0, -1), (0, 0, -1),
]


@pytest.mark.parametrize("width,up,want", OUT_WIDTH)
def test_out_width_table(lib, width, up, want):
    assert lib.fir_interp_out_width(width, up) == want
    if want >= 0:
        assert fir_hip.interp_out_width(width, up) == want == width * up
    else:
        with pytest.raises(fir_hip.FirHipError, match="up must be >= 1|width must be >= 0|does not fit in int64"):
            fir_hip.interp_out_width(width, up)


def _table():
    """(entry, arguments, status, piece of fir_last_error) -- None: the device lookup's text.  A call
    that is wrong in two ways names the check that comes first: check_fir1d's own order, then up,
    then the sizes, then NULL x or y (only for a problem that is not empty), then, for the host
    form, the device lookup."""
    h = (ctypes.c_int32 * 3)(1, 2, 1)
    buf = np.zeros(1024, np.uint8)
    X = Y = buf.ctypes.data
    sizes = b"rows * width * up * channels"
    t = []
    for fn, tail in (("fir_interp_rows_dev", None), ("fir_interp_rows", _NO_DEV)):
        def add(rc, msg, x=None, in_dtype=0, rows=0, width=16, ch=1, hq=h, taps=3, up=2, frac=12, acc=32,
                stage=0, y=None, fn=fn, tail=tail):
            t.append((fn, (x, in_dtype, rows, width, ch, hq, taps, up, frac, acc, stage, y, tail), rc, msg))
        # empty problems: FIR_OK without a device, NULL pointers and all
        add(0, b"")
        add(0, b"", rows=5, width=0)
        add(0, b"", rows=5, width=0, up=2**31 - 1)
        add(0, b"", rows=0, width=1 << 40, up=1000)
        add(0, b"", rows=0, width=1 << 40, up=1, ch=3, in_dtype=1, stage=1)
        # check_fir1d's checks, in its order, with its texts
        add(EINVAL, b"in_dtype must be FIR_IN_U8 or FIR_IN_I16", in_dtype=7, stage=5, up=0)
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=5, rows=-1, up=0)
        add(EINVAL, b"rows and width must be >= 0", rows=-1, ch=0, up=0)
        add(EINVAL, b"rows and width must be >= 0", width=-1, up=-1)
        add(EINVAL, b"channels must be >= 1", ch=0, hq=None, up=0)
        add(EINVAL, b"hq must not be NULL", hq=None, taps=0, up=0)
        add(EINVAL, b"taps must be in [1, ", taps=0, frac=0, up=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", frac=0, up=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", acc=0, up=-9, rows=1)
        # then up
        add(EINVAL, b"up must be >= 1", up=0, rows=1)
        add(EINVAL, b"up must be >= 1", up=-2)
        add(EINVAL, b"up must be >= 1", up=0, rows=1 << 40, width=1 << 40)  # before the sizes
        # then the sizes, with a text of their own: rows * width * up * channels * 4 past int64
        add(EINVAL, sizes, rows=1 << 40, width=1 << 40)
        add(EINVAL, sizes, rows=1, width=1 << 61, up=1)          # * 4
        add(EINVAL, sizes, rows=1, width=1 << 59, up=4)          # the factor up
        add(EINVAL, sizes, rows=1 << 20, width=1 << 20, up=1 << 20, ch=2, in_dtype=1)
        add(EINVAL, sizes, rows=1, width=1 << 59, up=2, ch=2, in_dtype=1, x=X, y=Y)
        add(0, b"", rows=0, width=1 << 62, up=4)                 # no outputs: the product is 0 whatever width * up is
        # then the pointers, only when something would be computed
        add(EINVAL, b"x and y must not be NULL", rows=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, x=X)
        add(EINVAL, b"x and y must not be NULL", rows=1, y=Y, up=16)
        if tail is not None:  # the host form gets as far as the device lookup
            add(ENODEV, None, rows=1, x=X, y=Y)
            add(ENODEV, None, rows=2, x=X, y=Y, up=16, in_dtype=1, stage=1)
    return t, buf


def test_refusal_order_of_both_entries(lib):
    count = ctypes.c_int32(-1)
    have = lib.fir_device_count(ctypes.byref(count)) == 0 and count.value > 0
    nodev = b"out of range" if have else b"no HIP device available"
    table, keep = _table()
    assert {fn for fn, *_ in table} == {"fir_interp_rows", "fir_interp_rows_dev"}
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
        for rows, width, up in ((0, 0, 1), (0, 4096, 4), (7, 0, 4), (7, 0, 1), (0, 1, 1000)):
            rc = lib.fir_interp_rows_dev(None, in_dtype, rows, width, ch, h, 5, up, 12, 32, stage, None, None)
            assert rc == 0, (in_dtype, ch, stage, rows, width, up, lib.fir_last_error())
            rc = lib.fir_interp_rows(None, in_dtype, rows, width, ch, h, 5, up, 12, 32, stage, None, _NO_DEV)
            assert rc == 0, (in_dtype, ch, stage, rows, width, up, lib.fir_last_error())


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a call the host layer must refuse")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(fir_hip, "lib", lambda: _NoLibrary())
    x = np.zeros((4, 16), np.uint8)
    h = [1, 2, 1]
    for up in (0, -1, -16):
        with pytest.raises(fir_hip.FirHipError, match="up must be >= 1"):
            fir_hip.fir1d_fixed_rows_interp(x, h, up)
    with pytest.raises(fir_hip.FirHipError, match="dtype"):
        fir_hip.fir1d_fixed_rows_interp(x.astype(np.float32), h, 2)
    with pytest.raises(fir_hip.FirHipError, match="channels"):
        fir_hip.fir1d_fixed_rows_interp(np.zeros((4, 15), np.int16), h, 2, channels=2)
    with pytest.raises(fir_hip.FirHipError, match="channels"):
        fir_hip.fir1d_fixed_rows_interp(x, h, 2, channels=0)
    for taps, text in (([], "non-empty 1-D"), ([[1, 2]], "non-empty 1-D"), ([1, 2**31], "fit in int32")):
        with pytest.raises(fir_hip.FirHipError, match=text):
            fir_hip.fir1d_fixed_rows_interp(x, taps, 2)
    # out=: wrong dtype, wrong shape (the input's shape is wrong too), layout, not an array, read-only
    ro = np.zeros((4, 64), np.uint8)
    ro.flags.writeable = False
    bad = [np.zeros((4, 64), np.int32), np.zeros((4, 16), np.uint8), np.zeros((4, 63), np.uint8),
           np.zeros((3, 64), np.uint8), np.zeros((64, 4), np.uint8).T, [[0] * 64] * 4, ro]
    for out in bad:
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            fir_hip.fir1d_fixed_rows_interp(x, h, 4, out=out)
    with pytest.raises(fir_hip.FirHipError, match="out must be int32"):
        fir_hip.fir1d_fixed_rows_interp(x, h, 4, out_stage=fir_hip.OUT_I32, out=np.zeros((4, 64), np.uint8))
    big = np.zeros(4 * 64 + 64, np.uint8)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # x inside out
        fir_hip.fir1d_fixed_rows_interp(big[32:96].reshape(4, 16), h, 4, out=big[:256].reshape(4, 64))
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # in place is refused even at up = 1
        fir_hip.fir1d_fixed_rows_interp(x.reshape(-1), h, 1, out=x.reshape(-1))
    x16 = np.zeros(256, np.int16)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # a partial overlap through a view
        fir_hip.fir1d_fixed_rows_interp(x16[:32], h, 2, out_stage=fir_hip.OUT_I32, out=x16.view(np.int32)[8:72])
    # a complex row counts frames: 16 int16 = 8 frames -> 32 frames = 64 values
    with pytest.raises(fir_hip.FirHipError, match=r"shape \(4, 64\)"):
        fir_hip.fir1d_fixed_rows_interp(np.zeros((4, 16), np.int16), h, 4, channels=2, out_stage=fir_hip.OUT_I32,
                                        out=np.zeros((4, 32), np.int32))
