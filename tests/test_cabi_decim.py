"""The decimating FIR's C ABI and host layer, without a GPU: the three fir_decim_* symbols, the
out_width rule, the order and texts of the refusals of both entries, empty problems, and the
Python layer's own refusals (each before any library call)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip

EINVAL, ENODEV = 1, 3
_NO_DEV = 1 << 20  # a device index no machine has: the device lookup itself refuses it
SYMBOLS = ("fir_decim_out_width", "fir_decim_rows", "fir_decim_rows_dev")


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
    assert fir_hip.EXPORTS["fir_decim_out_width"][0] is ctypes.c_int64
    assert len(fir_hip.EXPORTS["fir_decim_rows"][1]) == len(fir_hip.EXPORTS["fir_decim_rows_dev"][1]) == 14
    assert lib.fir_abi_version() == 6  # additive: the ABI number stays


OUT_WIDTH = [
    # width, decim, phase, out_width
    (0, 1, 0, 0), (1, 1, 0, 1), (17, 1, 0, 17),
    (16, 2, 0, 8), (16, 2, 1, 8), (17, 2, 0, 9), (17, 2, 1, 8),
    (10, 3, 0, 4), (10, 3, 1, 3), (10, 3, 2, 3),
    (5, 8, 0, 1), (5, 8, 4, 1), (5, 8, 5, 0), (5, 8, 7, 0),  # phase >= width: nothing kept
    (1, 1000, 0, 1), (1, 1000, 1, 0), (0, 4, 3, 0),
    (1 << 62, 1, 0, 1 << 62), ((1 << 62) + 1, 2, 0, (1 << 61) + 1), ((1 << 62) + 1, 2, 1, 1 << 61),
    ((1 << 62) - 1, (1 << 31) - 1, (1 << 31) - 2, ((1 << 62) - 1 - ((1 << 31) - 2) + (1 << 31) - 2) // ((1 << 31) - 1)),
    (2**63 - 1, 2**31 - 1, 0, (2**63 - 1 + 2**31 - 2) // (2**31 - 1)),
    # bad arguments
    (16, 0, 0, -1), (16, -3, 0, -1), (16, 4, -1, -1), (16, 4, 4, -1), (16, 1, 1, -1), (-1, 2, 0, -1),
]


@pytest.mark.parametrize("width,decim,phase,want", OUT_WIDTH)
def test_out_width_table(lib, width, decim, phase, want):
    assert lib.fir_decim_out_width(width, decim, phase) == want
    if want >= 0:
        assert fir_hip.decim_out_width(width, decim, phase) == want
        if width <= 1 << 16:
            assert want == len(range(width)[phase::decim])
    else:
        with pytest.raises(fir_hip.FirHipError):
            fir_hip.decim_out_width(width, decim, phase)


def _table():
    """(entry, arguments, status, piece of fir_last_error) -- None: the device lookup's text.  A call
    that is wrong in two ways names the check that comes first: check_fir1d's own order, then
    decim, then phase, then NULL x or y (only for a problem that is not empty), then, for the host
    form, the device lookup."""
    h = (ctypes.c_int32 * 3)(1, 2, 1)
    buf = np.zeros(1024, np.uint8)
    X = Y = buf.ctypes.data
    t = []
    for fn, tail in (("fir_decim_rows_dev", None), ("fir_decim_rows", _NO_DEV)):
        def add(rc, msg, x=None, in_dtype=0, rows=0, width=16, ch=1, hq=h, taps=3, decim=2, phase=0, frac=12, acc=32,
                stage=0, y=None, fn=fn, tail=tail):
            t.append((fn, (x, in_dtype, rows, width, ch, hq, taps, decim, phase, frac, acc, stage, y, tail), rc, msg))
        # empty problems: FIR_OK without a device, NULL pointers and all
        add(0, b"")
        add(0, b"", rows=5, width=0)
        add(0, b"", rows=5, width=3, decim=8, phase=3)  # phase >= width: out_width 0
        add(0, b"", rows=0, width=1 << 40, decim=1000, phase=999)
        # check_fir1d's checks, in its order, with its texts
        add(EINVAL, b"in_dtype must be FIR_IN_U8 or FIR_IN_I16", in_dtype=7, stage=5, decim=0)
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=5, rows=-1, decim=0)
        add(EINVAL, b"rows and width must be >= 0", rows=-1, ch=0, decim=0)
        add(EINVAL, b"rows and width must be >= 0", width=-1, phase=-1)
        add(EINVAL, b"channels must be >= 1", ch=0, hq=None, decim=0)
        add(EINVAL, b"hq must not be NULL", hq=None, taps=0, decim=0)
        add(EINVAL, b"taps must be in [1, ", taps=0, frac=0, decim=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", frac=0, decim=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", acc=0, phase=9, rows=1)
        # then decim, then phase
        add(EINVAL, b"decim must be >= 1", decim=0, phase=-1, rows=1)
        add(EINVAL, b"decim must be >= 1", decim=-2)
        add(EINVAL, b"phase must be in [0, decim)", phase=2, rows=1)
        add(EINVAL, b"phase must be in [0, decim)", phase=-1)
        add(EINVAL, b"phase must be in [0, decim)", decim=1, phase=1, rows=1, x=X)
        # then the pointers, only when something would be computed
        add(EINVAL, b"x and y must not be NULL", rows=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, x=X)
        add(EINVAL, b"x and y must not be NULL", rows=1, y=Y, decim=16, phase=15)
        if tail is not None:  # the host form gets as far as the device lookup
            add(ENODEV, None, rows=1, x=X, y=Y)
            add(ENODEV, None, rows=2, x=X, y=Y, decim=16, phase=15, in_dtype=1, stage=1)
    return t, buf


def test_refusal_order_of_both_entries(lib):
    count = ctypes.c_int32(-1)
    have = lib.fir_device_count(ctypes.byref(count)) == 0 and count.value > 0
    nodev = b"out of range" if have else b"no HIP device available"
    table, keep = _table()
    assert {fn for fn, *_ in table} == {"fir_decim_rows", "fir_decim_rows_dev"}
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
        for rows, width, decim, phase in ((0, 0, 1, 0), (0, 4096, 4, 1), (7, 0, 4, 3), (7, 3, 4, 3), (7, 1, 1000, 1)):
            rc = lib.fir_decim_rows_dev(None, in_dtype, rows, width, ch, h, 5, decim, phase, 12, 32, stage, None, None)
            assert rc == 0, (in_dtype, ch, stage, rows, width, decim, phase, lib.fir_last_error())


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a call the host layer must refuse")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(fir_hip, "lib", lambda: _NoLibrary())
    x = np.zeros((4, 64), np.uint8)
    h = [1, 2, 1]
    for decim, phase in ((0, 0), (-1, 0), (4, 4), (4, -1), (1, 1)):
        with pytest.raises(fir_hip.FirHipError, match="decim|phase"):
            fir_hip.fir1d_fixed_rows_decim(x, h, decim, phase)
    with pytest.raises(fir_hip.FirHipError, match="dtype"):
        fir_hip.fir1d_fixed_rows_decim(x.astype(np.float32), h, 2)
    with pytest.raises(fir_hip.FirHipError, match="channels"):
        fir_hip.fir1d_fixed_rows_decim(np.zeros((4, 63), np.int16), h, 2, channels=2)
    # out=: wrong dtype, wrong shape (the full-rate shape is wrong too), layout, read-only, overlap
    ro = np.zeros((4, 16), np.uint8)
    ro.flags.writeable = False
    bad = [np.zeros((4, 16), np.int32), np.zeros((4, 64), np.uint8), np.zeros((4, 15), np.uint8),
           np.zeros((16, 4), np.uint8).T, [[0] * 16] * 4, ro]
    for out in bad:
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            fir_hip.fir1d_fixed_rows_decim(x, h, 4, 1, out=out)
    with pytest.raises(fir_hip.FirHipError, match="out must be int32"):
        fir_hip.fir1d_fixed_rows_decim(x, h, 4, 1, out_stage=fir_hip.OUT_I32, out=np.zeros((4, 16), np.uint8))
    with pytest.raises(fir_hip.FirHipError, match="overlap"):
        fir_hip.fir1d_fixed_rows_decim(x, h, 4, out=x.reshape(-1)[:64].reshape(4, 16))
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # in place is refused: the shapes differ, rows move
        fir_hip.fir1d_fixed_rows_decim(x.reshape(-1), h, 1, out=x.reshape(-1))
    x16 = np.zeros(128, np.int16)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # a partial overlap through a view
        fir_hip.fir1d_fixed_rows_decim(x16[:64], h, 2, out_stage=fir_hip.OUT_I32, out=x16.view(np.int32)[16:48])
    # a complex row counts frames: 64 int16 = 32 frames -> 8 kept frames = 16 values
    with pytest.raises(fir_hip.FirHipError, match=r"shape \(4, 16\)"):
        fir_hip.fir1d_fixed_rows_decim(np.zeros((4, 64), np.int16), h, 4, channels=2, out_stage=fir_hip.OUT_I32,
                                       out=np.zeros((4, 8), np.int32))
