"""The five libraries (libfir_hip.so and the four extension libraries libfir_cdecim.so,
libfir_cinterp.so, libfir_cresample.so, libfir_cstream.so) in one process, without a GPU.  The four
extension libraries are built over one header-only host layer (csrc_cext/) and must share none of its
state: a refusal by one library leaves the other libraries' last-error texts byte for byte what they
were (the first library's too), and a call that one library records leaves the other records alone."""
from __future__ import annotations

import ctypes

import pytest

import fir_hip
from fir_hip import cdecim, cinterp, cresample, cstream

OK, EINVAL = 0, 1
_NO_DEV = 1 << 20  # a device index no machine has: an empty problem must not get as far as looking
I32 = fir_hip.OUT_I32
H = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)  # 3 taps of (hr, hi)
MODS = {"cdecim": cdecim, "cinterp": cinterp, "cresample": cresample, "cstream": cstream}
# the rate arguments of a legal call, per library, in its entries' order
RATES = {"cdecim": (2, 0), "cinterp": (3,), "cresample": (3, 2, 0), "cstream": (2, 0)}
# (the rate arguments of a refused call, the text of the refusal)
REFUSED = {"cdecim": ((0, 0), b"decim must be >= 1"),
           "cinterp": ((0,), b"up must be >= 1"),
           "cresample": ((3, 2, 2), b"phase must be in [0, decim)"),
           "cstream": ((4, 4), b"phase must be in [0, decim)")}


@pytest.fixture(scope="module")
def libs():
    for mod in MODS.values():
        if not mod.lib_path().exists():
            pytest.fail(f"{mod.lib_path()} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return {name: mod.lib() for name, mod in MODS.items()}


def _last_error(libs, name) -> bytes:
    return getattr(libs[name], f"fir_{name}_last_error")()


def _call(libs, name, rates, rows=1, hq=H, device=None):
    """The library's entry on one row of 16 frames that no check lets through to a device: x and y are
    NULL (``device``: the host form, else the device-pointer form)."""
    if name == "cstream":
        fn = libs[name].fir_cplx_stream_block if device is not None else libs[name].fir_cplx_stream_block_dev
        return fn(None, None, rows, 16, hq, 3, *rates, 12, 32, I32, None, None, device)
    fn = getattr(libs[name], f"fir_cplx_{name[1:]}_rows" + ("" if device is not None else "_dev"))
    return fn(None, rows, 16, hq, 3, *rates, 12, 32, I32, None, device)


def _last_launch(libs, name):
    r, b = ctypes.c_int(-1), ctypes.c_int(-1)
    entry = "fir_cplx_stream_last_launch" if name == "cstream" else f"fir_cplx_{name[1:]}_last_launch"
    assert getattr(libs[name], entry)(ctypes.byref(r), ctypes.byref(b)) == OK
    return r.value, b.value


def test_a_refusal_leaves_the_other_libraries_error_texts_alone(libs):
    first = fir_hip.lib()
    assert first.fir_cplx_rows_dev(None, 1, 16, H, 3, 0, 32, I32, None, None) == EINVAL  # the first library's own text
    first_text = bytes(first.fir_last_error())
    assert b"frac_bits" in first_text
    for name in MODS:  # every library starts from a text of its own making
        assert _call(libs, name, RATES[name], hq=None) == EINVAL
        assert _last_error(libs, name) == b"hq must not be NULL"
    for name, (rates, text) in REFUSED.items():
        others = {o: _last_error(libs, o) for o in MODS if o != name}
        assert all(others.values())
        assert _call(libs, name, rates) == EINVAL
        assert text in _last_error(libs, name) and _last_error(libs, name) != b"hq must not be NULL"
        assert {o: _last_error(libs, o) for o in others} == others, name
        assert bytes(first.fir_last_error()) == first_text, name


def test_an_empty_call_leaves_the_other_libraries_launch_records_alone(libs):
    for name in MODS:
        others = {o: _last_launch(libs, o) for o in MODS if o != name}
        # rows = 0, NULL x and y: FIR_OK, and no device is looked at
        assert _call(libs, name, RATES[name], rows=0, device=_NO_DEV) == OK
        assert _last_launch(libs, name) == (MODS[name].ROUTE_NONE, 0)
        assert {o: _last_launch(libs, o) for o in others} == others, name
