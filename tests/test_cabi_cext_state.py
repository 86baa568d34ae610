"""The three extension libraries (libfir_cdecim.so, libfir_cinterp.so, libfir_cresample.so) in one
process, without a GPU: they are built over one header-only host layer (csrc_cext/) and must share
none of its state.  A refusal by one library leaves the other two libraries' last-error texts byte
for byte what they were, and a call that one library records leaves the other two records alone."""
from __future__ import annotations

import ctypes

import pytest

import fir_hip
from fir_hip import cdecim, cinterp, cresample

OK, EINVAL = 0, 1
_NO_DEV = 1 << 20  # a device index no machine has: an empty problem must not get as far as looking
I32 = fir_hip.OUT_I32
H = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)  # 3 taps of (hr, hi)
MODS = {"cdecim": cdecim, "cinterp": cinterp, "cresample": cresample}
# the rate arguments of a legal call, per library, in its entries' order
RATES = {"cdecim": (2, 0), "cinterp": (3,), "cresample": (3, 2, 0)}
# (the rate arguments of a refused call, the text of the refusal)
REFUSED = {"cdecim": ((0, 0), b"decim must be >= 1"),            # decim = 0
           "cinterp": ((0,), b"up must be >= 1"),                # up = 0
           "cresample": ((3, 2, 2), b"phase must be in [0, decim)")}  # phase = decim


@pytest.fixture(scope="module")
def libs():
    for mod in MODS.values():
        if not mod.lib_path().exists():
            pytest.fail(f"{mod.lib_path()} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return {name: mod.lib() for name, mod in MODS.items()}


def _entry(libs, name, kind):
    return getattr(libs[name], f"fir_cplx_{name[1:]}_{kind}")


def _last_error(libs, name) -> bytes:
    return getattr(libs[name], f"fir_{name}_last_error")()


def _rows_dev(libs, name, rates, hq=H):
    """fir_cplx_*_rows_dev of one frame row that no check lets through to a device: x and y are NULL."""
    return _entry(libs, name, "rows_dev")(None, 1, 16, hq, 3, *rates, 12, 32, I32, None, None)


def _last_launch(libs, name):
    r, b = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _entry(libs, name, "last_launch")(ctypes.byref(r), ctypes.byref(b)) == OK
    return r.value, b.value


def test_a_refusal_leaves_the_other_libraries_error_texts_alone(libs):
    for name in MODS:  # every library starts from a text of its own making
        assert _rows_dev(libs, name, RATES[name], hq=None) == EINVAL
        assert _last_error(libs, name) == b"hq must not be NULL"
    for name, (rates, text) in REFUSED.items():
        others = {o: _last_error(libs, o) for o in MODS if o != name}
        assert all(others.values())
        assert _rows_dev(libs, name, rates) == EINVAL
        assert text in _last_error(libs, name) and _last_error(libs, name) != b"hq must not be NULL"
        assert {o: _last_error(libs, o) for o in others} == others, name


def test_an_empty_call_leaves_the_other_libraries_launch_records_alone(libs):
    for name in MODS:
        others = {o: _last_launch(libs, o) for o in MODS if o != name}
        # rows = 0, NULL x and y: FIR_OK, and no device is looked at
        assert _entry(libs, name, "rows")(None, 0, 16, H, 3, *RATES[name], 12, 32, I32, None, _NO_DEV) == OK
        assert _last_launch(libs, name) == (MODS[name].ROUTE_NONE, 0)
        assert {o: _last_launch(libs, o) for o in others} == others, name
