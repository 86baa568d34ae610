"""The decimating complex-tap FIR's C ABI (include/fir_cdecim.h, libfir_cdecim.so) and host layer,
without a GPU: the exported symbols, the source id, out_width, the order and texts of the refusals of
both entries (the restated check_fir1d texts held against libfir_hip.so's own), the dispatch against
tests/cdecim_cases.predicted_route, and the Python layer's own refusals (each before any library
call)."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cdecim_cases as dc
import fir_hip
from fir_hip import cdecim

EINVAL, ENODEV = 1, 3
_NO_DEV = 1 << 20  # a device index no machine has: the device lookup itself refuses it
ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fir_cdecim.h"
ENTRIES = ("fir_cplx_decim_rows_dev", "fir_cplx_decim_rows")


def _declared() -> set[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"^\s*(?!typedef\b)(?:const\s+)?\w+\s*\*?\s*(\w+)\s*\(", text, flags=re.M))


@pytest.fixture(scope="module")
def lib():
    if not cdecim.lib_path().exists():
        pytest.fail(f"{cdecim.lib_path()} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return cdecim.lib()


def test_library_exports_exactly_what_the_header_declares(lib):
    assert _declared() == set(cdecim.EXPORTS) and len(cdecim.EXPORTS) == 7
    raw = ctypes.CDLL(str(cdecim.lib_path()))
    for name in _declared():
        assert hasattr(raw, name), name
    # nothing else of the fir_ name space leaves the library, and nothing of the first library's
    out = subprocess.run(["nm", "-D", "--defined-only", str(cdecim.lib_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.split()[-1].startswith("fir")}
    assert exported == set(cdecim.EXPORTS)
    assert lib.fir_cdecim_build_id().decode() == cdecim.build_id()
    assert "fir1d_fixed_rows_cplx_decim" in fir_hip.__all__ and not set(cdecim.EXPORTS) & set(fir_hip.EXPORTS)


def test_importing_fir_hip_does_not_load_the_extension_library():
    probe = ("import sys; import fir_hip; "
             "maps = open('/proc/self/maps').read(); "
             "assert 'fir_hip.cdecim' not in sys.modules and 'libfir_cdecim' not in maps, 'loaded on import'; "
             "fir_hip.lib(); assert 'libfir_cdecim' not in open('/proc/self/maps').read(); "
             "from fir_hip import cdecim; assert 'libfir_cdecim' not in open('/proc/self/maps').read(); "
             "cdecim.lib(); maps = open('/proc/self/maps').read(); assert 'libfir_cdecim' in maps; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(Path(fir_hip.__file__).resolve().parents[1])] +
                                                      ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    r = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_the_extension_library_does_not_need_the_first():
    out = subprocess.run(["readelf", "-d", str(cdecim.lib_path())], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in out and "libfir_hip" not in out


def test_stale_library_is_refused(tmp_path):
    """The library carries the id of the sources it was built from; the loader refuses it when the
    sources beside it differ -- one flipped byte in each kind of source in turn, no rebuild."""
    pkg = Path(fir_hip.__file__).resolve().parents[1]  # warmup-fir-filter_amd/
    dst = tmp_path / "tree" / pkg.name
    shutil.copytree(pkg / "fir_hip", dst / "fir_hip", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(pkg / "csrc_cdecim", dst / "csrc_cdecim", ignore=shutil.ignore_patterns("build"))
    shutil.copytree(pkg / "csrc_cext", dst / "csrc_cext")
    (dst / "csrc").mkdir()
    for name in ("fir_common.h", "fir_dispatch.h"):
        shutil.copy(pkg / "csrc" / name, dst / "csrc" / name)
    (dst.parent / "include").mkdir()
    for name in ("fir_cdecim.h", "fir_hip.h"):
        shutil.copy(ROOT / "include" / name, dst.parent / "include" / name)
    env = {k: v for k, v in os.environ.items() if k != "FIR_HIP_LIB"}
    probe = (f"import sys; sys.path.insert(0, {str(dst)!r}); from fir_hip import cdecim; cdecim.lib(); "
             "print(cdecim.build_id())")

    ok = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert ok.stdout.strip() == cdecim.build_id()

    for src in (dst / "csrc_cdecim" / "fir1d_cplx_decim.hip", dst / "csrc_cdecim" / "cdecim.h", dst / "csrc_cdecim" / "Makefile",
                dst.parent / "include" / "fir_cdecim.h", dst / "csrc" / "fir_common.h", dst / "csrc" / "fir_dispatch.h",
                *sorted((dst / "csrc_cext").iterdir())):
        data = bytearray(src.read_bytes())
        i = next(k for k, c in enumerate(data) if chr(c).isalpha())
        data[i] ^= 0x20  # the case of the first letter, inside the leading comment
        src.write_bytes(bytes(data))
        bad = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
        assert bad.returncode != 0, src
        assert "built from other sources" in bad.stderr, (src, bad.stderr)
        data[i] ^= 0x20
        src.write_bytes(bytes(data))
    again = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
    assert again.returncode == 0, again.stderr


def test_out_width(lib):
    f = lib.fir_cplx_decim_out_width
    for D in range(1, 18):
        for phase in range(D):
            for width in range(0, 41):
                assert f(width, D, phase) == len(range(phase, width, D)) == cdecim.out_width(width, D, phase)
    for args in ((10, 0, 0), (10, -1, 0), (10, 4, -1), (10, 4, 4), (10, 4, 5), (-1, 1, 0), (-(1 << 63), 3, 1), (0, 0, 0)):
        assert f(*args) == -1, args
    top = (1 << 63) - 1
    assert f(top, 1, 0) == top and f(top, 2, 0) == 1 << 62 and f(top, 2, 1) == (1 << 62) - 1
    assert f(top, (1 << 31) - 1, (1 << 31) - 2) == len(range((1 << 31) - 2, top, (1 << 31) - 1))
    for bad in ((10, 0, 0), (10, 3, 3), (10, 3, -1), (-1, 2, 0)):
        with pytest.raises(fir_hip.FirHipError):
            cdecim.out_width(*bad)


def _table():
    """(entry, arguments, status, piece of fir_cdecim_last_error) -- None: the device lookup's text.  A
    call that is wrong in two ways names the check that comes first: fir_cplx_rows_dev's own order
    (the stage, rows and width, hq, taps, frac_bits and acc_bits), then decim, then phase, then the
    sizes, then NULL x or y (only for a problem that is not empty), then, for the host form, the
    device lookup."""
    h = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    buf = np.zeros(1024, np.uint8)
    X = Y = buf.ctypes.data
    sizes = b"rows * width * 2 * 4 bytes must fit in int64"
    t = []
    for fn, tail in (("fir_cplx_decim_rows_dev", None), ("fir_cplx_decim_rows", _NO_DEV)):
        def add(rc, msg, x=None, rows=0, width=16, hq=h, taps=3, decim=2, phase=0, frac=12, acc=32, stage=1, y=None,
                fn=fn, tail=tail):
            t.append((fn, (x, rows, width, hq, taps, decim, phase, frac, acc, stage, y, tail), rc, msg))
        # empty problems: FIR_OK without a device, NULL pointers and all
        add(0, b"")
        add(0, b"", rows=5, width=0)
        add(0, b"", rows=0, width=1 << 40, stage=0)
        add(0, b"", rows=1 << 40, width=0, acc=64, frac=40)
        add(0, b"", rows=7, width=3, decim=4, phase=3)            # phase >= width: out_width 0
        add(0, b"", rows=1 << 20, width=16, decim=1 << 30, phase=16)
        # fir_cplx_rows_dev's checks, in its order, with its texts
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=5, rows=-1, hq=None)
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=-1, taps=0, decim=0)
        add(EINVAL, b"rows and width must be >= 0", rows=-1, hq=None, taps=0)
        add(EINVAL, b"rows and width must be >= 0", width=-1, frac=0, phase=-1)
        add(EINVAL, b"hq must not be NULL", hq=None, taps=0, frac=0)
        add(EINVAL, b"taps must be in [1, 1073741824]", taps=0, frac=0)
        add(EINVAL, b"taps must be in [1, 1073741824]", taps=-3, rows=1 << 40, width=1 << 40, decim=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", frac=0, rows=1 << 40, width=1 << 40, decim=-1)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", acc=0, rows=1, phase=9)
        # then decim, then phase
        add(EINVAL, b"decim must be >= 1", decim=0)
        add(EINVAL, b"decim must be >= 1", decim=-2, phase=-1, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"decim must be >= 1", decim=0, phase=0, rows=1)
        add(EINVAL, b"phase must be in [0, decim)", phase=2)
        add(EINVAL, b"phase must be in [0, decim)", phase=-1, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"phase must be in [0, decim)", decim=1, phase=1, rows=1)
        # then the sizes, with a text of their own
        add(EINVAL, sizes, rows=1 << 40, width=1 << 40)
        add(EINVAL, sizes, rows=1, width=1 << 60)                    # * 2 * 4
        add(EINVAL, sizes, rows=1 << 30, width=1 << 30, x=X, y=Y)
        add(EINVAL, sizes, rows=1 << 62, width=2, decim=16, phase=15)
        # then the pointers, only when something would be computed
        add(EINVAL, b"x and y must not be NULL", rows=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, x=X)
        add(EINVAL, b"x and y must not be NULL", rows=1, y=Y, stage=0)
        add(EINVAL, b"x and y must not be NULL", rows=1 << 29, width=1 << 30)  # the largest legal size
        if tail is not None:  # the host form gets as far as the device lookup
            add(ENODEV, None, rows=1, x=X, y=Y)
            add(ENODEV, None, rows=2, x=X, y=Y, stage=0, acc=64, decim=3, phase=2)
    return t, buf


def test_refusal_order_of_both_entries(lib):
    n = ctypes.c_int(0)
    first = fir_hip.lib()
    have = first.fir_device_count(ctypes.byref(n)) == 0 and n.value > 0
    nodev = b"out of range" if have else b"no HIP device available"
    table, keep = _table()
    assert {fn for fn, *_ in table} == set(ENTRIES)
    bad = []
    for fn, args, want, msg in table:
        rc = getattr(lib, fn)(*args)
        err = lib.fir_cdecim_last_error()
        if rc != want or (want and (nodev if msg is None else msg) not in err):
            bad.append((fn, args, want, msg, rc, err))
        # the route query refuses what the entries refuse, and calls an empty problem NONE
        x, rows, width, hq, taps, decim, phase, frac, acc, stage, y, _ = args
        r = lib.fir_cplx_decim_route(x or 0, y or 0, rows, width, hq, taps, decim, phase, frac, acc, stage, None)
        if want == EINVAL and (r != -1 or msg not in lib.fir_cdecim_last_error()):
            bad.append(("route", args, -1, msg, r, lib.fir_cdecim_last_error()))
        if want == 0 and r != dc.NONE:
            bad.append(("route", args, dc.NONE, b"", r, b""))
    assert not bad, "\n".join(f"{fn}{args}: want {want} {msg!r}, got {rc} {err!r}" for fn, args, want, msg, rc, err in bad)
    del keep


def test_refusal_texts_are_the_first_librarys(lib):
    """Every refusal fir_cplx_rows also makes has, character for character, fir_cplx_rows' text: the
    check on the restated check_fir1d."""
    first = fir_hip.lib()
    h = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    base = dict(x=None, rows=1, width=16, hq=h, taps=3, frac=12, acc=32, stage=1, y=None)
    cases = [dict(stage=5), dict(stage=-1), dict(rows=-1), dict(width=-1), dict(rows=-5, width=-5), dict(hq=None),
             dict(taps=0), dict(taps=-1), dict(taps=(1 << 30) + 1), dict(frac=0), dict(acc=0), dict(frac=-3, acc=-3),
             dict(rows=1 << 40, width=1 << 40), dict(), dict(stage=7, rows=-1, hq=None, taps=0, frac=0)]
    for over in cases:
        a = dict(base, **over)
        for fn1, fn2, tail in (("fir_cplx_rows_dev", "fir_cplx_decim_rows_dev", None), ("fir_cplx_rows", "fir_cplx_decim_rows", _NO_DEV)):
            rc1 = getattr(first, fn1)(a["x"], a["rows"], a["width"], a["hq"], a["taps"], a["frac"], a["acc"], a["stage"], a["y"], tail)
            text1 = bytes(first.fir_last_error())
            rc2 = getattr(lib, fn2)(a["x"], a["rows"], a["width"], a["hq"], a["taps"], 3, 1, a["frac"], a["acc"], a["stage"], a["y"], tail)
            text2 = bytes(lib.fir_cdecim_last_error())
            assert rc1 == rc2 == EINVAL and text1 == text2 and text1, (over, fn2, rc1, rc2, text1, text2)


def test_empty_problems_need_no_device_and_launch_nothing(lib):
    h = (ctypes.c_int32 * 10)(-256, 3, -1024, 0, 6656, -7, -1024, 0, -256, 1)
    r, b = ctypes.c_int(-1), ctypes.c_int(-1)
    for stage in (0, 1):
        for rows, width, D, phase in ((0, 0, 1, 0), (0, 4096, 2, 1), (7, 0, 3, 0), (0, 1, 16, 15), (5, 9, 16, 9), (1, 1, 2, 1)):
            for acc, frac in ((32, 12), (64, 40), (8, 1)):
                rc = lib.fir_cplx_decim_rows_dev(None, rows, width, h, 5, D, phase, frac, acc, stage, None, None)
                assert rc == 0, (stage, rows, width, lib.fir_cdecim_last_error())
                rc = lib.fir_cplx_decim_rows(None, rows, width, h, 5, D, phase, frac, acc, stage, None, _NO_DEV)
                assert rc == 0, (stage, rows, width, lib.fir_cdecim_last_error())
                assert lib.fir_cplx_decim_last_launch(ctypes.byref(r), ctypes.byref(b)) == 0 and (r.value, b.value) == (0, 0)
    assert lib.fir_cplx_decim_last_launch(None, None) == 0
    assert cdecim.last_launch() == (dc.NONE, 0)


def _route(lib, x, y, rows, width, hq, D, phase=0, frac=12, acc=32, stage=1):
    h = np.ascontiguousarray(np.asarray(hq, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
    b = ctypes.c_int(-1)
    r = lib.fir_cplx_decim_route(x, y, rows, width, h.ctypes.data_as(ctypes.c_void_p), h.shape[0], D, phase, frac, acc,
                                 stage, ctypes.byref(b))
    return r, b.value


def test_route_is_the_documented_dispatch(lib):
    """fir_cplx_decim_route against predicted_route: every tap count 1..66, D in and around the fast
    range, x off 16 by 0, 4 and 8 bytes, y off by 0 and 4, rows of 4k, 4k + 1 and 4k + 2 frames against
    one row, tap values at the ends of int16 and past them, the bit widths at their thresholds, both
    stages.  The tap bucket is the smallest that holds the taps."""
    X = Y = 1 << 30
    rng = np.random.default_rng(5)
    n = 0

    def hold(*a, **k):
        nonlocal n
        n += 1
        got, want = _route(lib, *a, **k), dc.predicted_route(*a, **k)
        assert got == want, (a[:4], len(a[4]), a[5:], k, got, want)
        return got

    seen = set()
    for L in range(1, 67):
        hq = dc.taps(rng, L)
        for D in (1, 2, 3, 4, 8, 15, 16, 17):
            for xo in (0, 4, 8):
                for yo in (0, 4):
                    for rows, width in ((1, 1001), (3, 1000), (3, 1001), (3, 1002), (1, 1002)):
                        r, b = hold(X + xo, Y + yo, rows, width, hq, D, D - 1)
                        seen.add(r)
                        if r == dc.FAST:
                            assert b == min(k for k in dc.BUCKETS if k >= L) and 2 <= D <= 16 and xo == 0 and L <= 64
                        else:
                            assert b == 0
    assert seen == {dc.FAST, dc.GENERIC32}
    base = dc.taps(rng, 9)
    wide = np.full((2**16 + 9, 2), 2**31 - 1)
    wide[::2] *= -1
    for D in (1, 2, 16, 17):
        for stage in (dc.OUT_I32, dc.OUT_U8_SAT):
            for poke, at in ((32767, 0), (-32767, 1), (32768, 0), (32768, 1), (-32768, 0), (-32768, 1), (1 << 20, 0), (-(1 << 20), 1)):
                hq = base.copy()
                hq[4, at] = poke
                r, _ = hold(X, Y, 1, 4096, hq, D, 0, 12, 32, stage)
                assert (r in (dc.FAST, dc.GENERIC32)) == (abs(poke) == 32767)
            for acc, frac in ((32, 12), (33, 12), (64, 12), (32, 31), (32, 32), (31, 31), (1, 1), (63, 40), (64, 64), (128, 3)):
                r, _ = hold(X, Y, 1, 4096, base, D, 0, frac, acc, stage)
                assert (r == dc.GENERIC64) == (acc > 32 or frac > 31)
                for xo in (2, 6):  # an x that is only int16 aligned
                    assert hold(X + xo, Y, 1, 4096, base, D, 0, frac, acc, stage)[0] == dc.GENERIC64
                r, _ = hold(X, Y, 2, 150, wide, D, 0, frac, acc, stage)
                assert r == (dc.GENERIC128 if acc >= 64 else dc.GENERIC64)
                assert hold(X, Y, 2, 150, wide[:2**16 - 1], D, 0, frac, acc, stage)[0] == dc.GENERIC64
    # the grid: a row of 2^40 frames, and rows x tiles at 2^31
    tiny = [[1, 1]]
    assert hold(X, Y, 1, (1 << 40) - 4, tiny, 16)[0] == dc.FAST and hold(X, Y, 1, 1 << 40, tiny, 16)[0] == dc.GENERIC32
    assert hold(X, Y, (1 << 20) - 1, 1 << 20, tiny, 2)[0] == dc.FAST      # (2^20 - 1) rows x 2^10 tiles < 2^30
    assert hold(X, Y, 1 << 22, 1 << 20, tiny, 2)[0] == dc.GENERIC32       # 2^22 rows x 2^10 tiles = 2^32
    assert hold(X, Y, 1 << 21, 1 << 20, tiny, 2)[0] == dc.GENERIC32       # = 2^31
    assert hold(X, Y, (1 << 21) - 1, 1 << 20, tiny, 2)[0] == dc.FAST      # < 2^31
    assert n > 10000
    # the Python wrapper: a Route, and FirHipError for a refused call
    assert cdecim.route(X, Y, 1, 100, base, 4, 3) == (dc.FAST, 12) == tuple(cdecim.Route(dc.FAST, 12))
    with pytest.raises(fir_hip.FirHipError, match=r"phase must be in \[0, decim\)"):
        cdecim.route(X, Y, 1, 100, base, 4, 4)


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a call the host layer must refuse")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(cdecim, "lib", lambda: _NoLibrary())
    x = np.zeros((4, 16), np.int16)
    h = [[1, 2], [3, 4], [5, 6]]
    for f in (cdecim.fir1d_fixed_rows_cplx_decim, fir_hip.fir1d_fixed_rows_cplx_decim):
        for bad in (x.astype(np.uint8), x.astype(np.int32), x.astype(np.float32), x.astype(np.complex64), x.tolist()):
            with pytest.raises(fir_hip.FirHipError, match="x must be an int16 array"):
                f(bad, h, 2)
        with pytest.raises(fir_hip.FirHipError, match="at least one axis"):
            f(np.zeros((), np.int16), h, 2)
        for odd in (np.zeros((4, 15), np.int16), np.zeros(1, np.int16), np.zeros((2, 3, 7), np.int16)):
            with pytest.raises(fir_hip.FirHipError, match="even number of values"):
                f(odd, h, 2)
        for taps in ([1, 2, 3], [[1, 2, 3]] * 4, np.zeros((5, 3), np.int64), np.zeros((0, 2), np.int64), [], 7):
            with pytest.raises(fir_hip.FirHipError, match=r"non-empty \(taps, 2\) array"):
                f(x, taps, 2)
        with pytest.raises(fir_hip.FirHipError, match="hq must be an integer array"):
            f(x, [[1.0, 2.0]], 2)
        with pytest.raises(fir_hip.FirHipError, match="must fit in int32"):
            f(x, [[1, 2**31]], 2)
        for D, phase, text in ((0, 0, "decim must be >= 1"), (-1, 0, "decim must be >= 1"), (2, 2, "phase must be in"),
                               (2, -1, "phase must be in")):
            with pytest.raises(fir_hip.FirHipError, match=text):
                f(x, h, D, phase)
        # out=: x's leading axes x 2 * out_width, int32 (uint8 for the u8 stage)
        ro = np.zeros((4, 6), np.int32)
        ro.flags.writeable = False
        for out in (np.zeros((4, 6), np.uint8), np.zeros((4, 16), np.int32), np.zeros((4, 8), np.int32), np.zeros((4, 4), np.int32),
                    np.zeros((6, 4), np.int32).T, [[0] * 6] * 4, ro):
            with pytest.raises(fir_hip.FirHipError, match="out must"):
                f(x, h, 3, 1, out=out)  # 8 frames, phase 1, D 3: frames 1, 4, 7
        with pytest.raises(fir_hip.FirHipError, match="out must be uint8"):
            f(x, h, 3, 1, out_stage=fir_hip.OUT_U8_SAT, out=np.zeros((4, 6), np.int32))
        big = np.zeros(256, np.int16)
        with pytest.raises(fir_hip.FirHipError, match="overlap"):
            f(big[:32], h, 2, out=big.view(np.int32)[8:24])


def test_python_layer_passes_the_call_on(monkeypatch):
    """An accepted call reaches fir_cplx_decim_rows once, with rows, width in FRAMES, the taps and the
    scalars, and an output of the decimated shape."""
    calls = []

    class Rec:
        def fir_cplx_decim_rows(self, *a):
            taps = tuple((ctypes.c_int32 * (2 * a[4])).from_address(a[3].value))
            calls.append((a[1], a[2], taps) + tuple(a[4:10]) + (a[11],))
            return 0

    monkeypatch.setattr(cdecim, "lib", lambda: Rec())
    x = np.zeros((3, 5, 16), np.int16)
    y = fir_hip.fir1d_fixed_rows_cplx_decim(x, [[2**31 - 1, -2**31], [3, -4]], 3, 2, 7, 24, device=2)
    assert y.shape == (3, 5, 4) and y.dtype == np.int32
    assert calls == [(15, 8, (2**31 - 1, -2**31, 3, -4), 2, 3, 2, 7, 24, fir_hip.OUT_I32, 2)]
    y = cdecim.fir1d_fixed_rows_cplx_decim(x[..., :6], np.array([[1, 2]], np.int8), 4, 3, out_stage=fir_hip.OUT_U8_SAT)
    assert y.shape == (3, 5, 0) and y.dtype == np.uint8 and calls[-1][:2] == (15, 3)
    out = np.empty((3, 5, 16), np.int32)
    assert cdecim.fir1d_fixed_rows_cplx_decim(x, [[1, 2]], 1, out=out) is out
    import inspect
    for f in (cdecim.fir1d_fixed_rows_cplx_decim, fir_hip.fir1d_fixed_rows_cplx_decim):
        sig = inspect.signature(f)
        assert list(sig.parameters) == ["x", "hq", "decim", "phase", "frac_bits", "acc_bits", "out_stage", "device", "out"]
        assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
            phase=0, frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, device=0, out=None)
