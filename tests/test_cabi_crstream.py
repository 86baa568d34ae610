"""The streaming U/D resampling complex-tap FIR's C ABI (include/fir_crstream.h, libfir_crstream.so) and
host layer, without a GPU: the exported symbols, the source id, out_width, next_phase and hist_frames,
the order and texts of the refusals of both entries, the dispatch against
tests/crstream_cases.predicted_route for each condition of the fast route flipped alone, the tap
bucket of every (taps, up, decim, phase) of the fast route, the empty-problem rules, and the Python
layer's own refusals (each before any library call)."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import crstream_cases as rs
import fir_hip
from fir_hip import crstream

EINVAL, ENODEV = 1, 3
_NO_DEV = 1 << 20  # a device index no machine has: the device lookup itself refuses it
ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fir_crstream.h"
ENTRIES = ("fir_cplx_rstream_block_dev", "fir_cplx_rstream_block")


def _declared() -> set[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"^\s*(?!typedef\b)(?:const\s+)?\w+\s*\*?\s*(\w+)\s*\(", text, flags=re.M))


@pytest.fixture(scope="module")
def lib():
    if not crstream.lib_path().exists():
        pytest.fail(f"{crstream.lib_path()} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return crstream.lib()


def test_library_exports_exactly_what_the_header_declares(lib):
    assert _declared() == set(crstream.EXPORTS) and len(crstream.EXPORTS) == 9
    raw = ctypes.CDLL(str(crstream.lib_path()))
    for name in _declared():
        assert hasattr(raw, name), name
    # nothing else of the fir_ name space leaves the library, and nothing of the other libraries'
    out = subprocess.run(["nm", "-D", "--defined-only", str(crstream.lib_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.split()[-1].startswith("fir")}
    assert exported == set(crstream.EXPORTS)
    # nothing of the shared host layer leaves it either (internal linkage: each library its own state)
    assert not [line for line in out.stdout.splitlines() if "cext" in line]
    assert lib.fir_crstream_build_id().decode() == crstream.build_id()
    assert "fir1d_fixed_rows_cplx_resample_block" in fir_hip.__all__ and not set(crstream.EXPORTS) & set(fir_hip.EXPORTS)
    from fir_hip import cdecim, cinterp, cresample, cstream
    for other in (cdecim, cinterp, cresample, cstream):
        assert not set(crstream.EXPORTS) & set(other.EXPORTS)
    enum = re.search(r"enum \{([^}]*)\}", HEADER.read_text()).group(1)
    assert [s.strip() for s in enum.split(",")] == [f"FIR_CRSTREAM_{n} = {v}" for v, n in
                                                    enumerate(("NONE", "FAST", "GENERIC32", "GENERIC64", "GENERIC128"))]
    assert (crstream.ROUTE_NONE, crstream.ROUTE_FAST, crstream.ROUTE_GENERIC32, crstream.ROUTE_GENERIC64,
            crstream.ROUTE_GENERIC128) == (rs.NONE, rs.FAST, rs.GENERIC32, rs.GENERIC64, rs.GENERIC128)


def test_importing_fir_hip_does_not_load_the_extension_library():
    probe = ("import sys; import fir_hip; "
             "maps = open('/proc/self/maps').read(); "
             "assert 'fir_hip.crstream' not in sys.modules and 'libfir_crstream' not in maps, 'loaded on import'; "
             "fir_hip.lib(); assert 'libfir_crstream' not in open('/proc/self/maps').read(); "
             "from fir_hip import crstream; assert 'libfir_crstream' not in open('/proc/self/maps').read(); "
             "crstream.lib(); maps = open('/proc/self/maps').read(); assert 'libfir_crstream' in maps; "
             "assert 'libfir_cresample' not in maps and 'libfir_cstream' not in maps; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(Path(fir_hip.__file__).resolve().parents[1])] +
                                                      ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    r = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_the_extension_library_needs_no_other_library_of_the_project():
    out = subprocess.run(["readelf", "-d", str(crstream.lib_path())], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in out and "libfir_" not in out.replace("libfir_crstream", "")


def test_stale_library_is_refused(tmp_path):
    """The library carries the id of the sources it was built from; the loader refuses it when the
    sources beside it differ -- one flipped byte in each source in turn, every file of the shared
    csrc_cext/ included, no rebuild."""
    pkg = Path(fir_hip.__file__).resolve().parents[1]  # warmup-fir-filter_amd/
    dst = tmp_path / "tree" / pkg.name
    shutil.copytree(pkg / "fir_hip", dst / "fir_hip", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(pkg / "csrc_crstream", dst / "csrc_crstream", ignore=shutil.ignore_patterns("build"))
    shutil.copytree(pkg / "csrc_cext", dst / "csrc_cext")
    (dst / "csrc").mkdir()
    for name in ("fir_common.h", "fir_dispatch.h"):
        shutil.copy(pkg / "csrc" / name, dst / "csrc" / name)
    (dst.parent / "include").mkdir()
    for name in ("fir_crstream.h", "fir_hip.h"):
        shutil.copy(ROOT / "include" / name, dst.parent / "include" / name)
    env = {k: v for k, v in os.environ.items() if k != "FIR_HIP_LIB"}
    probe = (f"import sys; sys.path.insert(0, {str(dst)!r}); from fir_hip import crstream; crstream.lib(); "
             "print(crstream.build_id())")

    ok = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert ok.stdout.strip() == crstream.build_id()

    own = dst / "csrc_crstream"
    sources = [own / "fir1d_cplx_rstream.hip", own / "capi_crstream.hip", own / "crstream.h", own / "Makefile",
               dst.parent / "include" / "fir_crstream.h", dst / "csrc" / "fir_common.h", dst / "csrc" / "fir_dispatch.h",
               *sorted((dst / "csrc_cext").iterdir())]
    assert len(sources) == 11  # the seven of the library and the four files of csrc_cext/
    for src in sources:
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


def test_out_width_next_phase_and_hist_frames(lib):
    f, g, hf = lib.fir_cplx_rstream_out_width, lib.fir_cplx_rstream_next_phase, lib.fir_cplx_rstream_hist_frames
    for U in range(1, 18):
        for D in range(1, 18):
            for phase in range(D):
                for width in (0, 1, 2, 3, 7, 16, 41):
                    ow = len(range(phase, width * U, D))
                    assert f(width, U, D, phase) == ow == crstream.out_width(width, U, D, phase) == rs.out_width(width, U, D, phase)
                    want = phase + ow * D - width * U
                    assert g(width, U, D, phase) == want == crstream.next_phase(width, U, D, phase) == rs.next_phase(width, U, D, phase)
                    assert 0 <= want < D
    for args in ((10, 0, 2, 0), (10, 2, 0, 0), (10, -1, 2, 0), (10, 2, -1, 0), (10, 3, 4, -1), (10, 3, 4, 4), (10, 3, 4, 5),
                 (-1, 1, 1, 0), (-(1 << 63), 3, 3, 1), (0, 0, 0, 0), ((1 << 63) - 1, 2, 1, 0), (1 << 62, 2, 3, 1)):
        assert f(*args) == -1 and g(*args) == -1, args
    top = (1 << 63) - 1
    assert f(top, 1, 1, 0) == top and f(top, 1, 2, 0) == 1 << 62 and f(top, 1, 2, 1) == (1 << 62) - 1
    assert g(top, 1, 1, 0) == 0 and g(top, 1, 2, 0) == 1 and g(top, 1, 2, 1) == 0  # no overflow near 2^63
    assert f((1 << 62) - 1, 2, 3, 2) == len(range(2, (1 << 63) - 2, 3)) and g((1 << 62) - 1, 2, 3, 2) == rs.next_phase((1 << 62) - 1, 2, 3, 2)
    for L in range(1, 140):
        for U in range(1, 20):
            assert hf(L, U) == (L - 1) // U == crstream.hist_frames(L, U) == rs.hist_frames(L, U)
    assert hf(1 << 30, 1) == (1 << 30) - 1
    for bad in ((0, 1), (-1, 3), (5, 0), (5, -2)):
        assert hf(*bad) == -1
        with pytest.raises(fir_hip.FirHipError):
            crstream.hist_frames(*bad)
    for bad in ((10, 0, 2, 0), (10, 2, 0, 0), (10, 2, 3, 3), (10, 2, 3, -1), (-1, 2, 2, 0)):
        with pytest.raises(fir_hip.FirHipError):
            crstream.out_width(*bad)
        with pytest.raises(fir_hip.FirHipError):
            crstream.next_phase(*bad)


SIZES = b"width * up, rows * out_width * 2 * 4 bytes and rows * width * 4 bytes must fit in int64"
HSIZES = b"rows * ((taps - 1) / up) * 4 bytes must fit in int64"


def _table():
    """(entry, arguments, status, piece of fir_crstream_last_error) -- None: the device lookup's text.  A
    call that is wrong in two ways names the check that comes first: cext::check_head's order (the
    stage, rows and width, hq, taps, frac_bits and acc_bits), then up, decim, phase, then the sizes
    (x's and y's, then the histories'), then NULL x (rows * width > 0), then NULL y (rows * out_width >
    0), then, for the host form, the device lookup."""
    h = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    h1 = (ctypes.c_int32 * 2)(1, 2)
    buf = np.zeros(1024, np.uint8)
    X = Y = HI = HO = buf.ctypes.data
    t = []
    for fn, tail in (("fir_cplx_rstream_block_dev", None), ("fir_cplx_rstream_block", _NO_DEV)):
        def add(rc, msg, x=None, hi=None, rows=0, width=16, hq=h, taps=3, up=1, decim=2, phase=0, frac=12, acc=32, stage=1,
                y=None, ho=None, fn=fn, tail=tail):
            t.append((fn, (x, hi, rows, width, hq, taps, up, decim, phase, frac, acc, stage, y, ho, tail), rc, msg))
        # nothing to compute and no history to write: FIR_OK without a device, NULL pointers and all
        add(0, b"")
        add(0, b"", rows=0, hi=HI, ho=HO, x=X, y=Y)                # rows = 0 is a no-op
        add(0, b"", rows=5, width=0)                                # hist_out NULL: nothing is written
        add(0, b"", rows=0, width=1 << 40, stage=0, up=3)
        add(0, b"", rows=1 << 40, width=0, acc=64, frac=40)
        add(0, b"", rows=7, width=1, up=3, decim=4, phase=3, x=X)  # phase >= width * up: out_width 0, y may be NULL
        add(0, b"", rows=5, width=0, up=3, hi=HI, ho=HO)           # taps <= up: both history pointers are ignored
        add(0, b"", rows=5, width=0, up=4, hi=HI, ho=HO)
        add(0, b"", rows=5, width=1, hq=h1, taps=1, hi=HI, ho=HO, x=X, decim=3, phase=2)
        # check_head's checks, in its order, with its texts
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=5, rows=-1, hq=None)
        add(EINVAL, b"out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", stage=-1, taps=0, decim=0, up=0)
        add(EINVAL, b"rows and width must be >= 0", rows=-1, hq=None, taps=0)
        add(EINVAL, b"rows and width must be >= 0", width=-1, frac=0, phase=-1, up=0)
        add(EINVAL, b"hq must not be NULL", hq=None, taps=0, frac=0)
        add(EINVAL, b"taps must be in [1, 1073741824]", taps=0, frac=0)
        add(EINVAL, b"taps must be in [1, 1073741824]", taps=-3, rows=1 << 40, width=1 << 40, decim=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", frac=0, rows=1 << 40, width=1 << 40, decim=-1, up=0)
        add(EINVAL, b"frac_bits and acc_bits must be >= 1", acc=0, rows=1, phase=9)
        # then up, then decim, then phase
        add(EINVAL, b"up must be >= 1", up=0, decim=0, phase=-1)
        add(EINVAL, b"up must be >= 1", up=-2, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"decim must be >= 1", decim=0, phase=5)
        add(EINVAL, b"decim must be >= 1", decim=-2, phase=-1, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"phase must be in [0, decim)", phase=2)
        add(EINVAL, b"phase must be in [0, decim)", phase=-1, rows=1 << 40, width=1 << 40)
        add(EINVAL, b"phase must be in [0, decim)", decim=1, phase=1, rows=1)
        # then the sizes: width * up, y's, x's, then the histories'
        add(EINVAL, SIZES, rows=1 << 40, width=1 << 40)
        add(EINVAL, SIZES, rows=1, width=1 << 61)                     # rows * width * 4 = 2^63
        add(EINVAL, SIZES, rows=0, width=1 << 62, up=2)               # width * up = 2^63
        add(EINVAL, SIZES, rows=1, width=1 << 58, up=16, decim=1)     # rows * out_width * 8 = 2^65
        add(EINVAL, SIZES, rows=1 << 30, width=1 << 30, up=16, decim=1, x=X, y=Y)
        add(EINVAL, SIZES, rows=1 << 40, width=1 << 40, taps=1 << 30)
        add(EINVAL, HSIZES, rows=1 << 40, width=0, taps=1 << 30)
        add(EINVAL, HSIZES, rows=1 << 33, width=1, taps=(1 << 29) + 1, up=2)  # rows * H = 2^61: * 4 passes int64
        add(0, b"", rows=1 << 33, width=0, taps=1 << 29, up=2)                  # rows * H * 4 < 2^63, nothing to write
        # then the pointers: x when there are frames, then y when there are kept frames
        add(EINVAL, b"x and y must not be NULL", rows=1)
        add(EINVAL, b"x and y must not be NULL", rows=1, y=Y, stage=0)
        add(EINVAL, b"x and y must not be NULL", rows=1, x=X, up=3)
        add(EINVAL, b"x and y must not be NULL", rows=7, width=1, up=3, decim=4, phase=3, y=Y)  # no output, still NULL x
        add(EINVAL, b"x and y must not be NULL", rows=1 << 29, width=1 << 30)  # a legal size
        if tail is not None:  # the host form gets as far as the device lookup
            add(ENODEV, None, rows=1, x=X, y=Y)
            add(ENODEV, None, rows=2, x=X, y=Y, hi=HI, ho=HO, stage=0, acc=64, up=2, decim=3, phase=2)
            add(ENODEV, None, rows=5, width=0, ho=HO)                 # only the history to write: still a device
            add(ENODEV, None, rows=7, width=1, up=2, decim=4, phase=3, x=X, ho=HO)
    return t, buf


def test_refusal_order_of_both_entries(lib):
    n = ctypes.c_int(0)
    first = fir_hip.lib()
    have = first.fir_device_count(ctypes.byref(n)) == 0 and n.value > 0
    nodev = b"out of range" if have else b"no HIP device available"
    table, keep = _table()
    assert {fn for fn, *_ in table} == set(ENTRIES)
    bad = []
    r_, b_ = ctypes.c_int(-1), ctypes.c_int(-1)
    for fn, args, want, msg in table:
        rc = getattr(lib, fn)(*args)
        err = lib.fir_crstream_last_error()
        if rc != want or (want and (nodev if msg is None else msg) not in err):
            bad.append((fn, args, want, msg, rc, err))
        if want == 0:  # nothing was launched
            assert lib.fir_cplx_rstream_last_launch(ctypes.byref(r_), ctypes.byref(b_)) == 0 and (r_.value, b_.value) == (0, 0)
        # the route query refuses what the entries refuse, and reports NONE when no FIR kernel runs
        x, hi, rows, width, hq, taps, up, decim, phase, frac, acc, stage, y, ho, _ = args
        r = lib.fir_cplx_rstream_route(x or 0, hi or 0, y or 0, ho or 0, rows, width, hq, taps, up, decim, phase, frac, acc, stage, None)
        if want == EINVAL and (r != -1 or msg not in lib.fir_crstream_last_error()):
            bad.append(("route", args, -1, msg, r, lib.fir_crstream_last_error()))
        if want == 0 and r != rs.NONE:
            bad.append(("route", args, rs.NONE, b"", r, b""))
    assert not bad, "\n".join(f"{fn}{args}: want {want} {msg!r}, got {rc} {err!r}" for fn, args, want, msg, rc, err in bad)
    assert lib.fir_cplx_rstream_last_launch(None, None) == 0 and crstream.last_launch() == (rs.NONE, 0)
    del keep


def test_refusal_texts_are_the_one_shot_resamplers(lib):
    """Every refusal fir_cplx_resample_rows also makes (the head checks, the rates and the sizes it
    shares) has, character for character, that entry's text."""
    from fir_hip import cresample
    one = cresample.lib()
    h = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    base = dict(x=None, rows=1, width=16, hq=h, taps=3, up=2, decim=3, phase=1, frac=12, acc=32, stage=1, y=None)
    cases = [dict(stage=5), dict(rows=-1), dict(width=-1), dict(hq=None), dict(taps=0), dict(taps=(1 << 30) + 1), dict(frac=0),
             dict(acc=0), dict(up=0), dict(up=-1, decim=0), dict(decim=0), dict(phase=3), dict(phase=-1),
             dict(rows=1 << 40, width=1 << 40), dict(width=1 << 62), dict(), dict(stage=7, rows=-1, hq=None, taps=0, frac=0)]
    for over in cases:
        a = dict(base, **over)
        for fn1, fn2, tail in (("fir_cplx_resample_rows_dev", "fir_cplx_rstream_block_dev", None),
                               ("fir_cplx_resample_rows", "fir_cplx_rstream_block", _NO_DEV)):
            rc1 = getattr(one, fn1)(a["x"], a["rows"], a["width"], a["hq"], a["taps"], a["up"], a["decim"], a["phase"], a["frac"],
                                    a["acc"], a["stage"], a["y"], tail)
            text1 = bytes(one.fir_cresample_last_error())
            rc2 = getattr(lib, fn2)(a["x"], None, a["rows"], a["width"], a["hq"], a["taps"], a["up"], a["decim"], a["phase"],
                                    a["frac"], a["acc"], a["stage"], a["y"], None, tail)
            text2 = bytes(lib.fir_crstream_last_error())
            assert rc1 == rc2 == EINVAL and text1 == text2 and text1, (over, fn2, rc1, rc2, text1, text2)


def _route(lib, x, hi, y, ho, rows, width, hq, U, D, phase=0, frac=12, acc=32, stage=1):
    h = np.ascontiguousarray(np.asarray(hq, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
    b = ctypes.c_int(-1)
    r = lib.fir_cplx_rstream_route(x, hi, y, ho, rows, width, h.ctypes.data_as(ctypes.c_void_p), h.shape[0], U, D, phase, frac,
                                   acc, stage, ctypes.byref(b))
    return r, b.value


def test_route_is_the_documented_dispatch(lib):
    """fir_cplx_rstream_route against predicted_route, each condition of the fast route flipped alone on
    a call that is FAST without it: up and decim of 1 and 17, 129 taps, 33 taps per phase, a part of
    32768, acc_bits 33 and 64, frac_bits 32, the u8 stage, x off 16 bytes, rows of 6 frames, the grid
    bound, a history off 4 bytes -- and around them the histories NULL, given and off by 2, 4 and 8
    bytes at several rates and tap counts."""
    X = 1 << 30
    rng = np.random.default_rng(5)
    n = 0

    def hold(*a, **k):
        nonlocal n
        n += 1
        got, want = _route(lib, *a, **k), rs.predicted_route(*a, **k)
        assert got == want, (a[:6], len(a[6]), a[7:], k, got, want)
        return got

    seen = set()
    for L in (1, 2, 3, 4, 5, 9, 16, 17, 33, 64, 72, 127, 128, 129):
        hq = rs.taps(rng, L)
        for U, D in ((1, 2), (2, 1), (2, 3), (3, 2), (4, 3), (16, 15), (16, 16), (17, 3), (3, 17)):
            H = rs.hist_frames(L, U)
            for xo in (0, 4):
                for hi, ho in ((0, 0), (X, X), (X + 4, X + 8), (X + 2, X), (X, X + 6), (0, X + 2), (X + 2, 0)):
                    for rows, width in ((1, 1001), (3, 1000), (3, 6), (3, 1002)):
                        r, b = hold(X + xo, hi, X, ho, rows, width, hq, U, D, D - 1)
                        seen.add(r)
                        if r == rs.FAST:
                            assert b == rs.bucket(L, U, D, D - 1) and 2 <= U <= 16 and 2 <= D <= 16 and xo == 0 and L <= 128
                            assert H == 0 or (hi % 4 == 0 and ho % 4 == 0)
                        else:
                            assert b == 0
                        if H > 0 and (hi % 4 or ho % 4):
                            assert r == rs.GENERIC64
    assert seen == {rs.FAST, rs.GENERIC32, rs.GENERIC64}
    base = rs.taps(rng, 24)
    g32, g64 = rs.GENERIC32, rs.GENERIC64
    # one reason at a time, on a call that is FAST without it
    assert hold(X, X, X, X, 1, 4096, base, 3, 2, 1) == (rs.FAST, 8)
    assert hold(X, X, X, X, 1, 4096, base, 1, 2, 1)[0] == g32                      # up = 1
    assert hold(X, X, X, X, 1, 4096, base, 17, 2, 1)[0] == g32                     # up = 17
    assert hold(X, X, X, X, 1, 4096, base, 3, 1, 0)[0] == g32                      # decim = 1
    assert hold(X, X, X, X, 1, 4096, base, 3, 17, 1)[0] == g32                     # decim = 17
    assert hold(X, X, X, X, 1, 4096, base, 16, 16, 15) == (rs.FAST, 1)       # only phase 15 of the filter is ever met
    assert hold(X, X, X, X, 1, 4096, rs.taps(rng, 128), 4, 3, 2) == (rs.FAST, 32)
    assert hold(X, X, X, X, 1, 4096, rs.taps(rng, 129), 5, 3, 2)[0] == g32         # 129 taps (26 per phase)
    assert hold(X, X, X, X, 1, 4096, rs.taps(rng, 64), 2, 3, 2) == (rs.FAST, 32)
    assert hold(X, X, X, X, 1, 4096, rs.taps(rng, 65), 2, 3, 2)[0] == g32          # 33 taps per phase
    assert hold(X, X, X, X, 1, 4096, rs.taps(rng, 96), 3, 2, 1) == (rs.FAST, 32)
    assert hold(X, X, X, X, 1, 4096, rs.taps(rng, 97), 3, 2, 1)[0] == g32
    for poke, at in ((32767, 0), (-32767, 1), (32768, 0), (32768, 1), (-32768, 0), (-32768, 1), (1 << 20, 0)):
        hq = base.copy()
        hq[4, at] = poke
        assert (hold(X, X, X, X, 1, 4096, hq, 3, 2, 1)[0] == rs.FAST) == (abs(poke) == 32767)  # a part of 32768
        assert (hold(X, X, X, X, 1, 4096, hq, 3, 2, 1)[0] == g64) == (abs(poke) != 32767)
    for acc, frac in ((32, 12), (33, 12), (64, 12), (32, 31), (32, 32), (31, 31), (1, 1), (63, 40), (64, 64), (128, 3)):
        r, _ = hold(X, X, X, X, 1, 4096, base, 3, 2, 1, frac, acc)
        assert (r == g64) == (acc > 32 or frac > 31) and (r == rs.FAST) == (acc <= 32 and frac <= 31)
    assert hold(X, X, X, X, 1, 4096, base, 3, 2, 1, 12, 32, rs.OUT_U8_SAT)[0] == g32  # the u8 stage
    assert hold(X + 4, X, X, X, 1, 4096, base, 3, 2, 1)[0] == g32                  # x off 16 bytes
    assert hold(X + 2, X, X, X, 1, 4096, base, 3, 2, 1)[0] == g64                  # x only int16 aligned
    assert hold(X, X + 2, X, X, 1, 4096, base, 3, 2, 1)[0] == g64                  # a history off 4 bytes
    assert hold(X, X, X, X + 2, 1, 4096, base, 3, 2, 1)[0] == g64
    assert hold(X, X + 4, X, X + 12, 1, 4096, base, 3, 2, 1)[0] == rs.FAST         # 4-byte aligned is enough
    assert hold(X, X + 2, X, X + 2, 1, 4096, base[:3], 3, 2, 1) == (rs.FAST, 1)    # taps <= up: the histories are ignored
    assert hold(X, X + 2, X, X + 2, 1, 4096, base[:4], 3, 2, 1)[0] == g64          # one frame of history
    assert hold(X, X, X + 4, X, 1, 4096, base, 3, 2, 1)[0] == rs.FAST              # y at any int32 address
    assert hold(X, X, X, X, 3, 6, base, 3, 2, 1)[0] == g32                         # rows of 6 frames
    assert hold(X, X, X, X, 3, 8, base, 3, 2, 1)[0] == rs.FAST
    wide = np.full((2**16 + 9, 2), 2**31 - 1)
    wide[::2] *= -1
    for acc in (63, 64, 80):
        assert hold(X, X, X, X, 2, 150, wide, 3, 2, 0, 30, acc)[0] == (rs.GENERIC128 if acc >= 64 else g64)
        assert hold(X, X, X, X, 2, 150, wide[:2**16 - 1], 3, 2, 0, 30, acc)[0] == g64
    # the one-shot resampler's grid bound
    tiny = [[1, 1]]
    assert hold(X, 0, X, 0, 1, (1 << 40) - 4, tiny, 2, 16)[0] == rs.FAST and hold(X, 0, X, 0, 1, 1 << 40, tiny, 2, 16)[0] == g32
    per = rs.periods(2) * 2  # output frames per workgroup at 2 / 2
    assert hold(X, 0, X, 0, (1 << 21) - 1, per << 10, tiny, 2, 2)[0] == rs.FAST    # rows x groups < 2^31
    assert hold(X, 0, X, 0, 1 << 21, per << 10, tiny, 2, 2)[0] == g32              # = 2^31
    assert n > 7000
    # the Python wrapper: a Route, and FirHipError for a refused call
    assert crstream.route(X, X, X, X, 1, 100, base, 3, 2, 1) == (rs.FAST, 8) == tuple(crstream.Route(rs.FAST, 8))
    assert crstream.route(X, 0, X, 0, 1, 0, base, 3, 2, 1) == (rs.NONE, 0)
    with pytest.raises(fir_hip.FirHipError, match=r"phase must be in \[0, decim\)"):
        crstream.route(X, X, X, X, 1, 100, base, 3, 2, 2)


def test_the_tap_bucket_of_every_fast_call(lib):
    """Every (taps, up, decim, phase) with up, decim <= 16 and taps <= 128: FAST with the helper's
    bucket where at most 32 taps fall to a phase, GENERIC32 otherwise."""
    X = 1 << 30
    h = np.ones((128, 2), np.int32)
    hp = h.ctypes.data_as(ctypes.c_void_p)
    b = ctypes.c_int(-1)
    route = lib.fir_cplx_rstream_route
    n = 0
    for U in range(2, 17):
        for D in range(2, 17):
            for L in range(1, 129):
                fast = -(-L // U) <= 32
                for phase in range(D):
                    r = route(X, X, X, X, 1, 4096, hp, L, U, D, phase, 12, 32, 1, ctypes.byref(b))
                    n += 1
                    if fast:
                        assert (r, b.value) == (rs.FAST, rs.bucket(L, U, D, phase)), (L, U, D, phase, r, b.value)
                    else:
                        assert (r, b.value) == (rs.GENERIC32, 0), (L, U, D, phase, r, b.value)
    assert n == 15 * 128 * sum(range(2, 17))


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a call the host layer must refuse")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(crstream, "lib", lambda: _NoLibrary())
    x = np.zeros((4, 16), np.int16)
    h = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]]
    hist = np.zeros((4, 4), np.int16)  # H = (5 - 1) // 2
    for f in (crstream.fir1d_fixed_rows_cplx_resample_block, fir_hip.fir1d_fixed_rows_cplx_resample_block):
        for bad in (x.astype(np.uint8), x.astype(np.int32), x.astype(np.float32), x.tolist()):
            with pytest.raises(fir_hip.FirHipError, match="x must be an int16 array"):
                f(bad, None, h, 2, 3)
        with pytest.raises(fir_hip.FirHipError, match="at least one axis"):
            f(np.zeros((), np.int16), None, h, 2, 3)
        with pytest.raises(fir_hip.FirHipError, match="even number of values"):
            f(np.zeros((4, 15), np.int16), None, h, 2, 3)
        for taps in ([1, 2, 3], np.zeros((5, 3), np.int64), []):
            with pytest.raises(fir_hip.FirHipError, match=r"non-empty \(taps, 2\) array"):
                f(x, None, taps, 2, 3)
        for bad in (hist.astype(np.int32), hist.tolist(), hist.astype(np.uint16)):
            with pytest.raises(fir_hip.FirHipError, match="hist must be an int16 array"):
                f(x, bad, h, 2, 3)
        for bad in (np.zeros((4, 8), np.int16), np.zeros((3, 4), np.int16), np.zeros(4, np.int16), np.zeros((4, 2, 2), np.int16)):
            with pytest.raises(fir_hip.FirHipError, match="hist must have shape"):
                f(x, bad, h, 2, 3)
        for U, D, phase, text in ((0, 2, 0, "up must be >= 1"), (-1, 2, 0, "up must be >= 1"), (2, 0, 0, "decim must be >= 1"),
                                  (2, 2, 2, "phase must be in"), (2, 2, -1, "phase must be in")):
            with pytest.raises(fir_hip.FirHipError, match=text):
                f(x, None, h, U, D, phase)


def test_python_layer_passes_the_call_on(monkeypatch):
    """An accepted call reaches fir_cplx_rstream_block once, with rows, width in FRAMES, the taps, the
    scalars and the history (NULL for None), and returns (y, hist_out, next_phase) of the right shapes."""
    calls = []

    class Rec:
        def fir_cplx_rstream_block(self, *a):
            taps = tuple((ctypes.c_int32 * (2 * a[5])).from_address(a[4].value))
            calls.append((a[1] is None, a[2], a[3], taps) + tuple(a[5:12]) + (a[14],))
            return 0

    monkeypatch.setattr(crstream, "lib", lambda: Rec())
    x = np.zeros((3, 5, 16), np.int16)
    y, ho, p = fir_hip.fir1d_fixed_rows_cplx_resample_block(x, None, [[2**31 - 1, -2**31], [3, -4], [5, 6]], 2, 3, 2, 7, 24, device=2)
    assert y.shape == (3, 5, 2 * 5) and y.dtype == np.int32 and ho.shape == (3, 5, 2) and ho.dtype == np.int16
    assert p == rs.next_phase(8, 2, 3, 2) == 1
    assert calls == [(True, 15, 8, (2**31 - 1, -2**31, 3, -4, 5, 6), 3, 2, 3, 2, 7, 24, fir_hip.OUT_I32, 2)]
    hist = np.zeros((3, 5, 0), np.int16)
    y, ho, p = crstream.fir1d_fixed_rows_cplx_resample_block(x[..., :6], hist, np.array([[1, 2]], np.int8), 2, 4, 3,
                                                             out_stage=fir_hip.OUT_U8_SAT)
    assert y.shape == (3, 5, 2) and y.dtype == np.uint8 and ho.shape == (3, 5, 0) and p == 1 and calls[-1][:3] == (False, 15, 3)
    # rows of no frames still count: the history moves
    y, ho, p = crstream.fir1d_fixed_rows_cplx_resample_block(x[..., :0], None, [[1, 2], [3, 4], [5, 6]], 1, 4, 3)
    assert y.shape == (3, 5, 0) and ho.shape == (3, 5, 4) and p == 3 and calls[-1][:3] == (True, 15, 0)
    for f in (crstream.fir1d_fixed_rows_cplx_resample_block, fir_hip.fir1d_fixed_rows_cplx_resample_block):
        sig = inspect.signature(f)
        assert list(sig.parameters) == ["x", "hist", "hq", "up", "decim", "phase", "frac_bits", "acc_bits", "out_stage", "device"]
        assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
            phase=0, frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, device=0)
    assert set(crstream.__all__) >= {"lib", "lib_path", "build_id", "out_width", "next_phase", "hist_frames", "route", "last_launch",
                                     "Route", "ROUTE_NONE", "ROUTE_FAST", "ROUTE_GENERIC32", "ROUTE_GENERIC64", "ROUTE_GENERIC128"}
