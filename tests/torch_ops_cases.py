"""The argument contract of fir_hip.torch_ops as a table -- a test helper, not a test module.

The C ABI's ``*_dev`` entries take bare pointers and cannot know a buffer's size: for a torch
caller, ``torch_ops`` is the only place where a wrong ``out`` can be stopped before a kernel stores
through it.  ``CASES`` lists, per public entry of ``torch_ops``, one valid call (``Case.build``) and
variants of it that differ in exactly one argument (``Case.mutate``), each with the ``FirHipError``
text it must raise (``Case.error``, a regular expression) or, for a variant that must be accepted,
the C entry it must reach and every argument that entry must receive (``Case.expect``).

No case reaches the library.  ``run_case`` replaces ``torch_ops.lib`` by a ``StubLib`` whose every
attribute is a function that records its call and returns 0, so a missing check shows as a
recorded call, never as a stray store:

* a refused case passes only if ``FirHipError`` is raised with the stated text and the stub
  recorded no call;
* an accepted case passes only if exactly ``Case.ncalls`` (1; the empty problems too: torch_ops
  hands them to the C entry, which returns without a launch) calls were recorded, to the expected
  entry with the expected arguments: pointers, rows, width, channels, the tap values (read through
  the pointer at the call), filters, stage codes and the stream.

Two attributes of the stub are no launches but host-side size queries a check needs the answer of
(``fir_restore_work_bytes``, ``fir_metrics_work_bytes``): they return ``RESTORE_WORK`` and
``metrics_work(n)`` and are recorded apart (``StubLib.queries``).

The tensors of a case come from a ``Maker``.  ``Maker(standin=True)`` builds CPU tensors wrapped in
``StandIn`` (the nine attributes torch_ops reads, reporting a device of the test's choosing), so the
table runs where no GPU is (tests/test_torch_ops_contract.py); ``Maker(standin=False)`` builds real
``cuda:0`` tensors (tests/test_gpu_torch_ops_contract.py).  Either way every tensor is a view in the
middle of a larger allocation (``ROOM`` bytes on both sides), which is what lets a variant replace
``out`` alone by a tensor that overlaps the unchanged ``x`` (``Maker.alias``).  "Another device" is
always a stand-in (``cuda:1``): the machine may have one GPU.

``Case.check`` names the check of torch_ops.py a refused case pins (the check -> case record).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Callable

import numpy as np
import pytest
import torch

import fir_hip

U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
CLIP, NORMALIZE = fir_hip.RESTORE_CLIP, fir_hip.RESTORE_NORMALIZE
STREAM = 0x5150  # the stream stand-in's handle: every accepted call must pass it on
RESTORE_WORK = 1024
ROOM = 4096
SMALL_MAX_TAPS = 64  # the "more than MAX_TAPS" cases run with the limit patched down to this
I32_MAX, I32_MIN = 2**31 - 1, -2**31


def metrics_work(n: int) -> int:
    return 256 + 8 * int(n)


class Stream:
    cuda_stream = STREAM


class StandIn:
    """What torch_ops reads of a tensor, over a real tensor ``t``, on a device of the test's choosing."""

    def __init__(self, t: torch.Tensor, device):
        self.t, self.device = t, torch.device(device)
        self.shape, self.dtype, self.is_cuda = t.shape, t.dtype, self.device.type == "cuda"

    def is_contiguous(self):
        return self.t.is_contiguous()

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return self.t.numel()

    def element_size(self):
        return self.t.element_size()

    def dim(self):
        return self.t.dim()


class Maker:
    def __init__(self, standin: bool):
        self.standin = standin
        self.where = torch.device("cpu") if standin else torch.device("cuda", 0)
        self._arena = {}  # data_ptr -> (uint8 buffer, byte offset of the view)

    def _view(self, buf, off, shape, dtype):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + n <= buf.numel(), (off, n, buf.numel())
        v = buf[off:off + n].view(dtype).view(tuple(shape))
        self._arena[v.data_ptr()] = (buf, off)
        return v

    def _raw(self, shape, dtype):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        return self._view(torch.zeros(ROOM + n + ROOM, dtype=torch.uint8, device=self.where), ROOM, shape, dtype)

    def _dev(self, t):
        return StandIn(t, "cuda:0") if self.standin else t

    def dev(self, shape, dtype):
        """A contiguous tensor on cuda:0."""
        return self._dev(self._raw(shape, dtype))

    def alias(self, t, byte_delta: int, shape, dtype):
        """A contiguous cuda:0 tensor that starts ``byte_delta`` bytes after ``t`` does, inside
        t's own allocation."""
        buf, off = self._arena[t.data_ptr()]
        return self._dev(self._view(buf, off + byte_delta, shape, dtype))

    def strided(self, shape, dtype):
        """A non-contiguous cuda:0 view of ``shape`` (every other element of the last axis)."""
        assert shape[-1] > 1
        return self._dev(self._raw(tuple(shape[:-1]) + (2 * shape[-1],), dtype)[..., ::2])

    def host(self, shape, dtype):
        return torch.zeros(tuple(shape), dtype=dtype)

    def other(self, shape, dtype):
        return StandIn(self._raw(shape, dtype), "cuda:1")


# ---- the stub library ------------------------------------------------------------------------
# symbol -> (position of the tap pointer, taps behind it, their C type)
_TAPS_AT = {
    "fir1d_fixed_rows_dev": (5, lambda a: a[6], ctypes.c_int32),
    "fir_decim_rows_dev": (5, lambda a: a[6], ctypes.c_int32),
    "fir1d_fixed_rows_multi_dev": (5, lambda a: a[6] * a[7], ctypes.c_int32),
    "fir1d_fixed_images_multi_dev": (6, lambda a: a[7] * a[8], ctypes.c_int32),
    "fir1d_fixed_edges_dev": (4, lambda a: a[5], ctypes.c_int32),
    "fir1d_fixed_segment_dev": (4, lambda a: a[5], ctypes.c_int32),
    "fir2d_fixed_frames_dev": (4, lambda a: a[5] * a[6], ctypes.c_int32),
    "fir2d_ideal_frames_dev": (4, lambda a: a[5] * a[6], ctypes.c_double),
    "fir1d_ideal_rows_dev": (3, lambda a: a[4], ctypes.c_double),
}


def _norm(v):
    if v is None or isinstance(v, ctypes.c_void_p):  # pointers as integers, NULL as 0
        return (v.value or 0) if v is not None else 0
    if isinstance(v, ctypes.Array):
        return [_norm(e) for e in v]
    return v


class StubLib:
    """Stands in for the ctypes handle: records every call, launches nothing, returns 0."""

    def __init__(self):
        self.calls, self.queries = [], []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "fir_restore_work_bytes":
                self.queries.append(name)
                return RESTORE_WORK
            if name == "fir_metrics_work_bytes":
                self.queries.append(name)
                return metrics_work(*args)
            a = [_norm(v) for v in args]
            if name in _TAPS_AT:  # the host tap array is only alive during the call: read it now
                pos, count, ct = _TAPS_AT[name]
                a[pos] = tuple((ct * count(a)).from_address(a[pos])) if a[pos] else ()
            self.calls.append((name, a))
            return 0

        return fn


# ---- the table -------------------------------------------------------------------------------
@dataclass
class Case:
    id: str
    entry: str
    build: Callable          # Maker -> dict of the valid call's arguments
    call: Callable           # (torch_ops, dict) -> the entry's return value
    mutate: Callable | None  # (Maker, dict) -> None: changes one argument
    error: str | None        # the FirHipError text (regex); None: the call must be accepted
    expect: Callable         # dict -> (C symbol, its arguments)
    check: str = ""
    ncalls: int = 1
    max_taps: int | None = None
    returns: Callable | None = None  # dict -> (shape, dtype) of the returned tensor (accepted cases)


CASES: list[Case] = []


def run_case(case: Case, mk: Maker, torch_ops, monkeypatch):
    """Run one case against the stub; see the module docstring for what passes."""
    stub = StubLib()
    monkeypatch.setattr(torch_ops, "lib", lambda: stub)
    if case.max_taps is not None:
        monkeypatch.setattr(fir_hip, "MAX_TAPS", case.max_taps)
        monkeypatch.setattr(torch_ops, "MAX_TAPS", case.max_taps, raising=False)
    a = case.build(mk)
    if case.mutate is not None:
        case.mutate(mk, a)
    if case.error is not None:
        try:
            with pytest.raises(fir_hip.FirHipError, match=case.error):
                case.call(torch_ops, a)
        finally:
            assert stub.calls == [], f"{case.id}: reached the library: {[c[0] for c in stub.calls]}"
        return None
    got = case.call(torch_ops, a)
    assert len(stub.calls) == case.ncalls, f"{case.id}: {len(stub.calls)} library calls"
    symbol, want = case.expect(a)
    assert stub.calls[0][0] == symbol
    assert stub.calls[0][1] == list(want), f"{case.id}: {symbol} received {stub.calls[0][1]}, expected {list(want)}"
    if case.returns is not None:
        shape, dtype = case.returns(a)
        assert tuple(got.shape) == tuple(shape) and got.dtype == dtype, (case.id, got.shape, got.dtype)
    return got


def _isz(dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def _set(key, make):
    """A mutation that replaces argument ``key`` (a path such as ("outs", 1, 0)) by make(mk, a)."""
    path = key if isinstance(key, tuple) else (key,)

    def mutate(mk, a):
        tgt = a
        for k in path[:-1]:
            tgt = tgt[k]
        tgt[path[-1]] = make(mk, a)
    return mutate


def _get(a, key):
    for k in (key if isinstance(key, tuple) else (key,)):
        a = a[k]
    return a


def _name(key) -> str:
    if not isinstance(key, tuple):
        return key
    return key[0] + "".join(f"[{k}]" for k in key[1:])


def _re(key) -> str:
    return _name(key).replace("[", r"\[").replace("]", r"\]")


class _Entry:
    """Collects the cases of one valid call."""

    def __init__(self, entry: str, base: str, build, call, expect):
        self.entry, self.base, self.build, self.call, self.expect = entry, base, build, call, expect
        self.ok("valid", None)

    def _add(self, vid, mutate, error, check, **kw):
        CASES.append(Case(f"{self.entry}[{self.base}]-{vid}", self.entry, self.build, self.call, mutate, error,
                          self.expect, check, **kw))

    def bad(self, vid, mutate, error, check, **kw):
        self._add(vid, mutate, error, check, **kw)

    def ok(self, vid, mutate, **kw):
        self._add(vid, mutate, None, "", **kw)

    # -- the variants every output gets ----------------------------------------------------
    def out_variants(self, key, shape, dtype, wrong, inputs=("x",), full_rate=None):
        """``key``: the output's argument; ``shape`` / ``dtype``: what is due; ``wrong``: a dtype of
        another size; ``inputs``: the input arguments it must not overlap; ``full_rate``: the
        input-shaped form where a decimated or (F, ...) shape is due."""
        n, rx = _name(key), _re(key)
        shp = rf"{rx} must be {dtype} of shape"
        self.bad(f"{n}-dtype", _set(key, lambda mk, a: mk.dev(shape, wrong)), shp, "_check_out: shape and dtype")
        self.bad(f"{n}-short-last", _set(key, lambda mk, a: mk.dev(shape[:-1] + (shape[-1] - 1,), dtype)), shp,
                 "_check_out: shape and dtype")
        if len(shape) > 1:
            self.bad(f"{n}-short-row", _set(key, lambda mk, a: mk.dev(shape[:-2] + (shape[-2] - 1, shape[-1]), dtype)),
                     shp, "_check_out: shape and dtype")
        if len(shape) > 2:
            self.bad(f"{n}-short-lead", _set(key, lambda mk, a: mk.dev((shape[0] - 1,) + shape[1:], dtype)), shp,
                     "_check_out: shape and dtype")
        if full_rate is not None:
            self.bad(f"{n}-full-rate", _set(key, lambda mk, a: mk.dev(full_rate, dtype)), shp,
                     "_check_out: shape and dtype")
        self.bad(f"{n}-strided", _set(key, lambda mk, a: mk.strided(shape, dtype)), rf"{rx} must be contiguous",
                 "_check_out: contiguous")
        self.bad(f"{n}-host", _set(key, lambda mk, a: mk.host(shape, dtype)), rf"{rx} must be a device tensor",
                 "_check_out: device tensor")
        self.bad(f"{n}-other-device", _set(key, lambda mk, a: mk.other(shape, dtype)), rf"{rx} must be on cuda:0",
                 "_check_out: same device")
        isz, nb = _isz(dtype), math.prod(shape) * _isz(dtype)
        for ikey in inputs:  # the boundary variants need the input's end aligned for `dtype`: the first input's is
            i, msg = _name(ikey), rf"{rx} must not overlap the input \({_re(ikey)}\)"

            def at(delta, ikey=ikey):
                return _set(key, lambda mk, a: mk.alias(_get(a, ikey), delta(_nbytes(_get(a, ikey))), shape, dtype))

            self.bad(f"{n}-is-{i}", at(lambda xb: 0), msg, "_no_overlap: input")
            self.bad(f"{n}-ends-in-{i}", at(lambda xb: isz - nb), msg, "_no_overlap: input")
            if ikey != inputs[0]:
                continue
            self.bad(f"{n}-overlaps-{i}-tail", at(lambda xb: (xb - 1) // isz * isz), msg, "_no_overlap: input")
            self.ok(f"{n}-right-after-{i}", at(lambda xb: xb))
            self.ok(f"{n}-right-before-{i}", at(lambda xb: -nb))

    def x_variants(self, key, shape, dtype, wrong, dtype_error):
        n, rx = _name(key), _re(key)
        self.bad(f"{n}-dtype", _set(key, lambda mk, a: mk.dev(shape, wrong)), dtype_error, f"{self.entry}: x dtype")
        self.bad(f"{n}-strided", _set(key, lambda mk, a: mk.strided(shape, dtype)), rf"{rx} must be contiguous",
                 "_check_dev (before this change)")
        self.bad(f"{n}-host", _set(key, lambda mk, a: mk.host(shape, dtype)), rf"{rx} must be a device tensor",
                 "_check_dev (before this change)")

    def channels_variants(self, text, not_dividing: int):
        for vid, ch in (("not-dividing", not_dividing), ("zero", 0), ("negative", -1)):
            self.bad(f"channels-{vid}", _set("channels", lambda mk, a, ch=ch: ch), text, "channels >= 1 and dividing")

    def taps_variants(self, key, L: int, at_limit: bool = True):
        """1-D quantized taps (``at_limit``: also a filter of exactly the limit's length, where the
        valid call's other arguments do not depend on the tap count)."""
        c = "_taps_i32 (before this change)"
        self.bad("taps-empty", _set(key, lambda mk, a: []), "non-empty 1-D", c)
        self.bad("taps-2d", _set(key, lambda mk, a: np.ones((2, L), np.int64)), "non-empty 1-D", c)
        self.bad("taps-too-many", _set(key, lambda mk, a: np.ones(SMALL_MAX_TAPS + 1, np.int64)),
                 "exceed the library limit", c, max_taps=SMALL_MAX_TAPS)
        if at_limit:
            self.ok("taps-at-limit", _set(key, lambda mk, a: np.ones(SMALL_MAX_TAPS, np.int64)), max_taps=SMALL_MAX_TAPS)
        self.bad("taps-2p31", _set(key, lambda mk, a: [1] * (L - 1) + [2**31]), "must fit in int32", c)
        self.bad("taps-below-int32", _set(key, lambda mk, a: [-2**31 - 1] + [1] * (L - 1)), "must fit in int32", c)
        self.ok("taps-int32-ends", _set(key, lambda mk, a: [I32_MAX, I32_MIN] + [3] * (L - 2)))

    def bank_variants(self, key, F: int, L: int):
        """A (filters, taps) bank of quantized taps; F and L stay those of the valid call."""
        c = "_bank_i32"
        empty = r"non-empty \(filters, taps\) array"
        self.bad("bank-1d", _set(key, lambda mk, a: np.ones(L, np.int64)), empty, c + ": 2-D")
        self.bad("bank-no-filters", _set(key, lambda mk, a: np.ones((0, L), np.int64)), empty, c + ": F >= 1")
        self.bad("bank-no-taps", _set(key, lambda mk, a: np.ones((F, 0), np.int64)), empty, c + ": L >= 1")
        self.bad("bank-too-many", _set(key, lambda mk, a: np.ones((F, SMALL_MAX_TAPS + 1), np.int64)),
                 "exceed the library limit", c + ": MAX_TAPS", max_taps=SMALL_MAX_TAPS)

        def with_tap(v):
            def make(mk, a):
                h = np.arange(1, F * L + 1, dtype=np.int64).reshape(F, L)
                h[F - 1, 1] = v
                return h
            return _set(key, make)

        self.bad("bank-2p31", with_tap(2**31), "must fit in int32", c + ": int32 range")
        self.bad("bank-below-int32", with_tap(-2**31 - 1), "must fit in int32", c + ": int32 range")
        self.ok("bank-int32-max", with_tap(I32_MAX))
        self.ok("bank-int32-min", with_tap(I32_MIN))


def _flat(h) -> tuple:
    return tuple(int(v) for v in np.asarray(h).reshape(-1))


_IN = {torch.uint8: fir_hip.IN_U8, torch.int16: fir_hip.IN_I16}
_ST = {U8: torch.uint8, I32: torch.int32}
_OTHER = {torch.uint8: torch.int32, torch.int32: torch.uint8, torch.float64: torch.float32}
TAPS5 = [-256, -1024, 6656, -1024, -256]
BANK = np.array([[1365, 1365, 1366], [1024, 2048, 1024]], np.int64)
X_DTYPE = r"x dtype must be uint8 or int16, got torch\.float32"
ROWLEN = "row length must be a multiple of channels"


def _rows_geometry(x, ch):
    rowlen = x.shape[-1] if x.dim() else 1
    return (x.numel() // rowlen if rowlen else 0), rowlen // ch


# -- fir1d_fixed_rows_dev, fir1d_fixed_rows_decim_dev, fir1d_fixed_rows_multi_dev ---------------
_ROWS_BASES = (("u8", torch.uint8, U8, 1, (3, 40)), ("i16c2-i32", torch.int16, I32, 2, (3, 40)))


def _each(bases):
    """Run the decorated function once per base (its own scope per base: the variants' closures
    are called later, by the tests)."""
    def run(fn):
        for b in bases:
            fn(*b)
        return fn
    return run


def _rows_entries():
    @_each(_ROWS_BASES + (("u8-i32-1d", torch.uint8, I32, 1, (40,)),))
    def rows(base, xdt, stage, ch, shape):
        odt = _ST[stage]

        def build(mk, xdt=xdt, stage=stage, ch=ch, shape=shape, odt=odt):
            return dict(x=mk.dev(shape, xdt), hq=list(TAPS5), frac=12, acc=32, stage=stage, channels=ch,
                        out=mk.dev(shape, odt), stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_rows_dev(a["x"], a["hq"], a["frac"], a["acc"], a["stage"], a["channels"],
                                            out=a["out"], stream=a["stream"])

        def expect(a):
            rows, width = _rows_geometry(a["x"], a["channels"])
            return "fir1d_fixed_rows_dev", [a["x"].data_ptr(), _IN[a["x"].dtype], rows, width, a["channels"],
                                            _flat(a["hq"]), len(_flat(a["hq"])), 12, 32, a["stage"],
                                            a["out"].data_ptr(), STREAM]

        e = _Entry("fir1d_fixed_rows_dev", base, build, call, expect)
        e.out_variants("out", shape, odt, _OTHER[odt])
        if base == "u8":  # the one call whose out may be x itself by shape and dtype: still refused
            e.bad("out-is-the-x-object", _set("out", lambda mk, a: a["x"]), r"out must not overlap the input \(x\)",
                  "_no_overlap: input")
        e.x_variants("x", shape, xdt, torch.float32, X_DTYPE)
        e.channels_variants(ROWLEN, 3)
        e.taps_variants("hq", 5)
        e.bad("stage-unknown", _set("stage", lambda mk, a: 2), "out_stage must be", "_out_dtype")
        e.ok("x-empty-rows", lambda mk, a: a.update(x=mk.dev((0,) + shape[1:], xdt), out=mk.dev((0,) + shape[1:], odt)))
        e.ok("x-empty-width", lambda mk, a: a.update(x=mk.dev(shape[:-1] + (0,), xdt), out=mk.dev(shape[:-1] + (0,), odt)))
        e.ok("x-0d", lambda mk, a: a.update(x=mk.dev((), xdt), out=mk.dev((), odt), channels=1))

    D, PH = 4, 1

    @_each(_ROWS_BASES)
    def decim(base, xdt, stage, ch, shape):
        odt = _ST[stage]
        oshape = shape[:-1] + (fir_hip.decim_out_width(shape[-1] // ch, D, PH) * ch,)

        def build(mk, xdt=xdt, stage=stage, ch=ch, shape=shape, odt=odt, oshape=oshape):
            return dict(x=mk.dev(shape, xdt), hq=list(TAPS5), decim=D, phase=PH, frac=12, acc=32, stage=stage,
                        channels=ch, out=mk.dev(oshape, odt), stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_rows_decim_dev(a["x"], a["hq"], a["decim"], a["phase"], a["frac"], a["acc"], a["stage"],
                                                  a["channels"], out=a["out"], stream=a["stream"])

        def expect(a):
            rows, width = _rows_geometry(a["x"], a["channels"])
            return "fir_decim_rows_dev", [a["x"].data_ptr(), _IN[a["x"].dtype], rows, width, a["channels"], _flat(a["hq"]),
                                          len(_flat(a["hq"])), a["decim"], a["phase"], 12, 32, a["stage"],
                                          a["out"].data_ptr(), STREAM]

        e = _Entry("fir1d_fixed_rows_decim_dev", base, build, call, expect)
        e.out_variants("out", oshape, odt, _OTHER[odt], full_rate=shape)
        e.x_variants("x", shape, xdt, torch.float32, X_DTYPE)
        e.channels_variants(ROWLEN, 3)
        e.taps_variants("hq", 5)
        e.bad("decim-zero", _set("decim", lambda mk, a: 0), "decim must be >= 1", "decim_out_width (before this change)")
        e.bad("phase-is-decim", _set("phase", lambda mk, a: D), r"phase must be in \[0, decim\)",
              "decim_out_width (before this change)")
        e.ok("x-empty-rows", lambda mk, a, o=oshape: a.update(x=mk.dev((0,) + shape[1:], xdt), out=mk.dev((0,) + o[1:], odt)))

    @_each(_ROWS_BASES)
    def multi(base, xdt, stage, ch, shape):
        odt = _ST[stage]
        F, L = BANK.shape
        oshape = (F,) + shape

        def build(mk, xdt=xdt, stage=stage, ch=ch, shape=shape, odt=odt, oshape=oshape):
            return dict(x=mk.dev(shape, xdt), hq2=BANK.copy(), frac=12, acc=64, stage=stage, channels=ch,
                        out=mk.dev(oshape, odt), stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_rows_multi_dev(a["x"], a["hq2"], a["frac"], a["acc"], a["stage"], a["channels"],
                                                  out=a["out"], stream=a["stream"])

        def expect(a):
            rows, width = _rows_geometry(a["x"], a["channels"])
            nf, L = np.asarray(a["hq2"]).shape
            return "fir1d_fixed_rows_multi_dev", [a["x"].data_ptr(), _IN[a["x"].dtype], rows, width, a["channels"],
                                                  _flat(a["hq2"]), L, nf, 12, 64, a["stage"], a["out"].data_ptr(), STREAM]

        e = _Entry("fir1d_fixed_rows_multi_dev", base, build, call, expect)
        e.out_variants("out", oshape, odt, _OTHER[odt], full_rate=shape)
        e.x_variants("x", shape, xdt, torch.float32, X_DTYPE)
        e.channels_variants(ROWLEN, 3)
        e.bank_variants("hq2", F, L)
        e.ok("x-empty-rows", lambda mk, a: a.update(x=mk.dev((0,) + shape[1:], xdt), out=mk.dev((F, 0) + shape[1:], odt)))


_rows_entries()


# -- ImagesMultiPlan / fir1d_fixed_images_multi_dev ---------------------------------------------
def _images_entries():
    F, L = BANK.shape
    s0, s1 = (3, 40), (2, 24)
    @_each((("u8", torch.uint8, U8, 1), ("i16c2-i32", torch.int16, I32, 2)))
    def images(base, xdt, stage, ch):
        odt = _ST[stage]

        def build(mk, xdt=xdt, stage=stage, ch=ch, odt=odt):
            # both forms of outs[i]: one (F, *shape) tensor, and a list of F planes
            return dict(xs=[mk.dev(s0, xdt), mk.dev(s1, xdt)], hq2=BANK.copy(), frac=12, acc=64, stage=stage, channels=ch,
                        outs=[mk.dev((F,) + s0, odt), [mk.dev(s1, odt) for _ in range(F)]], stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_images_multi_dev(a["xs"], a["hq2"], a["frac"], a["acc"], a["stage"], a["channels"],
                                                    a["outs"], a["stream"])

        def expect(a):
            xs, ch = a["xs"], a["channels"]
            nf, L = np.asarray(a["hq2"]).shape
            planes = []
            for x, o in zip(xs, a["outs"]):
                if isinstance(o, list):
                    planes += [p.data_ptr() for p in o]
                else:
                    planes += [o.data_ptr() + f * x.numel() * o.element_size() for f in range(nf)]
            geo = [_rows_geometry(x, ch) for x in xs]
            return "fir1d_fixed_images_multi_dev", [len(xs), [x.data_ptr() for x in xs], [g[0] for g in geo],
                                                    [g[1] for g in geo], _IN[xs[0].dtype], ch, _flat(a["hq2"]), L, nf, 12, 64,
                                                    a["stage"], planes, STREAM]

        e = _Entry("fir1d_fixed_images_multi_dev", base, build, call, expect)
        e.out_variants(("outs", 0), (F,) + s0, odt, _OTHER[odt], inputs=(("xs", 0), ("xs", 1)), full_rate=s0)
        e.out_variants(("outs", 1, 1), s1, odt, _OTHER[odt], inputs=(("xs", 1), ("xs", 0)))
        e.bad("planes-overlap", _set(("outs", 1, 1), lambda mk, a: mk.alias(a["outs"][1][0], _isz(odt) * 5, s1, odt)),
              r"outs\[1\]\[1\] must not overlap outs\[1\]\[0\]", "_no_overlap: two outputs")
        e.bad("plane-in-other-images-out",
              _set(("outs", 1, 0), lambda mk, a: mk.alias(a["outs"][0], _isz(odt) * 8, s1, odt)),
              r"outs\[1\]\[0\] must not overlap outs\[0\]", "_no_overlap: two outputs")
        e.bad("outs-one-short", _set("outs", lambda mk, a: a["outs"][:1]), "outs must hold one entry per image",
              "ImagesMultiPlan (before this change)")
        e.bad("planes-one-short", _set(("outs", 1), lambda mk, a: a["outs"][1][:1]), rf"outs\[1\] must hold {F} planes",
              "ImagesMultiPlan (before this change)")
        other = torch.int16 if xdt == torch.uint8 else torch.uint8
        e.bad("xs[1]-dtype-differs", _set(("xs", 1), lambda mk, a: mk.dev(s1, other)), r"xs\[1\]: every image must be",
              "ImagesMultiPlan (before this change)")
        e.bad("xs[0]-dtype", _set(("xs", 0), lambda mk, a: mk.dev(s0, torch.float32)), r"xs\[0\]: every image must be",
              "ImagesMultiPlan (before this change)")
        e.bad("xs[1]-other-device", _set(("xs", 1), lambda mk, a: mk.other(s1, xdt)), r"xs\[1\]: every image must be on",
              "ImagesMultiPlan (before this change)")
        e.bad("xs[1]-strided", _set(("xs", 1), lambda mk, a: mk.strided(s1, xdt)), r"xs\[1\] must be contiguous",
              "ImagesMultiPlan (before this change)")
        e.bad("xs[1]-host", _set(("xs", 1), lambda mk, a: mk.host(s1, xdt)), r"xs\[1\] must be a device tensor",
              "ImagesMultiPlan (before this change)")
        e.channels_variants(r"xs\[0\]: row length must be a multiple of channels", 3)
        e.bank_variants("hq2", F, L)
        e.ok("image-empty", lambda mk, a: (a["xs"].__setitem__(1, mk.dev((0, 24), xdt)),
                                           a["outs"].__setitem__(1, [mk.dev((0, 24), odt) for _ in range(F)])))


_images_entries()


# -- fir1d_fixed_edges_dev, fir1d_fixed_segment_dev ---------------------------------------------
def _segment_entries():
    n = 40
    for entry in ("fir1d_fixed_edges_dev", "fir1d_fixed_segment_dev"):
        @_each(((entry, "u8-i32", torch.uint8, I32, 1), (entry, "i16c2-u8", torch.int16, U8, 2)))
        def segment(entry, base, xdt, stage, ch):
            odt = _ST[stage]
            hl_n, hr_n = 2 * ch, 2 * ch  # 5 taps

            def build(mk, xdt=xdt, stage=stage, ch=ch, odt=odt, hl_n=hl_n, hr_n=hr_n):
                return dict(x=mk.dev((n,), xdt), hq=list(TAPS5), out=mk.dev((n,), odt), halo_left=mk.dev((hl_n,), xdt),
                            halo_right=mk.dev((hr_n,), xdt), frac=12, acc=32, stage=stage, channels=ch, stream=Stream())

            if entry == "fir1d_fixed_edges_dev":
                def call(ops, a):
                    return ops.fir1d_fixed_edges_dev(a["x"], a["hq"], a["out"], a["halo_left"], a["halo_right"], a["frac"],
                                                     a["acc"], a["stage"], a["channels"], stream=a["stream"])
            else:
                def call(ops, a):
                    return ops.fir1d_fixed_segment_dev(a["x"], a["hq"], a["halo_left"], a["halo_right"], a["frac"],
                                                       a["acc"], a["stage"], a["channels"], out=a["out"], stream=a["stream"])

            def expect(a, entry=entry):
                def ptr(h, count):
                    if h is None or not count:
                        return 0
                    return h if isinstance(h, int) else h.data_ptr()
                L, ch = len(_flat(a["hq"])), a["channels"]
                return entry, [a["x"].data_ptr(), _IN[a["x"].dtype], a["x"].numel() // ch, ch, _flat(a["hq"]), L, 12, 32,
                               a["stage"], ptr(a["halo_left"], (L - 1 - L // 2) * ch), ptr(a["halo_right"], (L // 2) * ch),
                               a["out"].data_ptr(), STREAM]

            e = _Entry(entry, base, build, call, expect)
            e.out_variants("out", (n,), odt, _OTHER[odt], inputs=("x", "halo_left", "halo_right"))
            e.x_variants("x", (n,), xdt, torch.float32, X_DTYPE)
            e.channels_variants("segment length must be a multiple of channels", 3)
            e.taps_variants("hq", 5, at_limit=False)  # the halo lengths follow the tap count
            for side, cnt in (("halo_left", hl_n), ("halo_right", hr_n)):
                text = rf"{side} must hold {cnt} samples of"
                wrong = torch.int16 if xdt == torch.uint8 else torch.uint8
                e.bad(f"{side}-dtype", _set(side, lambda mk, a, c=cnt: mk.dev((c,), wrong)), text,
                      "_halo_ptrs (before this change)")
                e.bad(f"{side}-long", _set(side, lambda mk, a, c=cnt: mk.dev((c + 1,), xdt)), text,
                      "_halo_ptrs (before this change)")
                e.bad(f"{side}-short", _set(side, lambda mk, a, c=cnt: mk.dev((c - 1,), xdt)), text,
                      "_halo_ptrs (before this change)")
                e.bad(f"{side}-host", _set(side, lambda mk, a, c=cnt: mk.host((c,), xdt)), rf"{side} must be a device tensor",
                      "_halo_ptrs (before this change)")
                e.bad(f"{side}-strided", _set(side, lambda mk, a, c=cnt: mk.strided((c,), xdt)), rf"{side} must be contiguous",
                      "_halo_ptrs (before this change)")
                e.bad(f"{side}-other-device", _set(side, lambda mk, a, c=cnt: mk.other((c,), xdt)), rf"{side} must be on cuda:0",
                      "_check_in: same device")
                e.ok(f"{side}-none", _set(side, lambda mk, a: None))
                e.ok(f"{side}-address", _set(side, lambda mk, a: 0x7F0000001000))
            e.ok("one-tap-ignores-halos", _set("hq", lambda mk, a: [4096]))
            e.ok("x-empty", lambda mk, a: a.update(x=mk.dev((0,), xdt), out=mk.dev((0,), odt)))
            e.bad("stage-unknown", _set("stage", lambda mk, a: 7), "out_stage must be", "_out_dtype")


_segment_entries()


# -- halo_mailbox_init_dev, halo_gate_dev: device and contiguity of the tensor arguments only ----
def _gate_entries():
    def build_init(mk):
        return dict(mailbox=mk.dev((512,), torch.uint8), hl=4, hr=6, stream=Stream())

    e = _Entry("halo_mailbox_init_dev", "u8", build_init,
               lambda ops, a: ops.halo_mailbox_init_dev(a["mailbox"], a["hl"], a["hr"], a["stream"]),
               lambda a: ("fir_halo_mailbox_init_dev", [a["mailbox"].data_ptr(), 512, 4, 6, STREAM]))
    e.bad("mailbox-host", _set("mailbox", lambda mk, a: mk.host((512,), torch.uint8)), "mailbox must be a device tensor",
          "_check_dev (before this change)")
    e.bad("mailbox-strided", _set("mailbox", lambda mk, a: mk.strided((512,), torch.uint8)), "mailbox must be contiguous",
          "_check_dev (before this change)")

    shapes = dict(seg=((40,), torch.int16), mailbox=((512,), torch.uint8), halo_left=((2,), torch.int16),
                  halo_right=((3,), torch.int16), status=((2,), torch.int32))

    def build_gate(mk):
        a = {k: mk.dev(*v) for k, v in shapes.items()}
        a.update(hl=4, hr=6, left_mb=0x7F0000002000, right_mb=None, timeout=2.5, stream=Stream())
        return a

    def call_gate(ops, a):
        return ops.halo_gate_dev(a["seg"], a["hl"], a["hr"], a["mailbox"], a["left_mb"], a["right_mb"], a["halo_left"],
                                 a["halo_right"], a["status"], a["timeout"], a["stream"])

    def expect_gate(a):
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        return "fir_halo_gate_dev", [a["seg"].data_ptr(), 80, 4, 6, a["mailbox"].data_ptr(), a["left_mb"] or 0,
                                     a["right_mb"] or 0,
                                     ptr(a["halo_left"]), ptr(a["halo_right"]), ptr(a["status"]), 2.5, STREAM]

    e = _Entry("halo_gate_dev", "i16", build_gate, call_gate, expect_gate)
    for k, (shape, dt) in shapes.items():
        was = "_check_dev (before this change)" if k in ("seg", "mailbox") else "halo_gate_dev: tensor arguments"
        e.bad(f"{k}-host", _set(k, lambda mk, a, s=shape, d=dt: mk.host(s, d)), f"{k} must be a device tensor", was)
        e.bad(f"{k}-strided", _set(k, lambda mk, a, s=shape, d=dt: mk.strided(s, d)), f"{k} must be contiguous", was)
    e.ok("halos-none", lambda mk, a: a.update(halo_left=None, halo_right=None))


_gate_entries()


# -- fir2d_fixed_dev, fir2d_ideal_dev ------------------------------------------------------------
K3 = np.array([[0, -512, 0], [-512, 6144, -512], [0, -512, 0]], np.int64)
X2D = "x must be a 2-D"


def _fir2d_entries():
    @_each((("frames-i32", (2, 5, 16), I32), ("frame-u8", (5, 16), U8)))
    def fixed(base, shape, stage):
        odt = _ST[stage]

        def build(mk, shape=shape, stage=stage, odt=odt):
            return dict(x=mk.dev(shape, torch.uint8), hq2=K3.copy(), frac=12, acc=32, stage=stage, out=mk.dev(shape, odt),
                        stream=Stream())

        def call(ops, a):
            return ops.fir2d_fixed_dev(a["x"], a["hq2"], a["frac"], a["acc"], a["stage"], out=a["out"], stream=a["stream"])

        def expect(a):
            s = tuple(a["x"].shape)
            R, C = np.asarray(a["hq2"]).shape
            return "fir2d_fixed_frames_dev", [a["x"].data_ptr(), s[0] if len(s) == 3 else 1, s[-2], s[-1], _flat(a["hq2"]), R,
                                              C, 12, 32, a["stage"], a["out"].data_ptr(), STREAM]

        e = _Entry("fir2d_fixed_dev", base, build, call, expect)
        e.out_variants("out", shape, odt, _OTHER[odt])
        e.x_variants("x", shape, torch.uint8, torch.int16, X2D)
        e.bad("x-1d", _set("x", lambda mk, a: mk.dev((80,), torch.uint8)), X2D, "fir2d_fixed_dev (before this change)")
        e.bad("x-4d", _set("x", lambda mk, a: mk.dev((1, 2, 5, 8), torch.uint8)), X2D, "fir2d_fixed_dev (before this change)")
        b = "fir2d_fixed_dev (before this change)"
        e.bad("taps-1d", _set("hq2", lambda mk, a: np.ones(9, np.int64)), "hq2 must be 2-D", b)
        e.bad("taps-empty", _set("hq2", lambda mk, a: np.ones((0, 3), np.int64)), "non-empty 1-D", b)
        e.bad("taps-too-many", _set("hq2", lambda mk, a: np.ones((9, 9), np.int64)), "exceed the library limit", b,
              max_taps=SMALL_MAX_TAPS)
        e.bad("taps-2p31", _set("hq2", lambda mk, a: np.array([[1, 2**31, 1]])), "must fit in int32", b)
        e.bad("taps-below-int32", _set("hq2", lambda mk, a: np.array([[1], [-2**31 - 1], [1]])), "must fit in int32", b)
        e.ok("taps-int32-ends", _set("hq2", lambda mk, a: np.array([[I32_MAX, 1, I32_MIN]])))
        e.bad("stage-unknown", _set("stage", lambda mk, a: -1), "out_stage must be", "_out_dtype")
        e.ok("x-empty", lambda mk, a: a.update(x=mk.dev(shape[:-2] + (0, 16), torch.uint8), out=mk.dev(shape[:-2] + (0, 16), odt)))

    H3 = np.array([[0.0, -0.125, 0.0], [-0.125, 1.5, -0.125], [0.0, -0.125, 0.0]])
    @_each((("frames", (2, 5, 16)), ("frame", (5, 16))))
    def ideal(base, shape):
        def build(mk, shape=shape):
            return dict(x=mk.dev(shape, torch.uint8), h2=H3.copy(), out=mk.dev(shape, torch.float64), stream=Stream())

        def call(ops, a):
            return ops.fir2d_ideal_dev(a["x"], a["h2"], out=a["out"], stream=a["stream"])

        def expect(a):
            s = tuple(a["x"].shape)
            h = np.asarray(a["h2"], np.float64)
            return "fir2d_ideal_frames_dev", [a["x"].data_ptr(), s[0] if len(s) == 3 else 1, s[-2], s[-1],
                                              tuple(float(v) for v in h.reshape(-1)), h.shape[0], h.shape[1],
                                              a["out"].data_ptr(), STREAM]

        e = _Entry("fir2d_ideal_dev", base, build, call, expect)
        e.out_variants("out", shape, torch.float64, torch.float32)
        e.x_variants("x", shape, torch.uint8, torch.int16, X2D)
        e.bad("x-1d", _set("x", lambda mk, a: mk.dev((80,), torch.uint8)), X2D, "fir2d_ideal_dev (before this change)")
        b = "_taps2_f64 (before this change)"
        e.bad("taps-1d", _set("h2", lambda mk, a: np.ones(9)), "h2 must be a non-empty 2-D array", b)
        e.bad("taps-empty", _set("h2", lambda mk, a: np.ones((3, 0))), "h2 must be a non-empty 2-D array", b)
        e.bad("taps-too-many", _set("h2", lambda mk, a: np.ones((5, 13))), "exceed the library limit", b,
              max_taps=SMALL_MAX_TAPS)
        e.ok("x-empty", lambda mk, a: a.update(x=mk.dev(shape[:-1] + (0,), torch.uint8),
                                               out=mk.dev(shape[:-1] + (0,), torch.float64)))


_fir2d_entries()


# -- fir1d_ideal_rows_dev ------------------------------------------------------------------------
H5 = [-0.0625, -0.25, 1.625, -0.25, -0.0625]


def _ideal_entries():
    @_each((("rows", (3, 40)), ("1d", (40,))))
    def ideal(base, shape):
        def build(mk, shape=shape):
            return dict(x=mk.dev(shape, torch.uint8), h=list(H5), out=mk.dev(shape, torch.float64), stream=Stream())

        def call(ops, a):
            return ops.fir1d_ideal_rows_dev(a["x"], a["h"], out=a["out"], stream=a["stream"])

        def expect(a):
            x = a["x"]
            width = x.shape[-1] if x.dim() else 1
            h = tuple(float(v) for v in np.asarray(a["h"], np.float64).reshape(-1))
            return "fir1d_ideal_rows_dev", [x.data_ptr(), x.numel() // width if width else 0, width, h, len(h),
                                            a["out"].data_ptr(), STREAM]

        e = _Entry("fir1d_ideal_rows_dev", base, build, call, expect)
        e.out_variants("out", shape, torch.float64, torch.float32)
        e.x_variants("x", shape, torch.uint8, torch.int16, "x must be uint8")
        c = "fir1d_ideal_rows_dev: tap count"
        e.bad("taps-empty", _set("h", lambda mk, a: []), r"tap count must be in \[1, ", c)
        e.bad("taps-too-many", _set("h", lambda mk, a: np.ones(SMALL_MAX_TAPS + 1)), r"tap count must be in \[1, 64\]", c,
              max_taps=SMALL_MAX_TAPS)
        e.ok("taps-at-limit", _set("h", lambda mk, a: np.ones(SMALL_MAX_TAPS)), max_taps=SMALL_MAX_TAPS)
        e.ok("x-empty", lambda mk, a: a.update(x=mk.dev(shape[:-1] + (0,), torch.uint8),
                                               out=mk.dev(shape[:-1] + (0,), torch.float64)))
        e.ok("x-0d", lambda mk, a: a.update(x=mk.dev((), torch.uint8), out=mk.dev((), torch.float64)))


_ideal_entries()


# -- restore_u8_dev, compare_metrics_dev ---------------------------------------------------------
def _work_variants(e, need, inputs, out_key="out"):
    """``work`` is checked by byte count: any dtype, at least ``need`` bytes."""
    text = rf"work must be a contiguous device buffer of >= {need} bytes"
    e.bad("work-one-byte-short", _set("work", lambda mk, a: mk.dev((need - 1,), torch.uint8)), text, "_check_work: bytes")
    e.bad("work-strided", _set("work", lambda mk, a: mk.strided((need,), torch.uint8)), text, "_check_work: contiguous")
    e.bad("work-host", _set("work", lambda mk, a: mk.host((need,), torch.uint8)), text, "_check_work: device tensor")
    e.bad("work-other-device", _set("work", lambda mk, a: mk.other((need,), torch.uint8)), "work must be on cuda:0",
          "_check_work: same device")
    e.ok("work-float64-of-need-bytes", _set("work", lambda mk, a: mk.dev((need // 8,), torch.float64)))
    e.ok("work-larger", _set("work", lambda mk, a: mk.dev((need + 1,), torch.uint8)))
    e.bad("work-overlaps-out", _set("work", lambda mk, a: mk.alias(a[out_key], _nbytes(a[out_key]) - 1, (need,), torch.uint8)),
          r"work must not overlap out", "_no_overlap: two outputs")
    e.ok("work-right-after-out", _set("work", lambda mk, a: mk.alias(a[out_key], _nbytes(a[out_key]), (need,), torch.uint8)))
    for k in inputs:
        e.bad(f"work-overlaps-{k}", _set("work", lambda mk, a, k=k: mk.alias(a[k], 1 - need, (need,), torch.uint8)),
              rf"work must not overlap the input \({k}\)", "_no_overlap: input")


def _restore_entries():
    @_each((("normalize", (3, 40), NORMALIZE), ("clip-1d", (40,), CLIP)))
    def restore(base, shape, policy):
        def build(mk, shape=shape, policy=policy):
            return dict(a=mk.dev(shape, torch.float64), policy=policy, out=mk.dev(shape, torch.uint8),
                        work=mk.dev((RESTORE_WORK,), torch.uint8) if policy == NORMALIZE else None, stream=Stream())

        def call(ops, a):
            return ops.restore_u8_dev(a["a"], a["policy"], out=a["out"], work=a["work"], stream=a["stream"])

        def expect(a):
            return "fir_restore_u8_dev", [a["a"].data_ptr(), a["a"].numel(), a["policy"], a["out"].data_ptr(),
                                          0 if a["work"] is None else a["work"].data_ptr(), STREAM]

        e = _Entry("restore_u8_dev", base, build, call, expect)
        e.out_variants("out", shape, torch.uint8, torch.int32, inputs=("a",))
        e.bad("out-u8-view-of-a", _set("out", lambda mk, a: mk.alias(a["a"], 0, shape, torch.uint8)),
              r"out must not overlap the input \(a\)", "_no_overlap: input")
        e.x_variants("a", shape, torch.float64, torch.float32, "a must be float64")
        if policy == NORMALIZE:
            _work_variants(e, RESTORE_WORK, ("a",))
        else:  # a work buffer handed to the clip policy goes to the C entry too: the same checks
            e.bad("work-one-byte-short", _set("work", lambda mk, a: mk.dev((RESTORE_WORK - 1,), torch.uint8)),
                  "work must be a contiguous device buffer", "_check_work: bytes")
            e.ok("work-given", _set("work", lambda mk, a: mk.dev((RESTORE_WORK,), torch.uint8)))
        e.ok("a-empty", lambda mk, a: a.update(a=mk.dev((0,) + shape[1:], torch.float64),
                                               out=mk.dev((0,) + shape[1:], torch.uint8)))


_restore_entries()


def _metrics_entries():
    shape = (3, 40)
    need = metrics_work(120)
    @_each((("u8", torch.uint8, 0), ("i32", torch.int32, 5)))
    def metrics(base, fdt, code):
        def build(mk, fdt=fdt):
            return dict(ideal=mk.dev(shape, torch.float64), fixed=mk.dev(shape, fdt), out=mk.dev((9,), torch.float64),
                        work=mk.dev((need,), torch.uint8), stream=Stream())

        def call(ops, a):
            return ops.compare_metrics_dev(a["ideal"], a["fixed"], out=a["out"], work=a["work"], stream=a["stream"])

        def expect(a, code=code):
            return "fir_compare_metrics_dev", [a["ideal"].data_ptr(), a["fixed"].data_ptr(), code, a["ideal"].numel(),
                                               a["out"].data_ptr(), a["work"].data_ptr(), STREAM]

        e = _Entry("compare_metrics_dev", base, build, call, expect)
        e.out_variants("out", (9,), torch.float64, torch.float32, inputs=("ideal", "fixed"))
        e.bad("out-one-long", _set("out", lambda mk, a: mk.dev((10,), torch.float64)), "out must be torch.float64 of shape",
              "_check_out: shape and dtype")
        _work_variants(e, need, ("ideal", "fixed"))
        pair = "ideal must be float64 and fixed"
        b = "compare_metrics_dev (before this change)"
        e.bad("ideal-dtype", _set("ideal", lambda mk, a: mk.dev(shape, torch.float32)), pair, b)
        e.bad("fixed-dtype", _set("fixed", lambda mk, a: mk.dev(shape, torch.complex64)), pair, b)
        e.bad("fixed-shape", _set("fixed", lambda mk, a: mk.dev((3, 39), fdt)), pair, b)
        for k, dt in (("ideal", torch.float64), ("fixed", fdt)):
            e.bad(f"{k}-host", _set(k, lambda mk, a, dt=dt: mk.host(shape, dt)), f"{k} must be a device tensor", b)
            e.bad(f"{k}-strided", _set(k, lambda mk, a, dt=dt: mk.strided(shape, dt)), f"{k} must be contiguous", b)
        e.bad("fixed-other-device", _set("fixed", lambda mk, a: mk.other(shape, fdt)), "fixed must be on cuda:0",
              "_check_in: same device")

        def empty(mk, a, fdt=fdt):
            a.update(ideal=mk.dev((0, 40), torch.float64), fixed=mk.dev((0, 40), fdt), work=mk.dev((metrics_work(0),), torch.uint8))
        e.ok("empty", empty)


_metrics_entries()

assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
ENTRIES = sorted({c.entry for c in CASES})
