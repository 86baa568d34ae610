"""The argument contract of fir_hip.torch_resample as a table -- a test helper, not a test module.

Built like tests/torch_interp_cases.py on tests/torch_ops_cases.py, whose ``Case``, ``Maker``,
``StubLib`` and ``run_case`` it uses: per base (u8 -> u8 of one channel, complex int16 -> int32, a
1-D int16 row) one valid call of ``fir1d_fixed_rows_resample_dev`` and variants that differ in
exactly one argument, each with the ``FirHipError`` text it must raise or, where the variant must be
accepted, the exact ``fir_resample_rows_dev`` call the stub library must record.  ``run`` runs one
case against the stub: nothing is launched, so the table needs no GPU (``Maker(standin=True)``) and
is equally valid on device tensors (``Maker(standin=False)``).

The stub reads a call's taps through their pointer, by a per-symbol table that does not know the
new entry; ``_TAPS_AT`` gets its row here.  ``_ResampleEntry`` collects into this module's ``CASES``
(the base class appends to the torch_ops table, which must keep listing torch_ops' entries only).
"""
from __future__ import annotations

import ctypes

import torch

import fir_hip
import torch_ops_cases as tc
from torch_ops_cases import (I32, ROWLEN, STREAM, TAPS5, U8, X_DTYPE, Case, Maker, Stream, StubLib, run_case, _flat,
                             _IN, _OTHER, _ST, _rows_geometry, _set)

tc._TAPS_AT.setdefault("fir_resample_rows_dev", (5, lambda a: a[6], ctypes.c_int32))

ENTRY = "fir1d_fixed_rows_resample_dev"
CASES: list[Case] = []
UP, DECIM, PHASE = 3, 4, 1
__all__ = ["CASES", "ENTRY", "Maker", "StubLib", "run"]


class _ResampleEntry(tc._Entry):
    def _add(self, vid, mutate, error, check, **kw):
        CASES.append(Case(f"{self.entry}[{self.base}]-{vid}", self.entry, self.build, self.call, mutate, error,
                          self.expect, check, **kw))


def run(case: Case, mk: Maker, torch_resample, monkeypatch):
    """run_case with torch_resample in torch_ops' place: the stub replaces torch_resample.lib."""
    return run_case(case, mk, torch_resample, monkeypatch)


def _oshape(shape, ch, up=UP, decim=DECIM, phase=PHASE):
    return shape[:-1] + (len(range(phase, shape[-1] // ch * up, decim)) * ch,)


def _entries():
    for base, xdt, stage, ch, shape in (("u8", torch.uint8, U8, 1, (3, 40)), ("i16c2-i32", torch.int16, I32, 2, (3, 40)),
                                        ("i16-i32-1d", torch.int16, I32, 1, (40,))):
        odt = _ST[stage]
        oshape = _oshape(shape, ch)  # 40 frames * 3 -> 30 kept; 20 complex frames * 3 -> 15 kept = 30 values

        def build(mk, xdt=xdt, stage=stage, ch=ch, shape=shape, odt=odt, oshape=oshape):
            return dict(x=mk.dev(shape, xdt), hq=list(TAPS5), up=UP, decim=DECIM, phase=PHASE, frac=12, acc=32,
                        stage=stage, channels=ch, out=mk.dev(oshape, odt), stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_rows_resample_dev(a["x"], a["hq"], a["up"], a["decim"], a["phase"], a["frac"], a["acc"],
                                                     a["stage"], a["channels"], out=a["out"], stream=a["stream"])

        def expect(a):
            rows, width = _rows_geometry(a["x"], a["channels"])
            return "fir_resample_rows_dev", [a["x"].data_ptr(), _IN[a["x"].dtype], rows, width, a["channels"],
                                             _flat(a["hq"]), len(_flat(a["hq"])), a["up"], a["decim"], a["phase"], 12,
                                             32, a["stage"], a["out"].data_ptr(), STREAM]

        def reshaped(ch=ch, shape=shape, odt=odt, **kw):
            """The valid call with other rate arguments and the out they are due."""
            def mutate(mk, a):
                a.update(kw)
                a["out"] = mk.dev(_oshape(shape, ch, a["up"], a["decim"], a["phase"]), odt)
            return mutate

        e = _ResampleEntry(ENTRY, base, build, call, expect)
        e.out_variants("out", oshape, odt, _OTHER[odt], full_rate=shape)
        e.x_variants("x", shape, xdt, torch.float32, X_DTYPE)
        e.bad("x-other-dtype-int32", _set("x", lambda mk, a, s=shape: mk.dev(s, torch.int32)),
              r"x dtype must be uint8 or int16, got torch\.int32", f"{ENTRY}: x dtype")
        e.channels_variants(ROWLEN, 3)
        e.taps_variants("hq", 5)
        e.bad("stage-unknown", _set("stage", lambda mk, a: 2), "out_stage must be", "_out_dtype")
        e.bad("up-zero", _set("up", lambda mk, a: 0), "up must be >= 1", "resample_out_width: up")
        e.bad("up-negative", _set("up", lambda mk, a: -3), "up must be >= 1", "resample_out_width: up")
        e.bad("decim-zero", _set("decim", lambda mk, a: 0), "decim must be >= 1", "resample_out_width: decim")
        e.bad("decim-negative", _set("decim", lambda mk, a: -4), "decim must be >= 1", "resample_out_width: decim")
        e.bad("phase-is-decim", _set("phase", lambda mk, a: DECIM), r"phase must be in \[0, decim\)",
              "resample_out_width: phase")
        e.bad("phase-negative", _set("phase", lambda mk, a: -1), r"phase must be in \[0, decim\)",
              "resample_out_width: phase")
        # the out of another rate is refused by its shape
        e.bad("out-of-another-up", _set("up", lambda mk, a: UP - 1), r"out must be .* of shape", "_check_out: shape and dtype")
        e.bad("out-of-another-decim", _set("decim", lambda mk, a: DECIM + 1), r"out must be .* of shape",
              "_check_out: shape and dtype")
        e.bad("out-of-the-interpolator", _set("out", lambda mk, a, s=shape, odt=odt: mk.dev(s[:-1] + (s[-1] * UP,), odt)),
              r"out must be .* of shape", "_check_out: shape and dtype")
        # accepted: the forwards (up = 1, decim = 1, both), other phases, decim > up * width's share
        e.ok("up-1", reshaped(up=1))
        e.ok("decim-1", reshaped(decim=1, phase=0))
        e.ok("up-1-decim-1", reshaped(up=1, decim=1, phase=0))
        e.ok("phase-0", reshaped(phase=0))
        e.ok("phase-last", reshaped(phase=DECIM - 1))
        e.ok("up-16-decim-15", reshaped(up=16, decim=15, phase=14))
        e.ok("nothing-kept", reshaped(up=2, decim=1000, phase=999))
        e.ok("x-empty-rows", lambda mk, a, s=shape, o=oshape, xdt=xdt, odt=odt:
             a.update(x=mk.dev((0,) + s[1:], xdt), out=mk.dev((0,) + o[1:], odt)))
        e.ok("x-empty-width", lambda mk, a, s=shape, xdt=xdt, odt=odt:
             a.update(x=mk.dev(s[:-1] + (0,), xdt), out=mk.dev(s[:-1] + (0,), odt)))


_entries()
