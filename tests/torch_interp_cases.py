"""The argument contract of fir_hip.torch_interp as a table -- a test helper, not a test module.

In the style of tests/torch_ops_cases.py, whose ``Case``, ``Maker``, ``StubLib`` and ``run_case`` it
uses: per base (u8 -> u8 of one channel, complex int16 -> int32) one valid call of
``fir1d_fixed_rows_interp_dev`` and variants that differ in exactly one argument, each with the
``FirHipError`` text it must raise or, where the variant must be accepted, the exact
``fir_interp_rows_dev`` call the stub library must record.  ``run`` runs one case against the stub:
nothing is launched, so the table needs no GPU (``Maker(standin=True)``) and is equally valid on
device tensors (``Maker(standin=False)``).

The stub reads a call's taps through their pointer, by a per-symbol table that does not know the
new entry; ``_TAPS_AT`` gets its row here.  ``_InterpEntry`` collects into this module's ``CASES``
(the base class appends to the torch_ops table, which must keep listing torch_ops' entries only).
"""
from __future__ import annotations

import ctypes

import torch

import fir_hip
import torch_ops_cases as tc
from torch_ops_cases import (I32, ROWLEN, STREAM, TAPS5, U8, X_DTYPE, Case, Maker, Stream, StubLib, run_case, _flat,
                             _IN, _OTHER, _ST, _rows_geometry, _set)

tc._TAPS_AT.setdefault("fir_interp_rows_dev", (5, lambda a: a[6], ctypes.c_int32))

ENTRY = "fir1d_fixed_rows_interp_dev"
CASES: list[Case] = []
UP = 4
__all__ = ["CASES", "ENTRY", "Maker", "StubLib", "run"]


class _InterpEntry(tc._Entry):
    def _add(self, vid, mutate, error, check, **kw):
        CASES.append(Case(f"{self.entry}[{self.base}]-{vid}", self.entry, self.build, self.call, mutate, error,
                          self.expect, check, **kw))


def run(case: Case, mk: Maker, torch_interp, monkeypatch):
    """run_case with torch_interp in torch_ops' place: the stub replaces torch_interp.lib."""
    return run_case(case, mk, torch_interp, monkeypatch)


def _entries():
    for base, xdt, stage, ch, shape in (("u8", torch.uint8, U8, 1, (3, 40)), ("i16c2-i32", torch.int16, I32, 2, (3, 40)),
                                        ("i16-i32-1d", torch.int16, I32, 1, (40,))):
        odt = _ST[stage]
        oshape = shape[:-1] + (shape[-1] * UP,)

        def build(mk, xdt=xdt, stage=stage, ch=ch, shape=shape, odt=odt, oshape=oshape):
            return dict(x=mk.dev(shape, xdt), hq=list(TAPS5), up=UP, frac=12, acc=32, stage=stage, channels=ch,
                        out=mk.dev(oshape, odt), stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_rows_interp_dev(a["x"], a["hq"], a["up"], a["frac"], a["acc"], a["stage"],
                                                   a["channels"], out=a["out"], stream=a["stream"])

        def expect(a):
            rows, width = _rows_geometry(a["x"], a["channels"])
            return "fir_interp_rows_dev", [a["x"].data_ptr(), _IN[a["x"].dtype], rows, width, a["channels"],
                                           _flat(a["hq"]), len(_flat(a["hq"])), a["up"], 12, 32, a["stage"],
                                           a["out"].data_ptr(), STREAM]

        e = _InterpEntry(ENTRY, base, build, call, expect)
        e.out_variants("out", oshape, odt, _OTHER[odt], full_rate=shape)
        e.x_variants("x", shape, xdt, torch.float32, X_DTYPE)
        e.bad("x-other-dtype-int32", _set("x", lambda mk, a, s=shape: mk.dev(s, torch.int32)),
              r"x dtype must be uint8 or int16, got torch\.int32", f"{ENTRY}: x dtype")
        e.channels_variants(ROWLEN, 3)
        e.taps_variants("hq", 5)
        e.bad("stage-unknown", _set("stage", lambda mk, a: 2), "out_stage must be", "_out_dtype")
        e.bad("up-zero", _set("up", lambda mk, a: 0), "up must be >= 1", "interp_out_width: up")
        e.bad("up-negative", _set("up", lambda mk, a: -4), "up must be >= 1", "interp_out_width: up")
        # up = 1: the output has x's shape; up = 3: a width that is no power of two
        for up in (1, 3):
            e.ok(f"up-{up}", lambda mk, a, up=up, s=shape, odt=odt: a.update(up=up, out=mk.dev(s[:-1] + (s[-1] * up,), odt)))
        e.bad("out-of-another-up", _set("up", lambda mk, a: UP - 1), r"out must be .* of shape", "_check_out: shape and dtype")
        e.ok("x-empty-rows", lambda mk, a, s=shape, o=oshape, xdt=xdt, odt=odt:
             a.update(x=mk.dev((0,) + s[1:], xdt), out=mk.dev((0,) + o[1:], odt)))
        e.ok("x-empty-width", lambda mk, a, s=shape, xdt=xdt, odt=odt:
             a.update(x=mk.dev(s[:-1] + (0,), xdt), out=mk.dev(s[:-1] + (0,), odt)))


_entries()
