"""The argument contract of fir_hip.torch_cplx as a table -- a test helper, not a test module.

Built like tests/torch_resample_cases.py on tests/torch_ops_cases.py, whose ``Case``, ``Maker``,
``StubLib`` and ``run_case`` it uses: per base (complex int16 -> int32 rows, -> u8 rows, a 1-D row)
one valid call of ``fir1d_fixed_rows_cplx_dev`` and variants that differ in exactly one argument,
each with the ``FirHipError`` text it must raise or, where the variant must be accepted, the exact
``fir_cplx_rows_dev`` call the stub library must record.  ``run`` runs one case against the stub:
nothing is launched, so the table needs no GPU (``Maker(standin=True)``) and is equally valid on
device tensors (``Maker(standin=False)``).

The stub reads a call's taps through their pointer, by a per-symbol table that does not know the
new entry; ``_TAPS_AT`` gets its row here, for the (taps, 2) layout: 2 * taps int32 behind argument
3.  ``_CplxEntry`` collects into this module's ``CASES`` (the base class appends to the torch_ops
table, which must keep listing torch_ops' entries only).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

import torch_ops_cases as tc
from torch_ops_cases import (I32, I32_MAX, I32_MIN, SMALL_MAX_TAPS, STREAM, U8, Case, Maker, Stream, StubLib, run_case,
                             _flat, _OTHER, _ST, _rows_geometry, _set)

tc._TAPS_AT.setdefault("fir_cplx_rows_dev", (3, lambda a: 2 * a[4], ctypes.c_int32))

ENTRY = "fir1d_fixed_rows_cplx_dev"
CASES: list[Case] = []
TAPS3 = [[-256, 100], [6656, 0], [-1024, -77]]
X_DTYPE = r"x dtype must be int16 \(interleaved re, im\), got torch\."
ODD = "row length must be a multiple of channels"
__all__ = ["CASES", "ENTRY", "Maker", "StubLib", "run"]


class _CplxEntry(tc._Entry):
    def _add(self, vid, mutate, error, check, **kw):
        CASES.append(Case(f"{self.entry}[{self.base}]-{vid}", self.entry, self.build, self.call, mutate, error,
                          self.expect, check, **kw))


def run(case: Case, mk: Maker, torch_cplx, monkeypatch):
    """run_case with torch_cplx in torch_ops' place: the stub replaces torch_cplx.lib."""
    return run_case(case, mk, torch_cplx, monkeypatch)


def _entries():
    for base, stage, shape in (("c16-i32", I32, (3, 40)), ("c16-u8", U8, (3, 40)), ("c16-i32-1d", I32, (40,))):
        odt = _ST[stage]

        def build(mk, stage=stage, shape=shape, odt=odt):
            return dict(x=mk.dev(shape, torch.int16), hq=[list(p) for p in TAPS3], frac=12, acc=32, stage=stage,
                        out=mk.dev(shape, odt), stream=Stream())

        def call(ops, a):
            return ops.fir1d_fixed_rows_cplx_dev(a["x"], a["hq"], a["frac"], a["acc"], a["stage"], out=a["out"],
                                                 stream=a["stream"])

        def expect(a):
            rows, width = _rows_geometry(a["x"], 2)
            h = a["hq"].h if hasattr(a["hq"], "h") else a["hq"]
            return "fir_cplx_rows_dev", [a["x"].data_ptr(), rows, width, _flat(h), len(_flat(h)) // 2, 12, 32, a["stage"],
                                         a["out"].data_ptr(), STREAM]

        e = _CplxEntry(ENTRY, base, build, call, expect)
        e.out_variants("out", shape, odt, _OTHER[odt])
        e.x_variants("x", shape, torch.int16, torch.float32, X_DTYPE + "float32")
        e.bad("x-uint8", _set("x", lambda mk, a, s=shape: mk.dev(s, torch.uint8)), X_DTYPE + "uint8", f"{ENTRY}: x dtype")
        e.bad("x-int32", _set("x", lambda mk, a, s=shape: mk.dev(s, torch.int32)), X_DTYPE + "int32", f"{ENTRY}: x dtype")
        odd = shape[:-1] + (shape[-1] - 1,)
        e.bad("x-odd-row", lambda mk, a, s=odd, odt=odt: a.update(x=mk.dev(s, torch.int16), out=mk.dev(s, odt)), ODD,
              "_rows_of(x, 2)")
        e.bad("x-one-value", lambda mk, a, odt=odt: a.update(x=mk.dev((1,), torch.int16), out=mk.dev((1,), odt)), ODD,
              "_rows_of(x, 2)")
        e.bad("x-0d", lambda mk, a, odt=odt: a.update(x=mk.dev((), torch.int16), out=mk.dev((), odt)), ODD, "_rows_of(x, 2)")
        e.bad("stage-unknown", _set("stage", lambda mk, a: 2), "out_stage must be", "_out_dtype")
        # the (taps, 2) layout
        c = "_taps_cplx_i32"
        pairs = r"non-empty \(taps, 2\) array"
        e.bad("taps-empty", _set("hq", lambda mk, a: []), pairs, c + ": shape")
        e.bad("taps-no-rows", _set("hq", lambda mk, a: np.ones((0, 2), np.int64)), pairs, c + ": shape")
        e.bad("taps-1d", _set("hq", lambda mk, a: [1, 2, 3, 4]), pairs, c + ": shape")
        e.bad("taps-three-columns", _set("hq", lambda mk, a: np.ones((2, 3), np.int64)), pairs, c + ": shape")
        e.bad("taps-3d", _set("hq", lambda mk, a: np.ones((3, 2, 1), np.int64)), pairs, c + ": shape")
        e.bad("taps-3d-of-pairs", _set("hq", lambda mk, a: np.ones((3, 1, 2), np.int64)), pairs, c + ": shape")
        e.bad("taps-float", _set("hq", lambda mk, a: np.ones((3, 2), np.float64)), "hq must be an integer array", c + ": dtype")
        e.bad("taps-complex", _set("hq", lambda mk, a: np.ones(3, np.complex64)), pairs, c + ": shape")
        e.bad("taps-complex-pairs", _set("hq", lambda mk, a: np.ones((3, 2), np.complex64)), "hq must be an integer array",
              c + ": dtype")
        e.bad("taps-bool", _set("hq", lambda mk, a: np.ones((3, 2), bool)), "hq must be an integer array", c + ": dtype")
        e.bad("taps-too-many", _set("hq", lambda mk, a: np.ones((SMALL_MAX_TAPS + 1, 2), np.int64)),
              "exceed the library limit", c + ": MAX_TAPS", max_taps=SMALL_MAX_TAPS)
        e.ok("taps-at-limit", _set("hq", lambda mk, a: np.ones((SMALL_MAX_TAPS, 2), np.int64)), max_taps=SMALL_MAX_TAPS)
        e.bad("taps-hr-2p31", _set("hq", lambda mk, a: [[1, 2], [2**31, 3]]), "must fit in int32", c + ": int32 range")
        e.bad("taps-hi-2p31", _set("hq", lambda mk, a: [[1, 2], [3, 2**31]]), "must fit in int32", c + ": int32 range")
        e.bad("taps-hi-below-int32", _set("hq", lambda mk, a: [[1, -2**31 - 1], [3, 4]]), "must fit in int32",
              c + ": int32 range")
        e.bad("taps-python-int-2p70", _set("hq", lambda mk, a: [[2**70, 0]]), "must fit in int32", c + ": int32 range")
        e.ok("taps-int32-ends", _set("hq", lambda mk, a: [[I32_MAX, I32_MIN], [I32_MIN, I32_MAX]]))
        e.ok("taps-one", _set("hq", lambda mk, a: [[4096, -1]]))
        e.ok("taps-int8-array", _set("hq", lambda mk, a: np.array([[1, -2], [3, 4]], np.int8)))
        e.ok("taps-real-only", _set("hq", lambda mk, a: [[5, 0], [6, 0]]))

        def held(mk, a):
            from fir_hip import torch_cplx
            a["hq"] = torch_cplx.CplxTaps(TAPS3)
        e.ok("taps-held", held)
        e.ok("x-empty-rows", lambda mk, a, s=shape, odt=odt:
             a.update(x=mk.dev((0,) + s[1:], torch.int16), out=mk.dev((0,) + s[1:], odt)))
        e.ok("x-empty-width", lambda mk, a, s=shape, odt=odt:
             a.update(x=mk.dev(s[:-1] + (0,), torch.int16), out=mk.dev(s[:-1] + (0,), odt)))
        e.ok("x-one-frame", lambda mk, a, s=shape, odt=odt:
             a.update(x=mk.dev(s[:-1] + (2,), torch.int16), out=mk.dev(s[:-1] + (2,), odt)))


_entries()
assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
