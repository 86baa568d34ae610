"""The argument contract of fir_hip.torch_cstream, run without a GPU, as tests/test_torch_cplx_contract.py
does for torch_cplx: stand-in tensors (CPU memory, reporting cuda:0 / cuda:1, tests/torch_ops_cases.py),
an explicit ``out=`` and an explicit stream stand-in, against a stub library that records calls and
launches nothing.  A refused call must raise FirHipError with its text before any library call; an
accepted one must reach exactly ``fir_cplx_stream_block_dev`` with the expected arguments."""
from __future__ import annotations

import ctypes
import inspect

import pytest
import torch

import fir_hip
import torch_ops_cases as tc
from fir_hip import cstream, torch_cplx, torch_cstream, torch_ops

ENTRY = "fir_cplx_stream_block_dev"
HQ = [[1, -2], [3, 4], [-5, 6]]  # 3 taps: H = 2 frames
ROWS, WIDTH, D, PHASE = 4, 16, 3, 1
OW = len(range(PHASE, WIDTH, D))


class _Stub(tc.StubLib):
    """tc.StubLib, reading the taps of the new entry (argument 4, argument 5 of them) during the call."""

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if name != ENTRY:
            return fn

        def rec(*args):
            a = list(args)
            a[4] = tuple((ctypes.c_int32 * (2 * a[5])).from_address(a[4].value))
            return fn(*a)

        return rec


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(cstream, "lib", lambda: s)
    return s


def _args(mk, **over):
    a = dict(x=mk.dev((ROWS, 2 * WIDTH), torch.int16), hist_in=mk.dev((ROWS, 4), torch.int16),
             hist_out=mk.dev((ROWS, 4), torch.int16), out=mk.dev((ROWS, 2 * OW), torch.int32))
    for k, v in over.items():
        a[k] = v(mk, a) if callable(v) else v
    return a


def _call(a, **kw):
    return torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(a["x"], a["hist_in"], a["hist_out"], kw.pop("hq", HQ), D, PHASE,
                                                               out=a["out"], stream=tc.Stream(), **kw)


REFUSED = {
    "x-host": (dict(x=lambda mk, a: mk.host((ROWS, 2 * WIDTH), torch.int16)), "x must be a device tensor"),
    "x-strided": (dict(x=lambda mk, a: mk.strided((ROWS, 2 * WIDTH), torch.int16)), "x must be contiguous"),
    "x-int32": (dict(x=lambda mk, a: mk.dev((ROWS, 2 * WIDTH), torch.int32)), "x dtype must be int16"),
    "x-odd": (dict(x=lambda mk, a: mk.dev((ROWS, 2 * WIDTH - 1), torch.int16)), "multiple of channels"),
    "hist_in-host": (dict(hist_in=lambda mk, a: mk.host((ROWS, 4), torch.int16)), "hist_in must be a device tensor"),
    "hist_in-strided": (dict(hist_in=lambda mk, a: mk.strided((ROWS, 4), torch.int16)), "hist_in must be contiguous"),
    "hist_in-other-device": (dict(hist_in=lambda mk, a: mk.other((ROWS, 4), torch.int16)), "hist_in must be on cuda:0"),
    "hist_in-int32": (dict(hist_in=lambda mk, a: mk.dev((ROWS, 4), torch.int32)), "hist_in must be torch.int16 of shape"),
    "hist_in-frames": (dict(hist_in=lambda mk, a: mk.dev((ROWS, 6), torch.int16)), "hist_in must be torch.int16 of shape"),
    "hist_in-rows": (dict(hist_in=lambda mk, a: mk.dev((ROWS + 1, 4), torch.int16)), "hist_in must be torch.int16 of shape"),
    "hist_out-host": (dict(hist_out=lambda mk, a: mk.host((ROWS, 4), torch.int16)), "hist_out must be a device tensor"),
    "hist_out-strided": (dict(hist_out=lambda mk, a: mk.strided((ROWS, 4), torch.int16)), "hist_out must be contiguous"),
    "hist_out-other-device": (dict(hist_out=lambda mk, a: mk.other((ROWS, 4), torch.int16)), "hist_out must be on cuda:0"),
    "hist_out-uint8": (dict(hist_out=lambda mk, a: mk.dev((ROWS, 8), torch.uint8)), "hist_out must be torch.int16 of shape"),
    "hist_out-frames": (dict(hist_out=lambda mk, a: mk.dev((ROWS, 2), torch.int16)), "hist_out must be torch.int16 of shape"),
    "out-host": (dict(out=lambda mk, a: mk.host((ROWS, 2 * OW), torch.int32)), "out must be a device tensor"),
    "out-full-rate": (dict(out=lambda mk, a: mk.dev((ROWS, 2 * WIDTH), torch.int32)), "out must be torch.int32 of shape"),
    "out-uint8": (dict(out=lambda mk, a: mk.dev((ROWS, 2 * OW), torch.uint8)), "out must be torch.int32 of shape"),
    "out-other-device": (dict(out=lambda mk, a: mk.other((ROWS, 2 * OW), torch.int32)), "out must be on cuda:0"),
    # overlaps: every output against every input, and the two outputs against each other
    "out-on-x": (dict(out=lambda mk, a: mk.alias(a["x"], 0, (ROWS, 2 * OW), torch.int32)), r"out must not overlap the input \(x\)"),
    "out-on-hist_in": (dict(out=lambda mk, a: mk.alias(a["hist_in"], 0, (ROWS, 2 * OW), torch.int32)),
                       r"out must not overlap the input \(hist_in\)"),
    "hist_out-is-hist_in": (dict(hist_out=lambda mk, a: a["hist_in"]), r"hist_out must not overlap the input \(hist_in\)"),
    "hist_out-into-hist_in": (dict(hist_out=lambda mk, a: mk.alias(a["hist_in"], 4 * ROWS * 2 - 2, (ROWS, 4), torch.int16)),
                              r"hist_out must not overlap the input \(hist_in\)"),
    "hist_out-on-x": (dict(hist_out=lambda mk, a: mk.alias(a["x"], 64, (ROWS, 4), torch.int16)),
                      r"hist_out must not overlap the input \(x\)"),
    "hist_out-on-out": (dict(hist_out=lambda mk, a: mk.alias(a["out"], 8, (ROWS, 4), torch.int16)), "hist_out must not overlap out"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_before_any_library_call(name, stub):
    over, text = REFUSED[name]
    with pytest.raises(fir_hip.FirHipError, match=text):
        _call(_args(tc.Maker(standin=True), **over))
    assert stub.calls == []


def test_scalar_refusals_come_before_any_library_call(stub):
    mk = tc.Maker(standin=True)
    for kw, text in ((dict(out_stage=7), "out_stage must be"), (dict(hq=[1, 2, 3]), r"non-empty \(taps, 2\) array")):
        with pytest.raises(fir_hip.FirHipError, match=text):
            _call(_args(mk), **kw)
    a = _args(mk)
    for D_, phase, text in ((0, 0, "decim must be >= 1"), (3, 3, "phase must be in"), (3, -1, "phase must be in")):
        with pytest.raises(fir_hip.FirHipError, match=text):
            torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(a["x"], a["hist_in"], a["hist_out"], HQ, D_, phase, out=a["out"],
                                                                stream=tc.Stream())
    assert stub.calls == []


def test_accepted_calls_reach_the_entry(stub):
    mk = tc.Maker(standin=True)
    a = _args(mk)
    assert _call(a) is a["out"]
    flat = (1, -2, 3, 4, -5, 6)
    assert stub.calls == [(ENTRY, [a["x"].data_ptr(), a["hist_in"].data_ptr(), ROWS, WIDTH, flat, 3, D, PHASE, 12, 32,
                                   fir_hip.OUT_I32, a["out"].data_ptr(), a["hist_out"].data_ptr(), tc.STREAM])]
    # either history may be None: NULL
    stub.calls.clear()
    b = _args(mk, hist_in=None, hist_out=None)
    assert _call(b, hq=torch_cstream.CplxTaps(HQ), frac_bits=7, acc_bits=24) is b["out"]
    assert stub.calls == [(ENTRY, [b["x"].data_ptr(), 0, ROWS, WIDTH, flat, 3, D, PHASE, 7, 24, fir_hip.OUT_I32,
                                   b["out"].data_ptr(), 0, tc.STREAM])]
    # leading axes are rows; the u8 stage; one tap: histories of no frames
    stub.calls.clear()
    c = dict(x=mk.dev((2, 3, 10), torch.int16), hist_in=mk.dev((2, 3, 0), torch.int16), hist_out=mk.dev((2, 3, 0), torch.int16),
             out=mk.dev((2, 3, 4), torch.uint8))
    assert _call(c, hq=[[9, 9]], out_stage=fir_hip.OUT_U8_SAT) is c["out"]
    assert stub.calls[0][1][2:11] == [6, 5, (9, 9), 1, D, PHASE, 12, 32, fir_hip.OUT_U8_SAT]
    # rows of no frames still count as rows: the history moves
    stub.calls.clear()
    d = dict(x=mk.dev((ROWS, 0), torch.int16), hist_in=mk.dev((ROWS, 4), torch.int16), hist_out=mk.dev((ROWS, 4), torch.int16),
             out=mk.dev((ROWS, 0), torch.int32))
    assert _call(d) is d["out"] and stub.calls[0][1][2:4] == [ROWS, 0]


def test_push_refuses_a_wrong_leading_shape_and_carries_the_state(stub):
    mk = tc.Maker(standin=True)
    s = torch_cstream.CplxDecimStream(HQ, D, (ROWS,), phase=PHASE, device="cpu")
    for shape in ((ROWS + 1, 8), (8,), (1, ROWS, 8), (2, 2, 8)):
        with pytest.raises(fir_hip.FirHipError, match="leading axes"):
            s.push(mk.dev(shape, torch.int16), stream=tc.Stream())
    assert stub.calls == [] and (s.phase, s.frames_in, s.frames_out) == (PHASE, 0, 0)
    for bad in ((0, 0), (3, 3)):
        with pytest.raises(fir_hip.FirHipError):
            torch_cstream.CplxDecimStream(HQ, bad[0], (ROWS,), phase=bad[1], device="cpu")
    with pytest.raises(fir_hip.FirHipError, match="phase must be in"):
        s.reset(phase=D)
    with pytest.raises(fir_hip.FirHipError, match="history must be"):
        s.reset(torch.zeros((ROWS, 6), dtype=torch.int16))
    # accepted pushes: the two histories alternate, the phase and the counters follow the header's rule
    s._hist = [mk.dev((ROWS, 4), torch.int16) for _ in range(2)]
    ptrs = [h.data_ptr() for h in s._hist]
    phase, fin, fout = PHASE, 0, 0
    for k, width in enumerate((16, 0, 1, 7)):
        ow = len(range(phase, width, D))
        x, out = mk.dev((ROWS, 2 * width), torch.int16), mk.dev((ROWS, 2 * ow), torch.int32)
        assert s.push(x, out=out, stream=tc.Stream()) is out
        name, a = stub.calls[-1]
        assert name == ENTRY and a[1] == ptrs[k % 2] and a[12] == ptrs[1 - k % 2] and a[3] == width and a[7] == phase
        phase, fin, fout = phase + ow * D - width, fin + width, fout + ow
        assert (s.phase, s.frames_in, s.frames_out) == (phase, fin, fout) and 0 <= phase < D
    assert len(stub.calls) == 4


def test_module_surface():
    public = {n for n, v in vars(torch_cstream).items()
              if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == torch_cstream.__name__}
    assert public | {"CplxTaps"} == {"CplxTaps", "CplxDecimStream", "fir1d_fixed_rows_cplx_decim_block_dev"} == set(torch_cstream.__all__)
    assert torch_cstream.CplxTaps is torch_cplx.CplxTaps
    for name in ("_check_dev", "_check_in", "_rows_of", "_out_dtype", "_check_out", "_no_overlap", "_stream_ptr"):
        assert getattr(torch_cstream, name) is getattr(torch_ops, name), name
    sig = inspect.signature(torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev)
    assert list(sig.parameters) == ["x", "hist_in", "hist_out", "hq", "decim", "phase", "frac_bits", "acc_bits", "out_stage",
                                    "out", "stream"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        phase=0, frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, out=None, stream=None)
    sig = inspect.signature(torch_cstream.CplxDecimStream.__init__)
    assert list(sig.parameters) == ["self", "hq", "decim", "lead_shape", "phase", "frac_bits", "acc_bits", "out_stage", "device"]
    assert sig.parameters["phase"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["device"].default is inspect.Parameter.empty
    assert "stream-ordered" in torch_cstream.CplxDecimStream.__doc__
