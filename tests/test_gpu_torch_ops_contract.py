"""GPU: the argument contract of fir_hip.torch_ops on real device tensors, and parity through the
device entries for the argument forms no other test passes.

1. ``test_case``: the table of tests/torch_ops_cases.py on real ``cuda:0`` tensors, still against
   the stub library (nothing is launched: a refused case never reaches the real library, here or
   anywhere).  It shows that the stand-ins of tests/test_torch_ops_contract.py hide no difference.
   ``test_empty_problems_allocate_the_result``: the empty problems with ``out=None``, stub library.
2. Parity with the real library, bit-exact against the C oracle (float64 as uint64 views): leading
   axes, 1-D and 0-d inputs; bank taps at the int32 ends; a two-channel bank; every entry called
   twice into the same ``out`` (and ``work`` of exactly the stated size, inside guard bands).

Rows of 264 or 520 samples cross the 256-sample restore wave and the ragged ends of the u8 and
int16 register tiles.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
import torch_ops_cases as tc
from conftest import same_metrics
from fir_hip import torch_ops
from guarded import guarded_output
from ideal2d_ref import ideal2d
from oracle import c_oracle, fir_oracle as fo

DEV = torch.device("cuda:0")
U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
STAGES = (U8, I32)
_TDT = {U8: torch.uint8, I32: torch.int32}
CLIP, NORMALIZE = fir_hip.RESTORE_CLIP, fir_hip.RESTORE_NORMALIZE
TAPS5 = [-256, -1024, 6656, -1024, -256]
H5 = [-0.0625, -0.25, 1.625, -0.25, -0.0625]


# ---- 1. the table, on device tensors, against the stub -----------------------------------------
@pytest.mark.parametrize("case", tc.CASES, ids=[c.id for c in tc.CASES])
def test_case(case, monkeypatch):
    tc.run_case(case, tc.Maker(standin=False), torch_ops, monkeypatch)


def _empty_calls():
    """(id, call(ops, x) -> result, x shape, x dtype, result shape, result dtype, C entry)."""
    bank = [[1, 2, 1], [3, 4, 3]]
    k3 = np.ones((3, 3), np.int64)
    return [
        ("rows", lambda o, x: o.fir1d_fixed_rows_dev(x, TAPS5, out_stage=I32), (0, 40), torch.int16, (0, 40), torch.int32,
         "fir1d_fixed_rows_dev"),
        ("rows-width0", lambda o, x: o.fir1d_fixed_rows_dev(x, TAPS5, out_stage=U8), (3, 0), torch.uint8, (3, 0), torch.uint8,
         "fir1d_fixed_rows_dev"),
        ("decim", lambda o, x: o.fir1d_fixed_rows_decim_dev(x, TAPS5, 4, 1, out_stage=U8), (0, 40), torch.uint8, (0, 10),
         torch.uint8, "fir_decim_rows_dev"),
        ("decim-width-below-phase", lambda o, x: o.fir1d_fixed_rows_decim_dev(x, TAPS5, 4, 3), (3, 2), torch.uint8, (3, 0),
         torch.int32, "fir_decim_rows_dev"),
        ("multi", lambda o, x: o.fir1d_fixed_rows_multi_dev(x, bank), (0, 40), torch.uint8, (2, 0, 40), torch.uint8,
         "fir1d_fixed_rows_multi_dev"),
        ("images", lambda o, x: o.fir1d_fixed_images_multi_dev([x], bank)[0], (0, 40), torch.uint8, (2, 0, 40), torch.uint8,
         "fir1d_fixed_images_multi_dev"),
        ("segment", lambda o, x: o.fir1d_fixed_segment_dev(x, TAPS5, None, None), (0,), torch.int16, (0,), torch.int32,
         "fir1d_fixed_segment_dev"),
        ("fir2d", lambda o, x: o.fir2d_fixed_dev(x, k3), (0, 16), torch.uint8, (0, 16), torch.uint8, "fir2d_fixed_frames_dev"),
        ("fir2d-no-frames", lambda o, x: o.fir2d_fixed_dev(x, k3, out_stage=I32), (0, 5, 16), torch.uint8, (0, 5, 16),
         torch.int32, "fir2d_fixed_frames_dev"),
        ("fir2d-ideal", lambda o, x: o.fir2d_ideal_dev(x, np.ones((3, 3))), (5, 0), torch.uint8, (5, 0), torch.float64,
         "fir2d_ideal_frames_dev"),
        ("ideal-rows", lambda o, x: o.fir1d_ideal_rows_dev(x, H5), (0, 40), torch.uint8, (0, 40), torch.float64,
         "fir1d_ideal_rows_dev"),
        ("restore-clip", lambda o, x: o.restore_u8_dev(x, CLIP), (0, 40), torch.float64, (0, 40), torch.uint8,
         "fir_restore_u8_dev"),
        ("restore-normalize", lambda o, x: o.restore_u8_dev(x, NORMALIZE), (0,), torch.float64, (0,), torch.uint8,
         "fir_restore_u8_dev"),
        ("metrics", lambda o, x: o.compare_metrics_dev(x, torch.empty((0,), dtype=torch.uint8, device=DEV)), (0,),
         torch.float64, (9,), torch.float64, "fir_compare_metrics_dev"),
    ]


@pytest.mark.parametrize("name,call,xshape,xdt,shape,dtype,symbol", _empty_calls(), ids=[c[0] for c in _empty_calls()])
def test_empty_problems_allocate_the_result(name, call, xshape, xdt, shape, dtype, symbol, monkeypatch):
    """numel() == 0 with out=None: a device tensor of the right shape and dtype comes back, and
    the C entry is called once (it returns without a launch; the stub records the call)."""
    stub = tc.StubLib()
    monkeypatch.setattr(torch_ops, "lib", lambda: stub)
    y = call(torch_ops, torch.empty(xshape, dtype=xdt, device=DEV))
    assert tuple(y.shape) == shape and y.dtype == dtype and y.device == DEV
    assert [c[0] for c in stub.calls] == [symbol]


# ---- 2. parity with the real library -----------------------------------------------------------
def _same(y: torch.Tensor, want: np.ndarray, tag) -> None:
    got = y.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    got, want = got.reshape(-1), np.ascontiguousarray(want).reshape(-1)  # flat: a 0-d array has no uint64 view
    if got.dtype == np.float64:
        got, want = got.view(np.uint64), want.view(np.uint64)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{tag}: {bad.size} of {want.size} outputs differ from the oracle; the first at flat "
                             f"index {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}")


def _samples(rng, shape, dtype):
    lo, hi = (0, 256) if dtype == np.uint8 else (-32768, 32768)
    return np.asarray(rng.integers(lo, hi, shape), dtype=dtype)


def _decimated(full2: np.ndarray, ch: int, D: int, phase: int) -> np.ndarray:
    rows, rowlen = full2.shape
    return np.ascontiguousarray(full2.reshape(rows, rowlen // ch, ch)[:, phase::D]).reshape(rows, -1)


BANK3 = np.array([[1365, 1365, 1366], [1024, 2048, 1024], [-4096, 8191, -4095]], np.int64)
# a 0-d tensor is a row of one sample: no whole two-channel frame (refused: the table's channels cases)
AXES = [("u8", np.uint8, 1, s) for s in ((2, 3, 264), (264,), ())] + [("i16c2", np.int16, 2, s) for s in ((2, 3, 264), (264,))]


@pytest.mark.parametrize("name,dtype,ch,shape", AXES, ids=[f"{a[0]}-{a[3]}" for a in AXES])
def test_leading_axes(name, dtype, ch, shape):
    """x of shape (2, 3, 264), (264,) and (): each entry equals the oracle on x.reshape(rows, -1),
    reshaped back."""
    rng = np.random.default_rng(len(shape) * 10 + ch)
    co = c_oracle()
    x = _samples(rng, shape, dtype)
    x2 = x.reshape(-1, shape[-1] if shape else 1)
    xd = torch.from_numpy(x).to(DEV)
    D, phase = 4, 1
    for stage in STAGES:
        full2 = co.fir1d_rows(x2, TAPS5, 12, 32, stage, channels=ch)
        _same(torch_ops.fir1d_fixed_rows_dev(xd, TAPS5, 12, 32, stage, ch), full2.reshape(shape), (name, shape, stage))
        want = _decimated(full2, ch, D, phase)
        got = torch_ops.fir1d_fixed_rows_decim_dev(xd, TAPS5, D, phase, 12, 32, stage, ch)
        _same(got, want.reshape(tuple(shape[:-1]) + (want.shape[1],)), (name, shape, stage, "decim"))
        got = torch_ops.fir1d_fixed_rows_multi_dev(xd, BANK3, 12, 32, stage, ch)
        want = np.stack([co.fir1d_rows(x2, h, 12, 32, stage, channels=ch).reshape(shape) for h in BANK3])
        _same(got, want, (name, shape, stage, "multi"))
    if dtype == np.uint8:
        ideal2 = co.fir1d_ideal_rows(x2, H5)
        yi = torch_ops.fir1d_ideal_rows_dev(xd, H5)
        _same(yi, ideal2.reshape(shape), (name, shape, "ideal"))
        _same(torch_ops.restore_u8_dev(yi, CLIP), fo.to_u8_clip(ideal2).reshape(shape), (name, shape, "clip"))
        _same(torch_ops.restore_u8_dev(yi, NORMALIZE), fo.to_u8_normalized(ideal2).reshape(shape), (name, shape, "normalize"))


def _ends_bank(rng) -> np.ndarray:
    """Three filters of 9 taps whose rows hold 2**31 - 1 and -2**31."""
    bank = rng.integers(-2000, 2001, (3, 9)).astype(np.int64)
    bank[0, 4], bank[1, 0], bank[2, 8], bank[2, 1] = tc.I32_MAX, tc.I32_MIN, tc.I32_MAX, tc.I32_MIN
    return bank


def test_bank_taps_at_the_int32_ends():
    """acc_bits = 64, frac_bits = 20, int16 samples with |x| <= 100, 9 taps: every sum is below
    9 * 100 * 2^31 < 2^41, so the oracle's 64-bit sums are exact.  Through fir1d_fixed_rows_multi_dev
    and ImagesMultiPlan, each filter equals the oracle.  One unit further (a tap of 2**31, which a
    plain int32 cast wraps to -2**31) the answer differs, which is asserted on the CPU alone: the GPU
    is never given the refused tap."""
    rng = np.random.default_rng(64)
    co = c_oracle()
    bank = _ends_bank(rng)
    xs = [rng.integers(-100, 101, s).astype(np.int16) for s in ((5, 264), (2, 520))]
    xd = [torch.from_numpy(x).to(DEV) for x in xs]
    for stage in STAGES:
        want = [np.stack([co.fir1d_rows(x, h, 20, 64, stage) for h in bank]) for x in xs]
        for x, w in zip(xd, want):
            _same(torch_ops.fir1d_fixed_rows_multi_dev(x, bank, 20, 64, stage), w, ("multi", stage, tuple(x.shape)))
        outs = torch_ops.ImagesMultiPlan(xd, bank, 20, 64, stage).launch()
        for o, w in zip(outs, want):
            _same(o, w, ("images", stage, tuple(o.shape)))
    past = bank[0].copy()
    past[4] = 2**31
    wrapped = past.astype(np.int32).astype(np.int64)
    assert wrapped[4] == -2**31
    x64 = xs[0].astype(np.int64)
    assert not np.array_equal(fo.wrap_round(fo._mac_rows(x64, past), 20, 64), fo.wrap_round(fo._mac_rows(x64, wrapped), 20, 64))
    with pytest.raises(fir_hip.FirHipError, match="must fit in int32"):
        torch_ops._bank_i32(np.stack([past, bank[1]]))


def test_rows_multi_two_channels():
    rng = np.random.default_rng(2)
    co = c_oracle()
    x = _samples(rng, (5, 2 * 520), np.int16)
    xd = torch.from_numpy(x).to(DEV)
    for stage in STAGES:
        got = torch_ops.fir1d_fixed_rows_multi_dev(xd, BANK3, 12, 32, stage, channels=2)
        for f, h in enumerate(BANK3):
            _same(got[f], co.fir1d_rows(x, h, 12, 32, stage, channels=2), (stage, f))


# ---- out= and work= reuse: the second call's result is the oracle's, nothing of the first survives
def _twice(rng, make_x, run, want, tag):
    """run(x_dev) writes the shared output and returns it; two calls with different inputs."""
    for rep in range(2):
        x = make_x(rng)
        y = run(torch.from_numpy(x).to(DEV) if isinstance(x, np.ndarray) else [torch.from_numpy(a).to(DEV) for a in x])
        torch.cuda.synchronize()
    w = want(x)
    if isinstance(y, torch.Tensor):
        _same(y, w, tag)
    else:
        for i, (a, b) in enumerate(zip(y, w)):
            _same(a, b, tag + (i,))


REUSE = [("u8", np.uint8, 1, U8), ("u8-i32", np.uint8, 1, I32), ("i16c2-i32", np.int16, 2, I32)]


@pytest.mark.parametrize("name,dtype,ch,stage", REUSE, ids=[r[0] for r in REUSE])
def test_out_reuse_fixed_1d(name, dtype, ch, stage):
    rng = np.random.default_rng(REUSE.index((name, dtype, ch, stage)))
    co = c_oracle()
    shape, D, phase = (3, 264 * ch), 4, 1
    odt = _TDT[stage]
    make = lambda r: _samples(r, shape, dtype)  # noqa: E731
    out = torch.empty(shape, dtype=odt, device=DEV)
    _twice(rng, make, lambda x: torch_ops.fir1d_fixed_rows_dev(x, TAPS5, 12, 32, stage, ch, out=out),
           lambda x: co.fir1d_rows(x, TAPS5, 12, 32, stage, channels=ch), (name, "rows"))
    ow = fir_hip.decim_out_width(264, D, phase) * ch
    dout = torch.empty((3, ow), dtype=odt, device=DEV)
    _twice(rng, make, lambda x: torch_ops.fir1d_fixed_rows_decim_dev(x, TAPS5, D, phase, 12, 32, stage, ch, out=dout),
           lambda x: _decimated(co.fir1d_rows(x, TAPS5, 12, 32, stage, channels=ch), ch, D, phase), (name, "decim"))
    mout = torch.empty((3,) + shape, dtype=odt, device=DEV)
    _twice(rng, make, lambda x: torch_ops.fir1d_fixed_rows_multi_dev(x, BANK3, 12, 32, stage, ch, out=mout),
           lambda x: np.stack([co.fir1d_rows(x, h, 12, 32, stage, channels=ch) for h in BANK3]), (name, "multi"))
    shapes = [(3, 264 * ch), (2, 520 * ch)]
    iouts = [torch.empty((3,) + shapes[0], dtype=odt, device=DEV), [torch.empty(shapes[1], dtype=odt, device=DEV) for _ in BANK3]]
    _twice(rng, lambda r: [_samples(r, s, dtype) for s in shapes],
           lambda xs: [o if isinstance(o, torch.Tensor) else torch.stack(o) for o in
                       torch_ops.fir1d_fixed_images_multi_dev(xs, BANK3, 12, 32, stage, ch, outs=iouts)],
           lambda xs: [np.stack([co.fir1d_rows(x, h, 12, 32, stage, channels=ch) for h in BANK3]) for x in xs], (name, "images"))
    # a segment with both halos: one launch, and rows + edges, into the same out
    n = 520 * ch
    hl_n, hr_n = (v * ch for v in fo.halo_sizes(5))
    sout = torch.empty((n,), dtype=odt, device=DEV)

    def seg_inputs(r):
        return [_samples(r, (n,), dtype), _samples(r, (hl_n,), dtype), _samples(r, (hr_n,), dtype)]

    def seg_want(p):
        return [co.fir1d_rows(p[0], TAPS5, 12, 32, stage, channels=ch, halo_left=p[1], halo_right=p[2])]

    def edges(p):
        torch_ops.fir1d_fixed_rows_dev(p[0], TAPS5, 12, 32, stage, ch, out=sout)
        return [torch_ops.fir1d_fixed_edges_dev(p[0], TAPS5, sout, p[1], p[2], 12, 32, stage, ch)]

    _twice(rng, seg_inputs, lambda p: [torch_ops.fir1d_fixed_segment_dev(p[0], TAPS5, p[1], p[2], 12, 32, stage, ch, out=sout)],
           seg_want, (name, "segment"))
    _twice(rng, seg_inputs, edges, seg_want, (name, "edges"))


def test_out_reuse_2d_and_ideal():
    rng = np.random.default_rng(5)
    co = c_oracle()
    k = np.array([[0, -512, 0], [-512, 6144, -512], [0, -512, 0]], np.int64)
    h2 = rng.standard_normal((3, 3))
    shape = (2, 17, 264)
    make = lambda r: _samples(r, shape, np.uint8)  # noqa: E731
    for stage in STAGES:
        out = torch.empty(shape, dtype=_TDT[stage], device=DEV)
        _twice(rng, make, lambda x: torch_ops.fir2d_fixed_dev(x, k, 12, 32, stage, out=out),
               lambda x: np.stack([co.fir2d(f, k, 12, 32, stage) for f in x]), ("fir2d", stage))
    out = torch.empty(shape, dtype=torch.float64, device=DEV)
    _twice(rng, make, lambda x: torch_ops.fir2d_ideal_dev(x, h2, out=out), lambda x: np.stack([ideal2d(f, h2) for f in x]),
           ("fir2d_ideal",))
    _twice(rng, make, lambda x: torch_ops.fir1d_ideal_rows_dev(x, H5, out=out), lambda x: co.fir1d_ideal_rows(x, H5),
           ("ideal_rows",))


@pytest.mark.parametrize("policy", [CLIP, NORMALIZE], ids=["clip", "normalize"])
def test_out_and_work_reuse_restore(policy):
    """work of exactly fir_restore_work_bytes(), out and work inside guard bands."""
    rng = np.random.default_rng(policy)
    shape = (3, 264)
    out, check = guarded_output(shape, torch.uint8, device=DEV)
    work, check_work = guarded_output((int(fir_hip.lib().fir_restore_work_bytes()),), torch.uint8, device=DEV)
    restore = fo.to_u8_clip if policy == CLIP else fo.to_u8_normalized
    scale = iter((1.0, 3.0))  # the second input has another range: a stale minimum or maximum shows
    _twice(rng, lambda r: r.uniform(-80.0, 340.0, shape) * next(scale),
           lambda a: torch_ops.restore_u8_dev(a, policy, out=out, work=work), restore, ("restore", policy))
    check("out")
    check_work("work")


@pytest.mark.parametrize("dtype", [np.uint8, np.int32], ids=["u8", "i32"])
def test_out_and_work_reuse_metrics(dtype):
    """work of exactly fir_metrics_work_bytes(n), out and work inside guard bands."""
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    shape = (3, 264)
    n = 3 * 264
    out, check = guarded_output((9,), torch.float64, device=DEV)
    work, check_work = guarded_output((int(fir_hip.lib().fir_metrics_work_bytes(n)),), torch.uint8, device=DEV)
    for rep in range(2):
        yi = rng.uniform(-64.0, 320.0, shape) * (1 + rep)
        yf = np.rint(yi) + rng.integers(-3, 4, shape)
        yf = (np.clip(yf, 0, 255) if dtype == np.uint8 else yf).astype(dtype)
        torch_ops.compare_metrics_dev(torch.from_numpy(yi).to(DEV), torch.from_numpy(yf).to(DEV), out=out, work=work)
        torch.cuda.synchronize()
    got = fir_hip.metrics_from_sums(out.cpu().numpy(), n)
    want = fo.compute_metrics(yi.reshape(-1), yf.reshape(-1))
    bad = same_metrics(got, want)
    assert not bad, {k: (got[k], want[k]) for k in bad}
    check("out")
    check_work("work")
