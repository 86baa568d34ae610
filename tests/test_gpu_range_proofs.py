"""GPU: every host-side range proof at its threshold, on worst-case inputs, bit for bit.

The cases are the table of tests/range_cases.py (checked on the CPU by tests/test_range_cases.py):
per predicate the last configuration the proof accepts, the first it rejects and, for a
conservative proof, the first at which the narrow form would be wrong.  The inputs are the rows /
frames that attain the exact extremes of the sums, at every phase, plus all-0, all-255 and random
ones.  One test per source row; every output is compared with the C oracle.  A failure names the
case, the side of the threshold, and the first differing output with its exact sum.  The 128-bit
threshold alone is compared with the reference's arithmetic on Python ints: the C oracle sums in 64
bits, which is the very form under test; on the accepted side, where both are exact, the two agree.

entry                              shapes
fir1d_fixed_rows (register)        rows x 4096, rows x 1283
fir1d_fixed_rows_multi (banks)     rows x 4096, rows x 1283; one ImagesMultiPlan batch per bank
fir1d_fixed_rows (matrix cores)    rows x 2048, rows x 1000, and single ragged rows of 2051 (LDS kernel)
fir2d_fixed                        64 x 1040 and 29 x 64, frame by frame; two frames at once for one
                                   case per kernel family
fir1d_fixed_segment_dev            1024 outputs under 2^17 taps (the 128-bit threshold)
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import fir_hip
import range_cases as rc
from fir_hip import torch_ops
from oracle import c_oracle, fir_oracle as fo

DEV = torch.device("cuda:0")
CASES = {c.id: c for c in rc.CASES}
SEAMS = {s["id"]: s for s in rc.SEAMS}
STAGE_NAME = {rc.U8: "u8", rc.I32: "i32"}


def _ids(row):
    return [c.id for c in rc.CASES if c.row == row]


@functools.lru_cache(maxsize=8)
def _inputs(cid, side_name, shape):
    c = CASES[cid]
    x, names = c.inputs(dict(c.sides())[side_name], shape)
    x.setflags(write=False)
    return x, names


def _same(got, want, tag, x, names, taps, frame: bool):
    """Bit-exact, or an AssertionError naming the first differing output and its exact sum."""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    at = tuple(int(v) for v in bad[0])
    r = at[0]
    if frame:
        S = int(rc.mac2d(x[r], taps)[at[1], at[2]])
    else:
        S = int(fo._mac_rows(np.asarray(x[r:r + 1], np.int64), taps)[0, at[1]])
    raise AssertionError(f"{tag}: {len(bad)} of {want.size} outputs differ from the oracle; the first at {at} "
                         f"(input '{names[r]}'): got {got[at]}, want {want[at]}, exact sum {S}; sum(h > 0) = {rc.psum(taps)}, "
                         f"sum(h < 0) = {rc.nsum(taps)}")


def _form(c, name, log, tag, route=None, beside=()):
    """The call's launch log against the case's form (range_cases.Case.form): on the accept side
    every launch has the narrow form; on the reject and conservative sides at least one launch has
    not (a bank split per filter keeps it for the filters that do not cross); a run-time proof
    (Case.runtime) launches it on both sides.  route: the shape is in the list because it takes
    another kernel, named here: every launch is that kernel, on both sides.  beside: kernels that
    part of the call is known to take whatever the side, left out of the form's account."""
    insts = [l.inst for l in log]
    assert log, (tag, "nothing launched")
    log = [l for l in log if l.kernel not in beside]
    assert log, (tag, "every launch took", beside, insts)
    if route is not None:
        assert all(l.kernel in route for l in log), (tag, "route", route, insts)
    elif name == "accept" or c.runtime:
        assert all(c.form(l) for l in log), (tag, "the narrow form was not launched", insts)
    else:
        assert not all(c.form(l) for l in log), (tag, "the narrow form was launched past its proof", insts)


def _run_rows(c, name, side, shapes, single=()):
    """One filter through fir1d_fixed_rows; ``single``: widths of rows that also go alone (one row per call)."""
    co = c_oracle()
    for stage in c.stages:
        for w in shapes:
            x, names = _inputs(c.id, name, w)
            with fir_hip.launch_log() as log:
                got = fir_hip.fir1d_fixed_rows(x, side.taps, side.frac, side.acc, stage)
            # int16 -> int32 below 40 taps never reaches the matrix cores (fir1d.hip, kMfmaMinTapsI32):
            # at that stage these cases run the LDS kernel on both sides and show the proof at the u8
            # stage alone
            lds = c.row == "launch_mfma_t" and c.dtype == np.int16 and stage == rc.I32 and side.taps.size < 40
            _form(c, name, log, f"{c.id} [{name} side] stage {STAGE_NAME[stage]} rows x {w}",
                  route=("fir1d_lds_kernel",) if lds else None)
            want = co.fir1d_rows(x, side.taps, side.frac, side.acc, stage)
            _same(got, want, f"{c.id} [{name} side] stage {STAGE_NAME[stage]} rows x {w}", x, names, side.taps, False)
        for w in single:
            x, names = _inputs(c.id, name, w)
            for r in (0, 1):  # the phase-0 high and low rows
                with fir_hip.launch_log() as log:
                    got = fir_hip.fir1d_fixed_rows(x[r], side.taps, side.frac, side.acc, stage)
                # one row of no whole number of 8 samples: the matrix cores refuse it on both sides
                # (mfma_path_ok), the LDS kernel takes up to 64 taps, the generic kernel the rest
                _form(c, name, log, f"{c.id} [{name} side] one row of {w}",
                      route=("fir1d_lds_kernel",) if side.taps.size <= 64 else ("fir1d_generic_kernel",))
                want = co.fir1d_rows(x[r], side.taps, side.frac, side.acc, stage)
                _same(got[None], want[None], f"{c.id} [{name} side] stage {STAGE_NAME[stage]} one row of {w}", x[r:r + 1],
                      names[r:r + 1], side.taps, False)


def _run_bank(c, name, side, shapes):
    co = c_oracle()
    for stage in c.stages:
        for w in shapes:
            x, names = _inputs(c.id, name, w)
            with fir_hip.launch_log() as log:
                got = fir_hip.fir1d_fixed_rows_multi(x, side.taps, side.frac, side.acc, stage)
            # int32 planes of no whole number of 16 bytes (rows x 1283): the bank goes out filter by
            # filter (launch_fir1d_rows_multi), and a filter whose plane starts off 16 bytes takes the
            # generic kernel on both sides; the form is held on the filters the register kernel keeps
            tag = f"{c.id} [{name} side] stage {STAGE_NAME[stage]} bank rows x {w}"
            if stage == rc.I32 and x.size * 4 % 16 != 0:
                # one launch per filter, in order; the proof shows in the launch of the filter that
                # crosses (c.f), unless its plane starts off 16 bytes: then that filter runs the
                # generic kernel on both sides and this shape shows the proof at the u8 stage alone
                assert len(log) == len(side.taps), (tag, [l.inst for l in log])
                if c.f * x.size * 4 % 16 != 0:
                    _form(c, name, log[c.f:c.f + 1], tag, route=("fir1d_generic_kernel",))
                else:
                    _form(c, name, log[c.f:c.f + 1], tag)
            else:
                _form(c, name, log, tag)
            for f, h in enumerate(side.taps):
                want = co.fir1d_rows(x, h, side.frac, side.acc, stage)
                _same(got[f], want, f"{c.id} [{name} side] stage {STAGE_NAME[stage]} filter {f} rows x {w}", x, names, h, False)


def _run_frames(c, name, side, monkeypatch, path, stages, frames2, cid):
    co = c_oracle()
    if path is None:
        monkeypatch.delenv("FIR2D_PATH", raising=False)
    else:
        monkeypatch.setenv("FIR2D_PATH", path)
    for stage in stages:
        for shape in ((64, 1040), (29, 64)):
            x, names = _inputs(cid, name, shape) if cid in CASES else rc.worst_frames_u8(side.taps, *shape)
            with fir_hip.launch_log() as log:
                got = np.stack([fir_hip.fir2d_fixed(f, side.taps, side.frac, side.acc, stage) for f in x])
            if c is not None:
                _form(c, name, log, f"{cid} [{name} side] FIR2D_PATH={path} stage {STAGE_NAME[stage]} frames of {shape}")
            want = np.stack([co.fir2d(f, side.taps, side.frac, side.acc, stage) for f in x])
            tag = f"{cid} [{name} side] FIR2D_PATH={path} stage {STAGE_NAME[stage]} frames of {shape}"
            _same(got, want, tag, x, names, side.taps, True)
            if frames2:
                got2 = fir_hip.fir2d_fixed(x[:2], side.taps, side.frac, side.acc, stage)
                _same(got2, want[:2], tag + " (two at once)", x, names, side.taps, True)


# ---- one test per source row ---------------------------------------------------------------
@pytest.mark.parametrize("cid", _ids("launch_reg"))
def test_launch_reg(cid):
    """fir1d_reg_impl.h launch_reg: nowrap (acc 24 and 16, one filter and banks of 2 and 4 in which
    one filter crosses) and taps16 (32767 / 32768, -32768 / -32769)."""
    c = CASES[cid]
    for name, side in c.sides():
        (_run_bank if c.kind == "bank" else _run_rows)(c, name, side, (4096, 1283))


@pytest.mark.parametrize("cid", _ids("plan_u8_noclamp"))
def test_plan_u8_noclamp(cid):
    """fir1d_reg.h plan_u8_noclamp: the u8 stage as a shift alone, vmax at frac 8, 12, 15 and vmin;
    the filter alone and as filter 1 of a bank beside a packed-16 filter (the bank kernel's v_dot2 form)."""
    c = CASES[cid]
    co = c_oracle()
    for name, side in c.sides():
        _run_rows(c, name, side, (4096, 1283))
        L = side.taps.size
        bank = np.stack([np.r_[np.zeros(L - 1, np.int64), 1 << (side.frac - 2)], side.taps])  # filter 0: a quarter, s = f - 2
        for w in (4096, 1283):
            x, names = _inputs(c.id, name, w)
            got = fir_hip.fir1d_fixed_rows_multi(x, bank, side.frac, side.acc, rc.U8)
            for f in (0, 1):
                _same(got[f], co.fir1d_rows(x, bank[f], side.frac, side.acc, rc.U8),
                      f"{c.id} [{name} side] in a bank, filter {f}, rows x {w}", x, names, bank[f], False)


@pytest.mark.parametrize("cid", _ids("plan_u8_pk16"))
def test_plan_u8_pk16(cid):
    """fir1d_reg.h plan_u8_pk16: the four ends of the 16-bit ranges at s = 0 and s = 3, f - s = 15 / 16,
    and the high-byte form beside a signed filter and a filter at shift 7."""
    c = CASES[cid]
    for name, side in c.sides():
        _run_bank(c, name, side, (4096, 1283))


@pytest.mark.parametrize("cid", [c.id for c in rc.CASES if c.kind == "bank"])
def test_images_multi_plan_threshold_bank(cid):
    """The same threshold banks through one torch_ops.ImagesMultiPlan batch (the batch kernel): an
    image of whole vectors, a ragged one and a single row."""
    c = CASES[cid]
    co = c_oracle()
    for name, side in c.sides():
        x4, n4 = _inputs(c.id, name, 4096)
        x1, n1 = _inputs(c.id, name, 1283)
        imgs = [(np.array(x4), n4), (np.array(x1), n1), (np.array(x1[:1, :1031]), n1[:1])]
        plan = torch_ops.ImagesMultiPlan([torch.from_numpy(a).to(DEV) for a, _ in imgs], side.taps, side.frac, side.acc, rc.U8)
        with fir_hip.launch_log() as log:
            outs = plan.launch()
        torch.cuda.synchronize()
        assert [l.kernel for l in log] == ["fir1d_reg_batch_kernel"], [l.inst for l in log]
        _form(c, name, log, f"{c.id} [{name} side] one batch")
        for i, (a, names) in enumerate(imgs):
            for f, h in enumerate(side.taps):
                _same(outs[i][f].cpu().numpy(), co.fir1d_rows(a, h, side.frac, side.acc, rc.U8),
                      f"{c.id} [{name} side] image {i} filter {f}", a, names, h, False)


@pytest.mark.parametrize("cid", _ids("launch_mfma_t"))
def test_launch_mfma_t(cid):
    """fir1d_mfma.hip launch_mfma_t / mfma_path_ok: `fast` for u8 (acc 24) and int16 (acc 32, the sum
    exactly -2^31 and 2^31 - 1 on the rejected side) on the step, run and long kernels, and the
    32639 / 32640 tap (the LDS kernel takes 32640, and every ragged single row)."""
    c = CASES[cid]
    for name, side in c.sides():
        _run_rows(c, name, side, (2048, 1000), single=(2051,))


@pytest.mark.parametrize("cid", _ids("launch2d_reg"))
def test_launch2d_reg(cid, monkeypatch):
    """fir2d.hip launch2d_reg: nowrap at acc 24 and 20 (general and rank-1 kernels), int16 row sums
    (sum|row| = 128 / 129), 24-bit row sums (32896 / 32897) and the int16 column factor (32767 / 32768)."""
    c = CASES[cid]
    for name, side in c.sides():
        _run_frames(c, name, side, monkeypatch, c.path, c.stages, c.frames2, c.id)


@pytest.mark.parametrize("cid", _ids("plan_pk16"))
def test_plan_pk16(cid, monkeypatch):
    """fir2d_reg.h plan_pk16 / plan_pk16_gen (FIR2D_PATH=reg): the ends of the 16-bit ranges for
    general and rank-1 kernels (all four ends each), 3x3 and 5x5, the shift taken from the column factor, the high-byte form."""
    c = CASES[cid]
    for name, side in c.sides():
        _run_frames(c, name, side, monkeypatch, c.path, c.stages, c.frames2, c.id)


@pytest.mark.parametrize("cid", _ids("plan_mfma2"))
def test_plan_mfma2(cid, monkeypatch):
    """fir2d_mfma.hip plan_mfma2: one byte plane or two (127 / 128, -128 / -129), the 32639 / 32640 tap
    (refused: the register path runs), `fast` at frac 12 (sum|h| = 526335 / 526336) and acc 24; by
    default dispatch and with FIR2D_PATH=mfma."""
    c = CASES[cid]
    for name, side in c.sides():
        _run_frames(c, name, side, monkeypatch, c.path, c.stages, c.frames2, c.id)


@pytest.mark.parametrize("sid", list(SEAMS))
def test_dispatch_seams(sid, monkeypatch):
    """The limits on frac_bits and the clamp of the common shift at frac - 1: both sides compute the
    same values in either form (range_cases.SEAMS says why), and both must equal the oracle."""
    s = SEAMS[sid]
    co = c_oracle()
    import types
    form = types.SimpleNamespace(form=s["form"], runtime=False)
    for i, side in enumerate(s["sides"]):
        name = f"side {i}, frac {side.frac}"
        held = "accept" if s["launched"][i] else "reject"  # whether this side's launches show the form
        if s["kind"] == "frame":
            _run_frames(form, held, side, monkeypatch, s["path"], s["stages"], False, sid)
            continue
        for w in (4096, 1283) if s["row"] != "launch_mfma_t" else (2048, 1000):
            h0 = side.taps[0] if s["kind"] == "bank" else side.taps
            x, names = rc.worst_rows_u8(h0, w)
            for stage in s["stages"]:
                with fir_hip.launch_log() as log:
                    if s["kind"] == "bank":
                        got = fir_hip.fir1d_fixed_rows_multi(x, side.taps, side.frac, side.acc, stage)
                    else:
                        got = fir_hip.fir1d_fixed_rows(x, side.taps, side.frac, side.acc, stage)[None]
                _form(form, held, log, f"{sid} [{name}] stage {STAGE_NAME[stage]} rows x {w}")
                for f, h in enumerate(np.atleast_2d(side.taps)):
                    _same(got[f], co.fir1d_rows(x, h, side.frac, side.acc, stage),
                          f"{sid} [{name}] stage {STAGE_NAME[stage]} filter {f} rows x {w}", x, names, h, False)


# ---- the 128-bit threshold -------------------------------------------------------------------
def _exact_sums(full, h) -> list:
    """The exact sums of a shard with its halos as Python ints: the taps split into 16-bit halves, so that
    each half's sums are exact in int64."""
    hrev = np.asarray(h, np.int64)[::-1]
    f64 = np.asarray(full, np.int64)
    sl = np.correlate(f64, hrev & np.int64(0xFFFF), "valid")
    sh = np.correlate(f64, hrev >> np.int64(16), "valid")
    return [(int(b) << 16) + int(a) for a, b in zip(sl, sh)]


def _exact_stage(S: int, frac: int, acc: int, stage: int) -> int:
    """The reference's arithmetic on Python ints, fir_1d_fixed_ref.py:110-126: mask to acc_bits, restore the
    sign, add the half, shift, saturate (or keep the low 32 bits)."""
    S &= (1 << acc) - 1
    if S & (1 << (acc - 1)):
        S -= 1 << acc
    v = (S + (1 << (frac - 1))) >> frac
    return min(max(v, 0), 255) if stage == rc.U8 else ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def test_needs_wide_threshold():
    """fir1d.hip needs_wide, int16 samples, acc_bits >= 64: 2^17 taps with sum|h| = 2^48 - 1 / 2^48 over one
    shard of 1024 outputs and its halos, x = -32768 but for a few samples in the first 512 and the last 508:
    outputs 512..515 see none of them and sum to 2^63 - 32768 / exactly 2^63, the others to a little less.  At acc_bits = 64 the reference wraps 2^63
    to -2^63 itself, so a 64-bit sum would do (the proof is conservative there); from acc_bits = 65 the sum
    stays 2^63 and only the 128-bit sum gives it.  (The u8 threshold needs about 1.7e7 taps and as many
    samples: not covered.)"""
    co = c_oracle()
    rng = np.random.default_rng(63)
    n = 1024
    for name, h in zip(("accept", "reject"), rc.wide_case()):
        L = h.size
        hl_n, hr_n = fo.halo_sizes(L)
        full = np.full(hl_n + n + hr_n, -32768, np.int16)
        full[rng.integers(0, 512, 40)] = rng.integers(-32768, 32768, 40)
        full[full.size - 1 - rng.integers(0, 508, 40)] = rng.integers(-32768, 32768, 40)
        parts = [torch.from_numpy(np.ascontiguousarray(p)).to(DEV)
                 for p in (full[hl_n:hl_n + n], full[:hl_n], full[hl_n + n:])]
        sums = _exact_sums(full, h)
        assert len(sums) == n and sums[512:516] == [(1 << 63) if name == "reject" else (1 << 63) - 32768] * 4
        # 2^63 >> 12 is 0 mod 2^32 whatever its sign: frac 40 for the int32 stage
        for frac, acc, stage in ((12, 64, rc.U8), (12, 65, rc.U8), (40, 65, rc.I32), (40, 100, rc.I32)):
            want = [_exact_stage(S, frac, acc, stage) for S in sums]
            if name == "reject":
                assert want[512] == {(64, rc.U8): 0, (65, rc.U8): 255}.get((acc, stage), 1 << 23)
            y = torch_ops.fir1d_fixed_segment_dev(parts[0], h, parts[1], parts[2], frac, acc, stage).cpu().numpy()
            got = [int(v) for v in y]
            bad = [i for i in range(n) if got[i] != want[i]]
            assert not bad, (f"needs_wide [{name} side] acc {acc} stage {STAGE_NAME[stage]}: {len(bad)} outputs differ; the "
                             f"first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}, exact sum {sums[bad[0]]} "
                             f"(2^63 = {1 << 63})")
            if name == "accept":  # |sum| < 2^63: the C oracle's 64-bit sums are exact there too
                ref = co.fir1d_rows(full[hl_n:hl_n + n], h, frac, acc, stage, halo_left=full[:hl_n], halo_right=full[hl_n + n:])
                assert [int(v) for v in ref] == want
