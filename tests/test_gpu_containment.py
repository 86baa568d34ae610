"""GPU: every device entry and dispatch branch inside guard bands (tests/guarded.py).

The rest of the GPU suite goes through the host entries, which stage every call in 16-byte
aligned, ever-growing, recycled scratch buffers: a kernel that stores a vector past its output,
whose zero padding takes in a byte beside its input, or that only works on aligned pointers
passes there.  Here every case calls a ``fir_hip.torch_ops`` device entry with

* the input (and every halo and image) a ``guarded_input``: hostile samples on both sides,
* the output (and every plane and work buffer) a ``guarded_output``: canary-filled, >= 64 KiB of
  canaries on both sides (two frame rows more for 2-D shapes),

and asserts (a) the output equals the C oracle on the bare arrays, (b) every canary is intact,
and so (c), by (a), that every output element was written.  Data is full-range random; u8 data
also holds runs of 0 and 255.  ``(x_lead, y_lead)`` are the byte offsets of the views past a
512-byte boundary, i.e. what the dispatchers' ``x % 16``, ``x % 8`` and ``y % 16`` tests see.

Group -> kernel it reaches <- the dispatch condition that sends it there.  Every row is asserted:
each call runs under ``fir_hip.launch_log()`` and the log of that same call -- the kernel, its
template arguments, its flags spelled in words -- is held against the row before the output is
compared with the oracle, so a case that drifts off its kernel fails here instead of passing on the
bit-exact fall-back.
(launch_fir1d_rows, reg_path_ok: fir1d.hip; mfma_path_ok, launch_mfma_t: fir1d_mfma.hip;
lds_path_ok: fir1d_lds.hip; launch_fir2d: fir2d.hip; launch_fir2d_mfma: fir2d_mfma.hip):

=========================  ====================================  =====================================================
test                       kernel                                deciding condition
=========================  ====================================  =====================================================
test_register_kernel       fir1d_reg_kernel: u8 byte-pair dot2   reg_path_ok: L <= 9, ch 1 (or 2 with int16), acc <= 32,
                           (Q4.12, |h| <= 8), int16 dot2          frac <= 31, |h| < 2^23, x % 16 == 0, y % 16 == 0, one
                           (int16 taps), mad24 (a 2^23-1 tap,     row or rowlen >= vec + (L-1) ch.  launch_reg: taps16 and
                           or channels=2); kRagged / kMasked      no u8 sum can wrap -> kU8Dot2; int16, ch 1, taps16 ->
                           forms for rows of a ragged width       kDot2; else mad24.  rowlen % vec != 0 -> kRagged/kMasked
test_register_misaligned   fir1d_generic_kernel                  x % 16 != 0 or y % 16 != 0 fails reg_path_ok; L < 10 is
                                                                 below kMfmaMinTaps; lds_path_ok wants x % 8|16, y % 16
test_lds_kernel            fir1d_lds kernel (v_dot2 over LDS)    int16 -> int32 with L < kMfmaMinTapsI32 = 40; or a tap
                                                                 above 32639 (mfma_path_ok taps_ok) but <= 32767; or one
                                                                 ragged row (total % 8 != 0 fails mfma_path_ok, rows == 1
                                                                 passes lds_path_ok); u8 input at x % 16 == 8 (x % 8 == 0)
test_mfma_step_kernel      fir1d_mfma_step_kernel<KS = 2 | 3,    10 <= L <= 65 (int16 -> int32: 40 <= L), mfma_path_ok:
                           ACC32, FAST>: <true, true> FAST,      ch 1, taps in [-32768, 32639], acc <= 32, frac <= 31,
                           <true, false> acc 32 that may wrap,   rowlen % 8 == 0, x % 8 (u8) / 16 (int16), y % 16;
                           <false, false> acc 24 and acc 20      launch_mfma_t: KS = ceil((32 + L/2 + roundup8(L-1-L/2))
                                                                 / 32) <= 3; FAST = frac <= 22 and sum|h| xmax + 2^(f-1)
                                                                 < 2^(acc-1).  u8 samples reach <true, false> only with
                                                                 frac > 22 (65 taps of 32768 times 255 stay below 2^31)
test_mfma_step_y_lead      fir1d_generic_kernel                  y % 16 == 4 fails mfma_path_ok and lds_path_ok
test_mfma_run_kernel       fir1d_mfma_run_kernel<STAGE, NS,      launch_mfma_t: KS > 3 and u8 samples; launch_mfma_run:
                           MULTI, TPS> (u8, L >= 66): RUN_FORMS  k-steps of the halo rounded to 16.  L = 66: one chunk of
                                                                 4; 257: one chunk of 9; 258: one chunk of 10 (the case
                                                                 this row had meant by 257); 450: one chunk of 16, all
                                                                 one tile per run; 1000, 2048 (33, 65 k-steps): several
                                                                 chunks (u8 out: chunks of 6, 4-tile runs; int32 out:
                                                                 chunks of 12 / 14, 2-tile runs); x % 16 == 0 and == 8
test_mfma_long_kernel      fir1d_mfma_long_kernel<int16, STAGE,  launch_mfma_t: KS > 3 and int16 samples; launch_mfma_long
                           ACC32, FAST>, chunks of kMlChunk =     picks the form as above.  L = 66 / 481 / 483 / 993 / 995
                           16 k-steps; all six instantiations:    / 4099 -> 4 / 16 / 17 / 32 / 33 / 130 k-steps.
                           stage U8_SAT x form "fast"             <int16, U8_SAT, true, true>:  stage u8,  form fast
                                                "acc32"           <int16, U8_SAT, true, false>: stage u8,  form acc32
                                                "acc24"           <int16, U8_SAT, false, false>: stage u8, form acc24
                           stage I32 x form "fast"                <int16, I32, true, true>:     stage i32, form fast
                                            "acc32"               <int16, I32, true, false>:    stage i32, form acc32
                                            "acc24"               <int16, I32, false, false>:   stage i32, form acc24
test_generic_kernel        fir1d_generic_kernel                  each fast path refuses: channels = 3; acc 40; frac 33; a
                                                                 2^31-1 tap; L = 31 with rowlen % 8 != 0; misaligned leads
test_segment_and_edges     fir1d_reg_kernel kHalo (one launch)   launch_fir1d_segment: total % reg_tile_samples == 0 and
                           | rows dispatch + fir1d_edges_kernel  reg_path_ok -> one launch; else launch_fir1d_rows then
                           | fir1d_generic_kernel with halos     launch_fir1d_edges; total <= halo samples -> generic
test_rows_multi            fir1d_reg_kernel F = 1..4 (fused u8   launch_fir1d_rows_multi: u8, ch 1, reg_path_ok(x, x)
                           bank, planes at any byte for u8 out;  and (u8 out or plane bytes % 16 == 0), else per filter;
                           kU8Dot2 for bank "q412big", kU8Pk16   launch_reg: F > 1, u8 out and plan_u8_pk16 -> kU8Pk16
                           for bank "pk16" and for "q412"'s      (one filter of the group that fits is enough: "q412"'s
                           group with filter 0)                  filter 0 of small taps)
test_images_multi          fir1d_reg_batch_kernel (kRagged,      launch_fir1d_images_multi: u8 -> u8, ch 1 and
                           kDefer) | per-image dispatch          reg_path_ok(xs[i], xs[i]); an image at x % 16 == 1 and
                                                                 one narrower than 16 + (L-1) take launch_fir1d_rows
test_fir2d_*               fir2d_reg_kernel separable / packed-  launch_fir2d: FIR2D_PATH != reg and (forced or not rank
                           16 general / dot2 general; fir2d_      1) -> launch_fir2d_mfma (u8 out, W % 16 == 0, x, y % 16,
                           mfma_kernel NP = 1 | 2;                R in {3, 5}; NP = 1 when taps >> s fit a byte, else 2);
                           fir2d_generic_kernel                   else `fast` (reg2d_shape, W % 16, x, y % 16) -> register
                                                                 kernels; else generic (7x7, W = 17, a 1-byte lead)
test_ideal_rows            fir1d_ideal_reg_kernel | fir1d_ideal  launch_fir1d_ideal: L <= 9, x % (4 kIdealNV), y % 16 and
                           _kernel                                rows wide enough -> register form, else the LDS form
test_restore_u8            restore kernels, both policies        (a % 16 and out % 16 are required: lead 0 and 16 only)
test_compare_metrics       metrics kernels, vector and scalar    launch_metrics: vec = ideal % 16 == 0 and fixed % 16 == 0
=========================  ====================================  =====================================================
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
from conftest import same_metrics
from fir_hip import torch_ops
from guarded import guarded_input, guarded_output
from oracle import c_oracle, fir_oracle as fo

DEV = torch.device("cuda:0")
U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
STAGES = (U8, I32)
_TDT = {U8: torch.uint8, I32: torch.int32}


# ---- data ------------------------------------------------------------------------------
def _samples(rng, shape, dtype, pin_third: bool = False) -> np.ndarray:
    """Full-range random samples; u8 with runs of 0 and 255; pin_third: the middle third of every
    row held at -32768 (a sum of large taps over it wraps a 32-bit accumulator for certain)."""
    if dtype == np.uint8:
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        flat = x.reshape(-1)
        n = flat.size
        run = max(1, min(n // 9, 70))
        for k, v in enumerate((0, 255, 255, 0)):
            s = n * (2 * k + 1) // 9
            flat[s:s + run] = v
        return x
    x = rng.integers(-32768, 32768, shape, dtype=np.int16)
    if pin_third:
        w = x.shape[-1]
        x.reshape(-1, w)[:, w // 3:w // 3 + (w + 2) // 3] = -32768
    return x


def _hann(L: int, kind: str = "smooth") -> np.ndarray:
    """Unity-gain Q4.12 low-pass taps: a Hann window, or a Hann-windowed sinc (cutoff 0.1)."""
    w = np.hanning(L + 2)[1:-1]
    h = w if kind == "smooth" else 0.2 * np.sinc(0.2 * (np.arange(L) - (L - 1) / 2)) * w
    return np.rint(h / h.sum() * 4096).astype(np.int64)


def _wrap_taps(rng, L: int) -> np.ndarray:
    """Taps at the matrix-core byte-split limits, at least three of them of full size."""
    h = rng.choice(np.array([-32768, 32639, 1, -1, 127, 128, -129]), L)
    h[0], h[L // 2], h[-1] = -32768, -32768, 32639
    return h


def _big_taps(rng, L: int) -> np.ndarray:
    """Random taps with sum|h| >= 60000: even u8 sums pass 2^23 (an accumulator of 24 bits wraps)."""
    h = rng.integers(-30000, 30001, L)
    h[0], h[-1] = 30000, -30000
    return h


def _ks(L: int) -> int:
    """k-steps of launch_mfma_t."""
    c = L // 2
    return (32 + c + ((L - 1 - c + 7) & ~7) + 31) // 32


def _form(hq, dtype, frac: int, acc: int) -> str:
    """The arithmetic form launch_mfma_t picks."""
    xmax = 255 if dtype == np.uint8 else 32768
    habs = int(np.abs(np.asarray(hq, dtype=np.int64)).sum())
    if frac <= 22 and habs * xmax + (1 << (frac - 1)) < (1 << (acc - 1)):
        return "fast"
    return "acc32" if acc == 32 else "acclt32"


def _same(y: torch.Tensor, want: np.ndarray, tag) -> None:
    got = y.cpu().numpy()
    if got.dtype == np.float64:
        got, want = got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{tag}: {bad.size} of {want.size} outputs differ from the oracle; the first at flat "
                             f"index {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}")


# ---- what a call launched (fir_hip.launch_log) ---------------------------------------------
_CT = {np.uint8: "unsigned char", np.int16: "short", "uint8": "unsigned char", "int16": "short"}
# the register kernels' flags that name a form (the rest are the fixed store / load policy)
_FORM_FLAGS = frozenset({"kDot2", "kU8Dot2", "kAcc32", "kRagged", "kMasked", "kHalo", "kU8Pk16", "kU8PkHi8", "kDefer"})
_BOOL = {True: "true", False: "false"}
_MFMA_FORM = {"fast": ("true", "true"), "acc32": ("true", "false"), "acclt32": ("false", "false")}  # <ACC32, FAST>


def _one(log, kernel: str, tag):
    """The call made exactly one launch, of `kernel`."""
    assert [l.kernel for l in log] == [kernel], (tag, [l.inst for l in log])
    return log[0]


def _reg_form(dtype, ch: int, stage: int, hq, frac: int, acc: int, shape, halo: bool = False) -> set:
    """The form flags launch_reg / launch_reg_flags give ONE filter (fir1d_reg_impl.h), in words."""
    h = np.asarray(hq, dtype=np.int64)
    u8 = np.dtype(dtype) == np.uint8
    taps16 = bool((h >= -32768).all() and (h <= 32767).all())
    form = set()
    if u8 and ch == 1 and taps16 and frac <= 22 and 255 * int(np.abs(h).sum()) + (1 << (frac - 1)) < (1 << (acc - 1)):
        form.add("kU8Dot2")  # byte-pair v_dot2: no sum can wrap
    elif not u8 and ch == 1 and taps16:
        form.add("kDot2")
    if "kU8Dot2" not in form and acc == 32:
        form.add("kAcc32")
    vec = 16 if u8 else 8
    if len(shape) == 2 and shape[0] > 1 and shape[1] % vec:  # rows straddle vectors
        form.add("kRagged" if stage == U8 and ch == 1 else "kMasked")
    elif not u8:
        form.add("kMasked")  # one int16 filter keeps the masked pair compiled in (its code layout)
    if halo:
        form.add("kHalo")
    return form


def _is_reg(l, dtype, stage: int, L: int, ch: int, form: set, tag, F: int = 1) -> None:
    assert l.kernel == "fir1d_reg_kernel", (tag, l.inst)
    assert (l.targs[0], l.targs[1], l.targs[2], l.targs[3], l.targs[6]) == (_CT[np.dtype(dtype).name], str(stage), str(L),
                                                                           str(ch), str(F)), (tag, l.inst)
    assert l.flags & _FORM_FLAGS == form, (tag, sorted(l.flags & _FORM_FLAGS), sorted(form))


def _rows(x: np.ndarray, hq, frac=12, acc=32, stage=I32, ch=1, x_lead=0, y_lead=0, tag=(), want=None) -> None:
    """fir1d_fixed_rows_dev on a guarded input into a guarded output: want(log, tag) on the call's
    launch log (a kernel name: exactly one launch of it), then (a) oracle, (b) canaries."""
    tag = (x.dtype.name, x.shape, len(hq), frac, acc, stage, ch, x_lead, y_lead) + tuple(tag)
    xg = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    y, check = guarded_output(x.shape, _TDT[stage], lead_bytes=y_lead, device=DEV)
    assert xg.data_ptr() % 16 == x_lead % 16 and y.data_ptr() % 16 == y_lead % 16
    with fir_hip.launch_log() as log:
        torch_ops.fir1d_fixed_rows_dev(xg, hq, frac, acc, stage, ch, out=y)
    torch.cuda.synchronize()
    assert want is not None, "every case names the kernel it reaches"
    if isinstance(want, str):
        _one(log, want, tag)
    else:
        want(log, tag)
    _same(y, c_oracle().fir1d_rows(x, hq, frac, acc, stage, channels=ch), tag)
    check(str(tag))
    assert torch.equal(xg.cpu(), torch.from_numpy(x)), tag  # the input is only read


# ---- fir1d_fixed_rows_dev: the register kernel ------------------------------------------
REG_INPUTS = [("u8", np.uint8, 1), ("i16", np.int16, 1), ("i16c2", np.int16, 2)]
REG_SINGLE = [1, 15, 16, 17, 4095, 4096, 4097, 8 * 4096 + 3]
REG_ROWS = [(3, 1001), (5, 1000), (2, 4096), "exact"]


def _reg_taps(rng, L: int) -> dict:
    big = rng.integers(-8192, 8193, L)
    big[L // 2] = (1 << 23) - 1
    return {"q412": rng.integers(-8192, 8193, L), "small": rng.integers(-8, 9, L), "mad24": big}


@pytest.mark.parametrize("shape", REG_SINGLE + REG_ROWS, ids=str)
@pytest.mark.parametrize("name,dtype,ch", REG_INPUTS, ids=[r[0] for r in REG_INPUTS])
def test_register_kernel(name, dtype, ch, shape):
    rng = np.random.default_rng(REG_INPUTS.index((name, dtype, ch)) * 100 + (REG_SINGLE + REG_ROWS).index(shape))
    for L in (2, 3, 5, 9):
        vec = 16 if dtype == np.uint8 else 8
        if shape == "exact":  # rows of exactly vec + (L-1) ch samples: the narrowest reg_path_ok admits
            shp = (3, vec + (L - 1) * ch)
        elif isinstance(shape, tuple):
            shp = (shape[0], shape[1] * ch)
        else:
            shp = (shape * ch,)
        x = _samples(rng, shp, dtype)

        def reg(hq, frac, acc, stage):
            form = _reg_form(dtype, ch, stage, hq, frac, acc, shp)
            return lambda log, tag: _is_reg(_one(log, "fir1d_reg_kernel", tag), dtype, stage, L, ch, form, tag)

        for kind, hq in _reg_taps(rng, L).items():
            for stage in STAGES:
                form = _reg_form(dtype, ch, stage, hq, 12, 32, shp)
                # the arithmetic each kind of taps is here for
                assert ("kU8Dot2" in form) == (name == "u8" and kind != "mad24"), (kind, form)
                assert ("kDot2" in form) == (name == "i16" and kind != "mad24"), (kind, form)
                _rows(x, hq, 12, 32, stage, ch, tag=(kind,), want=reg(hq, 12, 32, stage))
        hq = _reg_taps(rng, L)["q412"]
        _rows(x, hq, 16, 24, I32, ch, tag=("acc24",), want=reg(hq, 16, 24, I32))


@pytest.mark.parametrize("name,dtype,ch", REG_INPUTS, ids=[r[0] for r in REG_INPUTS])
def test_register_misaligned(name, dtype, ch):
    """A pointer one sample (x) or one output element (y) off 16 bytes: the generic kernel."""
    rng = np.random.default_rng(7)
    item = np.dtype(dtype).itemsize
    for shp in ((4097 * ch,), (3, 1001 * ch), (5, 1000 * ch)):
        x = _samples(rng, shp, dtype)
        for L in (3, 9):
            hq = rng.integers(-8192, 8193, L)
            for stage in STAGES:
                _rows(x, hq, 12, 32, stage, ch, x_lead=item, want="fir1d_generic_kernel")
                _rows(x, hq, 12, 32, stage, ch, y_lead=4 if stage == I32 else 1, want="fir1d_generic_kernel")


# ---- the LDS v_dot2 kernel --------------------------------------------------------------
LDS_SHAPES = [(1, 2051), (3, 1000), (40, 8), (1, 2048)]


@pytest.mark.parametrize("shape", LDS_SHAPES, ids=str)
def test_lds_kernel(shape):
    rng = np.random.default_rng(shape[0] * 10000 + shape[1])
    xi, xu = _samples(rng, shape, np.int16), _samples(rng, shape, np.uint8)
    for L in (10, 24, 39):  # int16 -> int32 below kMfmaMinTapsI32
        _rows(xi, rng.integers(-32768, 32768, L), 12, 32, I32, want="fir1d_lds_kernel")
        _rows(xi, rng.integers(-3000, 3001, L), 16, 24, I32, want="fir1d_lds_kernel")
    big = rng.integers(-3000, 3001, 17)
    big[5] = 32640  # one past the matrix-core byte split: MFMA refuses, v_dot2 takes it
    for x in (xi, xu):
        for stage in STAGES:
            _rows(x, big, 12, 32, stage, want="fir1d_lds_kernel")
    for stage in STAGES:  # u8 input 8 bytes off a 16-byte boundary (lds_path_ok: x % 8 == 0)
        _rows(xu, big, 12, 32, stage, x_lead=8, want="fir1d_lds_kernel")


# ---- the matrix-core step kernel (2 and 3 k-steps) ------------------------------------------
STEP_SHAPES = [(3, 1032), (2, 2056), (5, 1000), (40, 8), (1, 5128)]
STEP_IO = [("u8_u8", np.uint8, U8), ("u8_i32", np.uint8, I32), ("i16_u8", np.int16, U8), ("i16_i32", np.int16, I32)]


def _step_forms(rng, L: int, dtype) -> list:
    """(expected form, taps, frac, acc)."""
    forms = [("fast", _hann(L), 12, 32), ("acc32", _wrap_taps(rng, L), 12 if dtype == np.int16 else 24, 32),
             ("acclt32", _big_taps(rng, L), 16, 24), ("acclt32", _big_taps(rng, L), 12, 20)]
    if dtype == np.uint8:  # two-plane taps at frac 12: u8 sums cannot wrap 32 bits, so this is FAST
        forms.append(("fast", _wrap_taps(rng, L), 12, 32))
    return forms


# int16 -> int32 below kMfmaMinTapsI32 = 40 taps is the LDS kernel's (test_lds_kernel)
STEP_CASES = [io + lk for io in STEP_IO for lk in ((10, 2), (33, 2), (40, 3), (64, 3), (65, 3))
              if not (io[0] == "i16_i32" and lk[0] < 40)]


@pytest.mark.parametrize("name,dtype,stage,L,ks", STEP_CASES, ids=[f"{c[0]}-{c[3]}" for c in STEP_CASES])
def test_mfma_step_kernel(name, dtype, stage, L, ks):
    assert _ks(L) == ks
    rng = np.random.default_rng(L * 10 + STEP_IO.index((name, dtype, stage)))
    for shape in STEP_SHAPES:
        for form, hq, frac, acc in _step_forms(rng, L, dtype):
            assert _form(hq, dtype, frac, acc) == form
            x = _samples(rng, shape, dtype, pin_third=form == "acc32")

            def step(log, tag, form=form):
                l = _one(log, "fir1d_mfma_step_kernel", tag)
                assert l.targs == (_CT[dtype], str(stage), str(ks)) + _MFMA_FORM[form], (tag, l.inst)

            _rows(x, hq, frac, acc, stage, tag=(form,), want=step)
            if dtype == np.uint8 and shape in ((3, 1032), (1, 5128), (40, 8)):
                _rows(x, hq, frac, acc, stage, x_lead=8, tag=(form,), want=step)


@pytest.mark.parametrize("name,dtype,stage", STEP_IO, ids=[r[0] for r in STEP_IO])
def test_mfma_step_y_lead(name, dtype, stage):
    """y four bytes off 16: mfma_path_ok and lds_path_ok refuse, the generic kernel runs."""
    rng = np.random.default_rng(3)
    for L in (10, 40, 65):
        for shape in ((3, 1032), (1, 5128)):
            _rows(_samples(rng, shape, dtype), _hann(L), 12, 32, stage, y_lead=4, want="fir1d_generic_kernel")


# ---- the matrix-core run kernel (u8, 66 taps and up) ---------------------------------------
# L -> stage -> (k-steps per chunk NS, several chunks, tiles per run): launch_mfma_run with the halo
# rounded to 16 (66 / 257 / 258 / 450 / 1000 / 2048 taps: 4 / 9 / 10 / 16 / 33 / 65 k-steps; past
# kMrU8One = 32 (u8 out) or kMrC = 16 (int32 out) k-steps the chunk with the least zero padding)
RUN_FORMS = {
    66: {U8: (4, False, 1), I32: (4, False, 1)},
    257: {U8: (9, False, 1), I32: (9, False, 1)},
    258: {U8: (10, False, 1), I32: (10, False, 1)},
    450: {U8: (16, False, 1), I32: (16, False, 1)},
    1000: {U8: (6, True, 4), I32: (12, True, 2)},
    2048: {U8: (6, True, 4), I32: (14, True, 2)},
}


def _run_form(L: int, stage: int, form: str, hn=None):
    ns, multi, tps = RUN_FORMS[L][stage]

    def want(log, tag):
        l = _one(log, "fir1d_mfma_run_kernel", tag)
        assert l.targs[:4] == (str(stage), str(ns), _BOOL[multi], str(tps)), (tag, l.inst)
        assert l.note["mode"] == {"fast": "fast", "acc32": "acc32", "acclt32": "acc24"}[form], (tag, l.note)
        if hn is not None:
            assert int(l.targs[4]) in hn, (tag, l.inst)
    return want


@pytest.mark.parametrize("L", list(RUN_FORMS))
def test_mfma_run_kernel(L):
    rng = np.random.default_rng(L)
    for shape in ((3, 3 * 1024 + 24), (16, 1000), (1, 5 * 1024 + 8)):
        x = _samples(rng, shape, np.uint8)
        for frac, acc, amp in ((12, 32, 400), (16, 24, 3000), (12, 32, 32639)):
            hq = rng.integers(-amp, amp + 1, L)
            for stage in STAGES:
                for x_lead in (0, 8):
                    form = _form(hq, np.uint8, frac, acc)
                    # random taps past a byte in every k-step: no high plane is skipped (HN = -1)
                    _rows(x, hq, frac, acc, stage, x_lead=x_lead, tag=(form,), want=_run_form(L, stage, form, hn=(-1,)))
    x = _samples(rng, (16, 1000), np.uint8)
    for stage in STAGES:  # the HN = 0 / partial high-plane forms of a one-chunk filter (u8 out)
        one = stage == U8 and not RUN_FORMS[L][stage][1]
        # a Hann window of unity gain over >= 66 taps stays within a byte: no high plane at all
        _rows(x, _hann(L), 12, 32, stage, x_lead=8, tag=("hann",), want=_run_form(L, stage, "fast", hn=(0,) if one else (-1,)))
        _rows(x, _hann(L, "sinc"), 12, 32, stage, x_lead=8, tag=("sinc",),
              want=_run_form(L, stage, "fast", hn=(-1, 2, 4) if one else (-1,)))


# ---- the chunked int16 kernel (66 taps and up): six instantiations ---------------------------
LONG_SHAPES = [(1, 2056), (3, 1000), (5, 1032), (40, 8), (2, 4096)]


def _long_form(rng, L: int, form: str):
    if form == "fast":
        return _hann(L, "sinc" if L % 2 else "smooth"), 12, 32
    if form == "acc32":
        return _wrap_taps(rng, L), 12, 32
    return rng.integers(-3000, 3001, L), 16, 24


@pytest.mark.parametrize("form,want", [("fast", "fast"), ("acc32", "acc32"), ("acc24", "acclt32")])
@pytest.mark.parametrize("stage", STAGES, ids=["u8", "i32"])
@pytest.mark.parametrize("L,ks", [(66, 4), (481, 16), (483, 17), (993, 32), (995, 33), (4099, 130)])
def test_mfma_long_kernel(L, ks, stage, form, want):
    """(stage, form) name the instantiation: see the module docstring's table."""
    assert _ks(L) == ks
    rng = np.random.default_rng(L * 7 + stage)
    hq, frac, acc = _long_form(rng, L, form)
    assert _form(hq, np.int16, frac, acc) == want
    for shape in ([(2, 1032)] if L == 4099 else LONG_SHAPES):
        x = _samples(rng, shape, np.int16, pin_third=form == "acc32")

        def long_kernel(log, tag):
            l = _one(log, "fir1d_mfma_long_kernel", tag)
            assert l.targs == ("short", str(stage)) + _MFMA_FORM[want], (tag, l.inst)
            assert l.note["ks"] == str(ks), (tag, l.note)

        _rows(x, hq, frac, acc, stage, tag=(form,), want=long_kernel)


# ---- the generic kernel --------------------------------------------------------------------
GENERIC = {
    "channels3_i16": dict(dtype=np.int16, shape=(3, 3 * 333), L=5, ch=3),
    "channels3_u8": dict(dtype=np.uint8, shape=(1, 3 * 1025), L=9, ch=3),
    "acc40": dict(dtype=np.int16, shape=(7, 1000), L=5, acc=40),
    "frac33": dict(dtype=np.int16, shape=(7, 1000), L=5, frac=33, acc=40),
    "frac33_acc32": dict(dtype=np.uint8, shape=(1, 4099), L=3, frac=33, acc=32, amp=(1 << 31) - 1),
    "tap_2p31": dict(dtype=np.int16, shape=(2, 1024), L=3, amp=(1 << 31) - 1, pin=True),
    "ragged_31_i16": dict(dtype=np.int16, shape=(3, 1001), L=31),
    "ragged_31_u8": dict(dtype=np.uint8, shape=(3, 1001), L=31),
    "i16_x_lead8_40": dict(dtype=np.int16, shape=(3, 1032), L=40, x_lead=8),
    "i16_x_lead2_66": dict(dtype=np.int16, shape=(1, 2056), L=66, x_lead=2),
    "u8_x_lead1_33": dict(dtype=np.uint8, shape=(5, 1000), L=33, x_lead=1),
    "u8_x_lead4_66": dict(dtype=np.uint8, shape=(3, 3 * 1024 + 24), L=66, x_lead=4),
    "i16_y_lead_66": dict(dtype=np.int16, shape=(3, 1000), L=66, y_lead=4),
    "u8_y_lead_257": dict(dtype=np.uint8, shape=(16, 1000), L=257, y_lead=4),
    "long_4099_ch2": dict(dtype=np.int16, shape=(2, 2 * 300), L=4099, ch=2),
}


@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_kernel(name):
    p = dict(frac=12, acc=32, ch=1, amp=3000, x_lead=0, y_lead=0, pin=False)
    p.update(GENERIC[name])
    rng = np.random.default_rng(list(GENERIC).index(name))
    x = _samples(rng, p["shape"], p["dtype"], pin_third=p["pin"])
    hq = rng.integers(-p["amp"], p["amp"] + 1, p["L"])
    if p["amp"] == (1 << 31) - 1:
        hq[0] = (1 << 31) - 1
    for stage in STAGES:
        _rows(x, hq, p["frac"], p["acc"], stage, p["ch"], x_lead=p["x_lead"], y_lead=p["y_lead"],
              want="fir1d_generic_kernel")


# ---- segments with halos -------------------------------------------------------------------
SEG_INPUTS = [("u8", np.uint8, 1, (3, 9, 31, 64, 257)), ("i16", np.int16, 1, (3, 9, 31, 64, 257)),
              ("i16c2", np.int16, 2, (3, 9))]
SEG_CASES = [(e, n, d, c, L) for e in ("segment", "edges") for n, d, c, Ls in SEG_INPUTS for L in Ls]


def _long_rows_kernel(dtype, stage: int, L: int, n: int) -> str:
    """launch_fir1d_rows for ONE row of n samples, one channel, int16 taps of 3000 at most, aligned
    buffers, past the register kernel's 9 taps: the matrix cores from 10 taps (int16 -> int32: from
    40) when n is a multiple of 8 (step kernel up to three k-steps, then the run kernel for u8 and
    the chunked one for int16), else the LDS kernel up to 64 taps, else the generic kernel."""
    mfma_from = 40 if dtype == np.int16 and stage == I32 else 10
    if L >= mfma_from and n % 8 == 0:
        return "fir1d_mfma_step_kernel" if _ks(L) <= 3 else "fir1d_mfma_run_kernel" if dtype == np.uint8 else "fir1d_mfma_long_kernel"
    return "fir1d_lds_kernel" if L <= 64 else "fir1d_generic_kernel"


@pytest.mark.parametrize("entry,name,dtype,ch,L", SEG_CASES, ids=[f"{c[0]}-{c[1]}-{c[4]}" for c in SEG_CASES])
def test_segment_and_edges(entry, name, dtype, ch, L):
    """fir1d_fixed_segment_dev, and fir1d_fixed_rows_dev + fir1d_fixed_edges_dev on the same
    buffers; every halo a guarded input of its own (a vector load of a 1-sample halo sees poison)."""
    rng = np.random.default_rng(SEG_CASES.index((entry, name, dtype, ch, L)))
    co = c_oracle()
    hl_n, hr_n = fo.halo_sizes(L)
    tile = 4096 if dtype == np.uint8 else 512  # reg_tile_samples
    sizes = {"tiles": 2 * tile // ch, "ragged": 2 * tile // ch + 7, "all_edge": max(1, L // 2)}
    for frac, acc in ((12, 32), (16, 24)):
        hq = rng.integers(-8192, 8193, L) if L <= 9 else rng.integers(-3000, 3001, L)
        for stage in STAGES:
            for what, n in sizes.items():
                for side in ("both", "left", "right", "none"):
                    tag = (entry, name, L, frac, acc, stage, what, side)
                    x = _samples(rng, (n * ch,), dtype)
                    hl = _samples(rng, (hl_n * ch,), dtype) if side in ("both", "left") else None
                    hr = _samples(rng, (hr_n * ch,), dtype) if side in ("both", "right") else None
                    xg = guarded_input(torch.from_numpy(x), device=DEV)
                    hlg = None if hl is None else guarded_input(torch.from_numpy(hl), device=DEV)
                    hrg = None if hr is None else guarded_input(torch.from_numpy(hr), device=DEV)
                    y, check = guarded_output(x.shape, _TDT[stage], device=DEV)
                    with fir_hip.launch_log() as log:
                        if entry == "segment":
                            torch_ops.fir1d_fixed_segment_dev(xg, hq, hlg, hrg, frac, acc, stage, ch, out=y)
                        else:
                            torch_ops.fir1d_fixed_rows_dev(xg, hq, frac, acc, stage, ch, out=y)
                            torch_ops.fir1d_fixed_edges_dev(xg, hq, y, hlg, hrg, frac, acc, stage, ch)
                    torch.cuda.synchronize()
                    # the three routes of the table's row
                    if entry == "segment" and what == "tiles" and L <= 9:  # one launch, the halos in the kernel
                        form = _reg_form(dtype, ch, stage, hq, frac, acc, x.shape, halo=side != "none")
                        _is_reg(_one(log, "fir1d_reg_kernel", tag), dtype, stage, L, ch, form, tag)
                    else:  # the rows dispatch with zero padding, then the edges redone from the halos
                        assert len(log) == 2, (tag, [l.inst for l in log])
                        if L <= 9:
                            _is_reg(log[0], dtype, stage, L, ch, _reg_form(dtype, ch, stage, hq, frac, acc, x.shape), tag)
                        else:
                            assert log[0].kernel == _long_rows_kernel(dtype, stage, L, n), (tag, log[0].inst)
                        edge = "fir1d_generic_kernel" if what == "all_edge" else "fir1d_edges_kernel"
                        assert log[1].kernel == edge, (tag, log[1].inst)
                    _same(y, co.fir1d_rows(x, hq, frac, acc, stage, channels=ch, halo_left=hl, halo_right=hr), tag)
                    check(str(tag))


# ---- filter banks ------------------------------------------------------------------------------
def _banks(rng, F: int, L: int) -> dict:
    """Q4.12 taps (the v_dot2 byte-pair form, filter 0 of small taps), and a bank that fits the
    fused u8 kernel's packed-16 form (kU8Pk16: small integers times a power of two; unsigned,
    signed and high-byte filters, the last one of odd taps when there are several); "q412big":
    Q4.12 taps none of whose filters fits it (the plain byte-pair bank)."""
    q412 = rng.integers(-8192, 8193, (F, L))
    q412[0] = rng.integers(-8, 9, L)
    small = rng.integers(-12, 13, (F, L))
    small[0] = np.abs(small[0])
    shifts = rng.integers(0, 12, (F, 1))
    pk16 = small << shifts
    if F > 1:
        pk16[-1] = rng.integers(-3000, 3000, L) | 1
    for f in range(F):
        if not pk16[f].any():
            pk16[f, 0] = 1 << int(shifts[f, 0])
    big = rng.integers(4097, 8193, (F, L)) | 1  # odd taps whose sums pass 16 bits: no filter fits the packed-16 form
    return {"q412": q412, "q412big": big * rng.choice([-1, 1], (F, L)), "pk16": pk16}


def _bank_route(log, dtype, shape, F, L, kind, bank, stage, tag) -> None:
    """launch_fir1d_rows_multi: the fused register kernel over groups of <= 4 filters, or one
    launch_fir1d_rows per filter."""
    total = shape[0] * shape[1]
    fused = dtype == np.uint8 and shape[1] >= 16 + (L - 1) and (stage == U8 or total * 4 % 16 == 0)
    if not fused:
        assert len(log) == F and all(l.kernel in ("fir1d_reg_kernel", "fir1d_generic_kernel") and
                                     (l.kernel != "fir1d_reg_kernel" or l.targs[6] == "1") for l in log), (tag, [l.inst for l in log])
        if dtype == np.uint8 and shape[1] < 16 + (L - 1):  # rows narrower than a vector and its halo
            assert all(l.kernel == "fir1d_generic_kernel" for l in log), (tag, [l.inst for l in log])
        return
    groups = [min(4, F - f0) for f0 in range(0, F, 4)]
    assert [l.kernel for l in log] == ["fir1d_reg_kernel"] * len(groups), (tag, [l.inst for l in log])
    for g, (l, nf) in enumerate(zip(log, groups)):
        assert (l.targs[0], l.targs[1], l.targs[2], l.targs[6]) == ("unsigned char", str(stage), str(L), str(nf)), (tag, l.inst)
        assert "kU8Dot2" in l.flags, (tag, l.inst)  # every bank here has int16 taps whose u8 sums cannot wrap
        assert ("kRagged" in l.flags or "kMasked" in l.flags) == (shape[1] % 16 != 0), (tag, l.inst)
        if kind == "pk16":
            assert ("kU8Pk16" in l.flags) == (nf > 1 and stage == U8), (tag, l.inst)
        elif kind == "q412big":
            assert "kU8Pk16" not in l.flags, (tag, l.inst)
        else:  # "q412": filter 0's small taps fit the packed form, and one fitting filter is enough
            assert ("kU8Pk16" in l.flags) == (g == 0 and nf > 1 and stage == U8), (tag, l.inst)


@pytest.mark.parametrize("shape", [(3, 4499), (2, 4096), (5, 17)], ids=str)
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 9])
def test_rows_multi(F, shape):
    """fir1d_fixed_rows_multi_dev: guards around the whole (F, ...) block; the per-plane oracle
    comparison covers spill between planes (total % 16 != 0: u8 planes start at odd bytes)."""
    rng = np.random.default_rng(F * 100 + shape[1])
    co = c_oracle()
    for dtype in (np.uint8, np.int16):
        x = _samples(rng, shape, dtype)
        xg = guarded_input(torch.from_numpy(x), device=DEV)
        for L in (3, 5):
            for kind, bank in _banks(rng, F, L).items():
                for stage in STAGES:
                    tag = (dtype.__name__, F, shape, L, kind, stage)
                    y, check = guarded_output((F,) + shape, _TDT[stage], device=DEV)
                    with fir_hip.launch_log() as log:
                        torch_ops.fir1d_fixed_rows_multi_dev(xg, bank, 12, 32, stage, out=y)
                    torch.cuda.synchronize()
                    _bank_route(log, dtype, shape, F, L, kind, bank, stage, tag)
                    for f in range(F):
                        _same(y[f], co.fir1d_rows(x, bank[f], 12, 32, stage), tag + (f,))
                    check(str(tag))


@pytest.mark.parametrize("kind", ["q412", "q412big", "pk16"])
@pytest.mark.parametrize("L", [3, 5])
@pytest.mark.parametrize("F", [4, 6])
def test_images_multi(F, L, kind):
    """fir1d_fixed_images_multi_dev: every plane its own guarded output at leads 0, 16, 1, 7, 3,
    every image a guarded input, one of them a byte off 16 (the per-image path), one narrower
    than a vector plus the halo (per-image too)."""
    rng = np.random.default_rng(F * 10 + L)
    co = c_oracle()
    shapes = [(5, 4499), (3, 1280), (1, 5000), (2, 9)]
    xs = [_samples(rng, s, np.uint8) for s in shapes]
    xg = [guarded_input(torch.from_numpy(x), lead_bytes=1 if i == 1 else 0, device=DEV) for i, x in enumerate(xs)]
    bank = _banks(rng, F, L)[kind]
    leads = (0, 16, 1, 7, 3)
    outs, checks = [], []
    for i, s in enumerate(shapes):
        planes = [guarded_output(s, torch.uint8, lead_bytes=leads[(i + f) % 5], device=DEV) for f in range(F)]
        outs.append([p[0] for p in planes])
        checks.append([p[1] for p in planes])
    with fir_hip.launch_log() as log:
        torch_ops.fir1d_fixed_images_multi_dev(xg, bank, 12, 32, U8, outs=outs)
    torch.cuda.synchronize()
    # images 1 (a byte off 16) and 3 (narrower than 16 + L - 1) go per image and filter, on the
    # generic kernel; images 0 and 2 share the batch kernel, one launch per group of <= 4 filters,
    # in the deferred-store seam form since image 0's rows (4499) straddle vectors
    groups = [min(4, F - f0) for f0 in range(0, F, 4)]
    insts = [l.inst for l in log]
    assert [l.kernel for l in log] == ["fir1d_generic_kernel"] * (2 * F) + ["fir1d_reg_batch_kernel"] * len(groups), insts
    for g, (l, nf) in enumerate(zip(log[2 * F:], groups)):
        assert (l.targs[0], l.targs[1], l.targs[2], l.targs[6]) == ("unsigned char", str(U8), str(L), str(nf)), insts
        assert {"kU8Dot2", "kRagged", "kDefer"} <= l.flags, insts
        pk16 = {"pk16": nf > 1, "q412big": False, "q412": g == 0 and nf > 1}[kind]
        assert ("kU8Pk16" in l.flags) == pk16, (kind, insts)
    for i, x in enumerate(xs):
        for f in range(F):
            _same(outs[i][f], co.fir1d_rows(x, bank[f], 12, 32, U8), (F, L, kind, i, f))
            checks[i][f](str((F, L, kind, i, f)))


# ---- 2-D frames ------------------------------------------------------------------------------
def _outer(col, row):
    return np.outer(np.asarray(col), np.asarray(row)).astype(np.int64)


# name -> (FIR2D_PATH, taps, frac, stages): the five paths of launch_fir2d
FIR2D = {
    "sep3x3": (None, _outer([1, 2, 1], [16, 32, 16]), 8, STAGES),
    "sep5x5": (None, _outer([1, 4, 6, 4, 1], [16, 64, 96, 64, 16]), 12, STAGES),
    "sep3x3_big": (None, _outer([-181, 181, 181], [-181, 181, -181]), 4, STAGES),
    "general3x3_reg": ("reg", np.array([[0, -512, 0], [-512, 6144, -512], [0, -512, 0]]), 12, STAGES),
    "general5x5_reg": ("reg", np.arange(-12, 13).reshape(5, 5) * 37 + 300, 12, STAGES),
    "general3x3_reg_wide": ("reg", np.array([[-30000, 29000, 1], [32767, -32768, 77], [5, -20000, 31000]]), 12, STAGES),
    "mfma3x3_byte": (None, np.array([[1, -2, 3], [4, 100, -6], [7, 8, -9]]), 7, (U8,)),
    "mfma5x5_byte": (None, np.arange(-12, 13).reshape(5, 5) * 10 + 5, 10, (U8,)),
    "mfma3x3_two_plane": (None, np.array([[-30000, 29001, 1], [32639, -32768, 77], [5, -20001, 31001]]), 12, (U8,)),
    "mfma5x5_two_plane": (None, np.arange(-12, 13).reshape(5, 5) * 37 + 301, 12, (U8,)),
    "mfma_forced_sep3x3": ("mfma", _outer([1, 2, 1], [16, 32, 16]), 8, (U8,)),
    "mfma_forced_sep5x5": ("mfma", _outer([1, 4, 6, 4, 1], [16, 64, 96, 64, 16]), 12, (U8,)),
}


def _fir2d_route(name: str, stage: int, hq2):
    """What launch_fir2d picks for a case of FIR2D (the table's test_fir2d_* row): the separable
    register forms (u8 out whose sums fit 16 bits: the packed-16 strip kernel), the general register
    forms under FIR2D_PATH=reg, the matrix-core kernel with one or two tap planes."""
    R, C = np.asarray(hq2).shape

    def want(log, tag):
        if name.startswith("mfma"):
            l = _one(log, "fir2d_mfma_kernel", tag)
            assert l.targs[:2] == (str(R), "2" if "two_plane" in name else "1"), (tag, l.inst)
        elif name.startswith("sep") and stage == U8 and name != "sep3x3_big":
            l = _one(log, "fir2d_pk16_strip_kernel", tag)
            assert l.targs[:2] == (str(R), str(C)) and "pk16" in l.flags, (tag, l.inst)
        else:
            l = _one(log, "fir2d_reg_kernel", tag)
            assert l.targs[:3] == (str(R), str(C), str(stage)), (tag, l.inst)
            assert ("sep" in l.flags) == name.startswith("sep") and ("dot2" in l.flags) == name.startswith("general"), (tag, l.inst)
            if name == "general3x3_reg" and stage == U8:  # the sharpen kernel's sums fit 16 bits
                assert "pk16" in l.flags, (tag, l.inst)
            else:
                assert "pk16" not in l.flags, (tag, l.inst)
    return want


def _frames(rng, frames, H, W, hq2, frac, acc, stage, x_lead=0, y_lead=0, tag=(), want="fir2d_generic_kernel"):
    co = c_oracle()
    shape = (H, W) if frames == 1 else (frames, H, W)
    x = _samples(rng, shape, np.uint8)
    xg = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    y, check = guarded_output(shape, _TDT[stage], lead_bytes=y_lead, device=DEV)
    with fir_hip.launch_log() as log:
        torch_ops.fir2d_fixed_dev(xg, hq2, frac, acc, stage, out=y)
    torch.cuda.synchronize()
    tag = (frames, H, W, frac, acc, stage, x_lead, y_lead) + tuple(tag)
    if isinstance(want, str):
        _one(log, want, tag)
    else:
        want(log, tag)
    want = np.stack([co.fir2d(f, hq2, frac, acc, stage) for f in x.reshape(-1, H, W)]).reshape(shape)
    _same(y, want, tag)
    check(str(tag))


@pytest.mark.parametrize("W", [16, 1024, 1040])
@pytest.mark.parametrize("name", list(FIR2D))
def test_fir2d_paths(name, W, monkeypatch):
    path, hq2, frac, stages = FIR2D[name]
    if path is None:
        monkeypatch.delenv("FIR2D_PATH", raising=False)
    else:
        monkeypatch.setenv("FIR2D_PATH", path)
    rng = np.random.default_rng(list(FIR2D).index(name) * 10000 + W)
    for H in (1, 2, 17, 33):  # 17: one row past a 16-row strip; 33: one past the 32-row strips
        for frames in (1, 3):
            for stage in stages:
                _frames(rng, frames, H, W, hq2, frac, 32, stage, tag=(name,), want=_fir2d_route(name, stage, hq2))
    _frames(rng, 3, 33, W, hq2, frac, 24, stages[0], tag=(name, "acc24"), want=_fir2d_route(name, stages[0], hq2))


@pytest.mark.parametrize("why", ["7x7", "W17", "x_lead1", "y_lead1", "y_lead4_i32", "acc40"])
def test_fir2d_generic(why, monkeypatch):
    monkeypatch.delenv("FIR2D_PATH", raising=False)
    rng = np.random.default_rng(len(why))
    h3, h7 = rng.integers(-3000, 3001, (3, 3)), rng.integers(-800, 801, (7, 7))
    for H in (1, 2, 17, 33):
        for frames in (1, 3):
            if why == "7x7":
                for stage in STAGES:
                    _frames(rng, frames, H, 16, h7, 12, 32, stage, tag=(why,))
                    _frames(rng, frames, H, 1040, h7, 12, 32, stage, tag=(why,))
            elif why == "W17":
                for stage in STAGES:
                    _frames(rng, frames, H, 17, h3, 12, 32, stage, tag=(why,))
            elif why == "x_lead1":
                for stage in STAGES:
                    _frames(rng, frames, H, 1024, h3, 12, 32, stage, x_lead=1, tag=(why,))
            elif why == "y_lead1":
                _frames(rng, frames, H, 1024, h3, 12, 32, U8, y_lead=1, tag=(why,))
            elif why == "y_lead4_i32":
                _frames(rng, frames, H, 16, h3, 12, 32, I32, y_lead=4, tag=(why,))
            else:
                for stage in STAGES:
                    _frames(rng, frames, H, 1024, h3, 12, 40, stage, tag=(why,))


# ---- float64 ideal rows, restore, metrics ------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 1001), (3, 4096)], ids=str)
@pytest.mark.parametrize("L", [1, 3, 5, 11, 257])
def test_ideal_rows(L, shape):
    rng = np.random.default_rng(L * 10 + shape[0])
    co = c_oracle()
    x = _samples(rng, shape, np.uint8)
    h = rng.standard_normal(L)
    want = co.fir1d_ideal_rows(x, h)
    for x_lead, y_lead in ((0, 0), (1, 0), (0, 8), (16, 16)):
        xg = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
        y, check = guarded_output(shape, torch.float64, lead_bytes=y_lead, device=DEV)
        with fir_hip.launch_log() as log:
            torch_ops.fir1d_ideal_rows_dev(xg, h, out=y)
        torch.cuda.synchronize()
        # up to 9 taps on aligned buffers: the register form (L its template argument); else LDS
        if L <= 9 and x_lead % 4 == 0 and y_lead % 16 == 0:
            assert _one(log, "fir1d_ideal_reg_kernel", (L, shape, x_lead, y_lead)).targs[0] == str(L)
        else:
            _one(log, "fir1d_ideal_kernel", (L, shape, x_lead, y_lead))
        _same(y, want, (L, shape, x_lead, y_lead))  # compared as uint64 views
        check(str((L, shape, x_lead, y_lead)))


@pytest.mark.parametrize("policy", [fir_hip.RESTORE_CLIP, fir_hip.RESTORE_NORMALIZE], ids=["clip", "normalize"])
@pytest.mark.parametrize("n", [1, 1023, 1025, 3 * 4096 + 5])
def test_restore_u8(n, policy):
    rng = np.random.default_rng(n + policy)
    a = rng.uniform(-80.0, 340.0, n)
    a[rng.integers(0, n, max(1, n // 50))] = np.round(a[:max(1, n // 50)]) + 0.5  # ties
    want = fo.to_u8_clip(a) if policy == fir_hip.RESTORE_CLIP else fo.to_u8_normalized(a)
    wb = int(fir_hip.lib().fir_restore_work_bytes())
    for lead in (0, 16):
        ag = guarded_input(torch.from_numpy(a), lead_bytes=lead, device=DEV)
        y, check = guarded_output((n,), torch.uint8, lead_bytes=lead, device=DEV)
        work, check_work = guarded_output((wb,), torch.uint8, device=DEV)
        with fir_hip.launch_log() as log:
            torch_ops.restore_u8_dev(ag, policy, out=y, work=work)
        torch.cuda.synchronize()
        if policy == fir_hip.RESTORE_CLIP:  # one map, no parameters
            assert [l.inst for l in log] == ["restore_map_kernel<false>"], (n, lead, [l.inst for l in log])
        else:  # min / max, the scale, then the map with it
            assert [l.inst for l in log] == ["restore_minmax_kernel", "restore_params_kernel",
                                             "restore_map_kernel<true>"], (n, lead, [l.inst for l in log])
        _same(y, want, (n, policy, lead))
        check(f"out {(n, policy, lead)}")
        check_work(f"work {(n, policy, lead)}")


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32], ids=["u8", "i16", "f32"])
@pytest.mark.parametrize("n", [1, 8193, 3 * 8192 + 129])
def test_compare_metrics(n, dtype):
    rng = np.random.default_rng(n + np.dtype(dtype).itemsize)
    yi = rng.uniform(-64.0, 320.0, n)
    yf = np.rint(yi) + rng.integers(-3, 4, n)
    yf = (np.clip(yf, 0, 255) if dtype == np.uint8 else yf).astype(dtype)
    want = fo.compute_metrics(yi, yf)
    need = int(fir_hip.lib().fir_metrics_work_bytes(n))
    item = np.dtype(dtype).itemsize
    for i_lead, f_lead in ((0, 0), (8, 0), (0, item), (16, 16)):
        ig = guarded_input(torch.from_numpy(yi), lead_bytes=i_lead, device=DEV)
        fg = guarded_input(torch.from_numpy(yf), lead_bytes=f_lead, device=DEV)
        out, check = guarded_output((9,), torch.float64, device=DEV)
        work, check_work = guarded_output((need,), torch.uint8, device=DEV)
        with fir_hip.launch_log() as log:
            torch_ops.compare_metrics_dev(ig, fg, out=out, work=work)
        torch.cuda.synchronize()
        # launch_metrics_t: aligned u8 with a full 8192-sample block: the one streaming pass (vector
        # loads); other u8: metrics_blocks per part; other types: the scalar metrics_blocks_any<T>;
        # then the ragged last block and the final sum
        ks = [l.kernel for l in log]
        vec, full, ragged = i_lead % 16 == 0 and f_lead % 16 == 0, n // 8192 > 0, n % 8192 > 0
        if dtype == np.uint8 and vec and full:
            assert ks == ["metrics_prep", "metrics_leaf_kernel"], (n, i_lead, f_lead, ks)
        else:
            blocks = "metrics_blocks" if dtype == np.uint8 else "metrics_blocks_any"
            assert ks == [blocks] * full + ["metrics_ragged"] * ragged + ["metrics_final"], (n, i_lead, f_lead, ks)
            ct = {np.uint8: "unsigned char", np.int16: "short", np.float32: "float"}[dtype]
            assert all(l.targs == (ct,) for l in log if l.kernel in ("metrics_blocks_any", "metrics_ragged")), [l.inst for l in log]
        got = fir_hip.metrics_from_sums(out.cpu().numpy(), n)
        bad = same_metrics(got, want)
        assert not bad, (n, dtype.__name__, i_lead, f_lead, {k: (got[k], want[k]) for k in bad})
        check(f"out {(n, i_lead, f_lead)}")
        check_work(f"work {(n, i_lead, f_lead)}")
