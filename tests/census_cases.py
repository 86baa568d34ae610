"""The kernel census by family, and the generated cases that launch each family's share of it.

``fir_hip.kernel_census()`` lists every kernel instantiation a launch site of the library can name.
FAMILIES splits it by kernel template (the register kernel further by build configuration, the 12
INSTS of csrc/Makefile); ``family_of`` places a record, and every record has exactly one family
(tests/test_cabi.py checks that without a GPU).  ``cases(family)`` yields callables: each makes one
or a few small calls on the GPU and compares every output bit for bit with the C oracle.  The
generators are loops over tap count, filter count, stage, sample type, channels, arithmetic form and
geometry; the shapes are the smallest at which the kernel can still go wrong: two of the kernel's
own tiles and some, a row seam for the multi-row forms, a width one sample short of whole vectors
for the ragged and masked forms, halos for kHalo.  tests/test_gpu_kernel_census.py runs them under
``fir_hip.launch_log()`` and holds the set of instantiations each family launched against the census.

Instantiations are named by ``key``: ``kernel<template arguments> [flags in words]``.
UNREACHED: instantiation (an ``fnmatch`` pattern over ``key``) -> why no argument of any
entry that ends can launch it, citing the source line; UNREACHED_COUNT: how many census entries each
pattern matches, asserted.  Every family has a generator (GENERATED == FAMILIES, asserted).
"""
from __future__ import annotations

import fnmatch

import numpy as np

import fir_hip

U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
_CT = {"unsigned char": "u8", "short": "i16"}

# kernel template -> family; the register kernel's families carry the build configuration
_FAMILY_OF_KERNEL = {
    "fir1d_reg_batch_kernel": "batch",
    "fir1d_mfma_step_kernel": "mfma_step", "fir1d_mfma_run_kernel": "mfma_run", "fir1d_mfma_long_kernel": "mfma_long",
    "fir1d_lds_kernel": "lds", "fir1d_generic_kernel": "generic", "fir1d_edges_kernel": "edges",
    "fir1d_decim_kernel": "decim", "fir1d_decim_generic_kernel": "decim",
    "fir1d_interp_kernel": "interp", "fir1d_interp_generic_kernel": "interp",
    "fir1d_resample_kernel": "resample", "fir1d_resample_generic_kernel": "resample",
    "fir1d_cplx_kernel": "cplx", "fir1d_cplx_generic_kernel": "cplx", "fir1d_cplx_generic32_kernel": "cplx",
    "fir2d_reg_kernel": "fir2d_reg", "fir2d_pk16_strip_kernel": "fir2d_pk16", "fir2d_mfma_kernel": "fir2d_mfma",
    "fir2d_generic_kernel": "fir2d_generic",
    "fir1d_ideal_reg_kernel": "ideal", "fir1d_ideal_kernel": "ideal",
    "fir2d_ideal_reg_kernel": "ideal2d", "fir2d_ideal_generic_kernel": "ideal2d",
    "metrics_prep": "metrics", "metrics_leaf_kernel": "metrics", "metrics_blocks": "metrics",
    "metrics_blocks_any": "metrics", "metrics_ragged": "metrics", "metrics_final": "metrics",
    "restore_map_kernel": "restore", "restore_minmax_kernel": "restore", "restore_params_kernel": "restore",
    "halo_gate_kernel": "halo", "halo_mailbox_init_kernel": "halo",
}
REG_CONFIGS = ["u8_0_1_1", "u8_0_1_2", "u8_0_1_3", "u8_0_1_4", "u8_1_1_1", "u8_1_1_2", "u8_1_1_3", "u8_1_1_4",
               "i16_0_1_1", "i16_1_1_1", "i16_0_2_1", "i16_1_2_1"]  # INSTS of csrc/Makefile: type_stage_ch_f
FAMILIES = ["reg_" + c for c in REG_CONFIGS] + sorted(set(_FAMILY_OF_KERNEL.values()))


def family_of(l) -> str | None:
    """The one family of a Launch / census record; None for a kernel no family claims."""
    if l.kernel == "fir1d_reg_kernel":
        t = l.targs
        cfg = f"{_CT.get(t[0], t[0])}_{t[1]}_{t[3]}_{t[6]}"
        return "reg_" + cfg if cfg in REG_CONFIGS else None
    return _FAMILY_OF_KERNEL.get(l.kernel)


def key(l) -> str:
    """An instantiation's name: kernel<template arguments> [its bit-mask argument's flags in words]."""
    return f"{l.inst} [{'|'.join(sorted(l.flags))}]"


def census_of(family: str) -> set:
    return {key(l) for l in fir_hip.kernel_census() if family_of(l) == family}


UNREACHED: dict = {
    "fir1d_reg_batch_kernel<short, *": "fir1d.hip:341 sends only u8 -> u8 images of one channel to the batch kernel and "
                                       "fir1d.hip:370 names launch_reg_batch_taps<uint8_t, ...> alone; the int16 forms exist "
                                       "because fir1d_reg_inst.hip instantiates the batch launcher for every configuration",
    "fir1d_mfma_step_kernel<short, 1, 2, *": "fir1d.hip:261: int16 -> int32 takes the matrix cores from kMfmaMinTapsI32 = 40 "
                                             "taps on, and 40 taps are already three k-steps (two end at 33 taps)",
    "fir1d_mfma_run_kernel<0, [45], false, 1, 2>*": "fir1d_mfma.hip:955: a partial high plane of 2 k-steps is taken only "
                                                    "when ksp >= 6",
    "fir1d_mfma_run_kernel<0, [4-9], false, 1, 4>*": "fir1d_mfma.hip:955: a partial high plane of 4 k-steps is taken only "
                                                     "when ksp >= 12",
    "fir1d_mfma_run_kernel<0, 1[01], false, 1, 4>*": "fir1d_mfma.hip:955: a partial high plane of 4 k-steps is taken only "
                                                     "when ksp >= 12",
    "fir2d_reg_kernel<1, ?, * [[]*sep*": "fir2d.hip:158: the separable forms need tap_rows > 1 and tap_cols > 1 (launch2d_reg "
                                         "compiles them for every shape, one-row kernels included)",
    "fir2d_reg_kernel<[35], 1, * [[]*sep*": "fir2d.hip:158: the separable forms need tap_rows > 1 and tap_cols > 1",
    "fir2d_pk16_strip_kernel<1, ?, *": "fir2d.hip:158: the separable packed-16 strips need tap_rows > 1 and tap_cols > 1",
    "fir2d_pk16_strip_kernel<[35], 1, *": "fir2d.hip:158: the separable packed-16 strips need tap_rows > 1 and tap_cols > 1",
    "fir1d_edges_kernel<unsigned char, ?, true>*": "fir1d.hip (needs_wide): 128-bit sums need sum|h| * 255 >= 2^63, with int32 taps "
                                                   "2^24 of them at least; fir1d.hip:413 gives the edges kernel only shards longer "
                                                   "than their halos, so it would redo 2^24 outputs of 2^24 taps each: 2^48 "
                                                   "128-bit MACs, days of GPU time.  No call that ends can launch it",
}



# how many census entries each UNREACHED pattern matches: a pattern that a typo widens (or a library
# change empties) fails test_gpu_kernel_census / test_cabi by count
UNREACHED_COUNT = {
    'fir1d_reg_batch_kernel<short, *': 72,
    'fir1d_mfma_step_kernel<short, 1, 2, *': 3,
    'fir1d_mfma_run_kernel<0, [45], false, 1, 2>*': 2,
    'fir1d_mfma_run_kernel<0, [4-9], false, 1, 4>*': 6,
    'fir1d_mfma_run_kernel<0, 1[01], false, 1, 4>*': 2,
    'fir2d_reg_kernel<1, ?, * [[]*sep*': 33,
    'fir2d_reg_kernel<[35], 1, * [[]*sep*': 22,
    'fir2d_pk16_strip_kernel<1, ?, *': 9,
    'fir2d_pk16_strip_kernel<[35], 1, *': 6,
    'fir1d_edges_kernel<unsigned char, ?, true>*': 2,
}
assert set(UNREACHED_COUNT) == set(UNREACHED)


def listed(inst: str, table: dict) -> bool:
    return any(fnmatch.fnmatchcase(inst, p) for p in table)


def expected(family: str) -> set:
    """The instantiations the family's cases must launch: its census minus UNREACHED."""
    return {i for i in census_of(family) if not listed(i, UNREACHED)}


# ---- data ---------------------------------------------------------------------------------------
def samples(rng, shape, dtype) -> np.ndarray:
    """Full-range random samples with runs of the extreme values (as test_gpu_containment's)."""
    if np.dtype(dtype) == np.uint8:
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        lo, hi = 0, 255
    else:
        x = rng.integers(-32768, 32768, shape, dtype=np.int16)
        lo, hi = -32768, 32767
    flat = x.reshape(-1)
    n = flat.size
    run = max(1, min(n // 9, 70))
    for k, v in enumerate((lo, hi, hi, lo)):
        s = n * (2 * k + 1) // 9
        flat[s:s + run] = v
    return x


def _same(got, want, tag) -> None:
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{tag}: {bad.size} of {want.size} outputs differ from the oracle; the first at flat "
                             f"index {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}")


def _oracle():
    from oracle import c_oracle
    return c_oracle()


# ---- the register kernel, per build configuration ------------------------------------------------
REG_TILE = {np.uint8: 64 * 4 * 16, np.int16: 64 * 8}  # reg_tile_samples (fir1d_reg_launch.h)


def _reg_taps(rng, L: int, arith: str, F: int = 1, acc: int = 32) -> np.ndarray:
    """The taps of one arithmetic form, chosen so that no other form can take them.
    dot2: int16 taps whose u8 sums cannot wrap the accumulator (32 bits at frac 12, 24 bits at frac 6),
    and in EVERY filter an odd centre tap of magnitude >= 1001: 255 * 1001 passes 16 bits either way,
    so no filter fits the packed-16 form (plan_u8_pk16) and a bank stays on byte-pair v_dot2;
    pk16: small taps times a power of two, every filter within 16 bits; mad: one tap past int16
    (below 2^23), which takes the whole bank off v_dot2."""
    if arith == "pk16":
        h = rng.integers(-6, 7, (F, L)) << int(rng.integers(0, 3))
        h[:, 0] |= 4
        return h
    h = rng.integers(-3000, 3001, (F, L)) if acc == 32 else rng.integers(-47, 48, (F, L))
    h[:, L // 2] = (rng.integers(1001, 1024, F) | 1) * rng.choice([-1, 1], F)
    if arith == "mad":
        h[0, 0] = 40000 + int(rng.integers(0, 1000))
    return h


def reg_cases(cfg: str):
    """One configuration (type, stage, channels, filters) of fir1d_reg_kernel: every tap count 1..9 x
    arithmetic (byte-pair / packed v_dot2, mad24) x accumulator (32 bits, 24 bits) x geometry
    (whole-vector rows, rows one sample short of whole vectors, one row, one row with halos)."""
    tname, stage, ch, F = cfg.split("_")
    dtype, stage, ch, F = (np.uint8 if tname == "u8" else np.int16), int(stage), int(ch), int(F)
    vec = 16 if dtype == np.uint8 else 8
    tile = REG_TILE[dtype]
    # the packed-16 form exists for fused u8 -> u8 banks only (launch_reg: F > 1, u8 stage)
    ariths = ("dot2", "mad", "pk16") if dtype == np.uint8 and stage == U8 and F > 1 else ("dot2", "mad")
    for L in range(1, 10):
        for arith in ariths:
            for frac, acc in ((12, 32), (6, 24)):
                def run(L=L, arith=arith, frac=frac, acc=acc):
                    import torch
                    from fir_hip import torch_ops
                    dev = torch.device("cuda:0")
                    rng = np.random.default_rng(L * 100 + acc + len(arith))
                    co = _oracle()
                    hq = _reg_taps(rng, L, arith, F, acc)
                    width = 2 * tile // ch + 3 * vec  # two wave tiles and some, in frames
                    # (4 rows: the ragged int32 planes of a bank stay whole 16-byte runs, so it stays fused)
                    geoms = {"whole": (3, width), "ragged": (4, width - 1), "row": (1, width)}
                    for what, (rows, w) in geoms.items():
                        x = samples(rng, (rows, w * ch), dtype)
                        tag = (cfg, L, arith, acc, what)
                        if F == 1:
                            got = fir_hip.fir1d_fixed_rows(x, hq[0], frac, acc, stage, channels=ch)
                            _same(got, co.fir1d_rows(x, hq[0], frac, acc, stage, channels=ch), tag)
                        else:
                            got = fir_hip.fir1d_fixed_rows_multi(x, hq, frac, acc, stage)
                            for f in range(F):
                                _same(got[f], co.fir1d_rows(x, hq[f], frac, acc, stage), tag + (f,))
                    if F == 1 and L > 1:  # a shard of whole tiles with both halos: the kHalo form
                        n = 2 * tile // ch
                        hl_n, hr_n = L - 1 - L // 2, L // 2
                        x = samples(rng, (n * ch,), dtype)
                        hl = samples(rng, (max(hl_n, 1) * ch,), dtype)[:hl_n * ch]
                        hr = samples(rng, (max(hr_n, 1) * ch,), dtype)[:hr_n * ch]
                        td = lambda a: torch.from_numpy(a).to(dev) if a.size else None  # noqa: E731
                        y = torch_ops.fir1d_fixed_segment_dev(td(x), hq[0], td(hl), td(hr), frac, acc, stage, ch)
                        torch.cuda.synchronize()
                        want = co.fir1d_rows(x, hq[0], frac, acc, stage, channels=ch,
                                             halo_left=hl if hl.size else None, halo_right=hr if hr.size else None)
                        _same(y.cpu().numpy(), want, (cfg, L, arith, acc, "halo"))
                    if F == 1 and L == 1:
                        # kHalo at one tap: no halo sample exists, so torch_ops passes NULL; the C entry
                        # with non-NULL halo pointers takes the kHalo kernel.  The kernel reads a halo
                        # only under NDL > 0 / NDR > 0 (fir1d_reg.h, the lane 0 / lane 63 edge loads),
                        # which are 0 at one tap: the pointers (here x itself) are never dereferenced.
                        import ctypes
                        x = samples(rng, (2 * tile,), dtype)
                        xd = torch.from_numpy(x).to(dev)
                        y = torch.empty(x.shape, dtype=torch.uint8 if stage == U8 else torch.int32, device=dev)
                        h = (ctypes.c_int32 * 1)(int(hq[0][0]))
                        vp = ctypes.c_void_p
                        rc = fir_hip.lib().fir1d_fixed_segment_dev(vp(xd.data_ptr()), 0 if dtype == np.uint8 else 1,
                                                                  x.size // ch, ch, h, 1, frac, acc, stage, vp(xd.data_ptr()),
                                                                  vp(xd.data_ptr()), vp(y.data_ptr()),
                                                                  vp(torch.cuda.current_stream().cuda_stream))
                        assert rc == 0, fir_hip.lib().fir_last_error()
                        torch.cuda.synchronize()
                        _same(y.cpu().numpy(), co.fir1d_rows(x, hq[0], frac, acc, stage, channels=ch), (cfg, arith, acc, "halo L=1"))
                yield run


def batch_cases():
    """fir1d_reg_batch_kernel (u8 -> u8 image batches): tap counts 1..9 x filters 1..4 x arithmetic
    x accumulator x (every image of whole-vector rows | one image whose rows straddle vectors)."""
    for L in range(1, 10):
        for F in range(1, 5):
            for arith in ("dot2", "mad", "pk16"):
                for frac, acc in ((12, 32), (6, 24)):
                    def run(L=L, F=F, arith=arith, frac=frac, acc=acc):
                        rng = np.random.default_rng(L * 1000 + F * 10 + acc)
                        co = _oracle()
                        hq = _reg_taps(rng, L, arith, F, acc)
                        for ragged in (False, True):
                            shapes = [(3, 4096 + 48), (2, 4096 + (47 if ragged else 32)), (1, 5000)]
                            xs = [samples(rng, s, np.uint8) for s in shapes]
                            got = fir_hip.fir1d_fixed_images_multi(xs, hq, frac, acc, U8)
                            for i, x in enumerate(xs):
                                for f in range(F):
                                    _same(got[i][f], co.fir1d_rows(x, hq[f], frac, acc, U8), (L, F, arith, acc, ragged, i, f))
                    yield run


# ---- the long-filter 1-D kernels ------------------------------------------------------------------
def _rows_case(dtype, shape, hq, frac, acc, stage, ch=1, tag=()):
    def run():
        rng = np.random.default_rng(len(hq) * 31 + shape[1])
        x = samples(rng, shape, dtype)
        got = fir_hip.fir1d_fixed_rows(x, hq, frac, acc, stage, channels=ch)
        _same(got, _oracle().fir1d_rows(x, hq, frac, acc, stage, channels=ch),
              (np.dtype(dtype).name, shape, len(hq), frac, acc, stage) + tuple(tag))
    return run


def _form_taps(rng, L: int, form: str):
    """(taps, frac, acc) of the three arithmetic forms of the matrix-core kernels: no wrap possible
    ("fast"), a 32-bit accumulator that can wrap, a narrower one."""
    if form == "fast":
        w = np.hanning(L + 2)[1:-1]
        return np.rint(w / w.sum() * 4096).astype(np.int64), 12, 32
    if form == "acc32":
        h = rng.choice(np.array([-32768, 32639, 1, -1, 127, 128, -129]), L)
        h[0], h[L // 2], h[-1] = -32768, -32768, 32639
        return h, 24, 32
    h = rng.integers(-30000, 30001, L)
    h[0], h[-1] = 30000, -30000
    return h, 16, 24


def mfma_step_cases():
    """fir1d_mfma_step_kernel<InT, STAGE, KS, ACC32, FAST>: 2 and 3 k-steps (10 and 64 taps; int16
    -> int32 takes the matrix cores from 40 taps on: 64 only) x sample type x stage x form."""
    for dtype in (np.uint8, np.int16):
        for stage in (U8, I32):
            for L in ((64,) if dtype == np.int16 and stage == I32 else (10, 64)):
                for form in ("fast", "acc32", "acc24"):
                    hq, frac, acc = _form_taps(np.random.default_rng(L), L, form)
                    if form == "acc32" and dtype == np.int16:
                        frac = 12
                    yield _rows_case(dtype, (3, 2 * 1024 + 8), hq, frac, acc, stage, tag=(form,))


def mfma_long_cases():
    """fir1d_mfma_long_kernel<int16, STAGE, ACC32, FAST>: 66 taps (4 k-steps) and 483 (17: two
    chunks) x stage x form."""
    for stage in (U8, I32):
        for L in (66, 483):
            for form in ("fast", "acc32", "acc24"):
                hq, frac, acc = _form_taps(np.random.default_rng(L), L, form)
                yield _rows_case(np.int16, (3, 2 * 1024 + 8), hq, 12 if form == "acc32" else frac, acc, stage, tag=(form,))


def _ks16(L: int) -> int:
    c = L // 2
    return (32 + c + ((L - 1 - c + 15) & ~15) + 31) // 32


def mfma_run_cases():
    """fir1d_mfma_run_kernel<STAGE, NS, MULTI, TPS, HN>: every k-step count 4..88 (the first tap
    count of each) x stage, with taps past a byte everywhere (HN = -1); and for the one-chunk u8-out
    forms the three high-plane forms: all taps within a byte (HN = 0), one large tap (2), two large
    taps 80 taps apart (4)."""
    first = {}
    for L in range(66, 2800):  # 85 k-steps and up: the int32 stage's chunks of 8
        first.setdefault(_ks16(L), L)
    for ks, L in sorted(first.items()):
        for stage in (U8, I32):
            rng = np.random.default_rng(L)
            yield _rows_case(np.uint8, (3, 2 * 1024 + 24), rng.integers(-400, 401, L), 12, 32, stage, tag=("hn-1",))
        if ks <= 32:
            rng = np.random.default_rng(L + 1)
            small = rng.integers(-128, 128, L)
            one, two = small.copy(), small.copy()
            one[L // 2] = 2000
            two[L // 2], two[min(L - 1, L // 2 + 80)] = 2000, -1500
            for name, hq in (("hn0", small), ("hn2", one), ("hn4", two)):
                yield _rows_case(np.uint8, (3, 2 * 1024 + 24), hq, 12, 32, U8, tag=(name,))


def lds_cases():
    """fir1d_lds_kernel<InT, STAGE, LP, ACC32>: every tap count 10..64 x sample type x stage x
    accumulator, with one tap past the matrix cores' byte split (32640) so that they refuse."""
    for dtype in (np.uint8, np.int16):
        for stage in (U8, I32):
            for L in range(10, 65):
                for frac, acc in ((12, 32), (16, 24)):
                    hq = np.random.default_rng(L).integers(-3000, 3001, L)
                    hq[L // 3] = 32640
                    yield _rows_case(dtype, (3, 2 * 2048 + 8), hq, frac, acc, stage)


def generic_cases():
    """fir1d_generic_kernel<InT, STAGE, WIDE>: three channels (no fast path takes them) x sample type
    x stage; and the 128-bit form."""
    for dtype in (np.uint8, np.int16):
        for stage in (U8, I32):
            yield _rows_case(dtype, (3, 3 * 700), np.random.default_rng(3).integers(-3000, 3001, 5), 12, 32, stage, ch=3)
    yield from _wide_rows_cases()


# ---- the 2-D register kernels ------------------------------------------------------------------------
_VEC = {1: [1], 3: [1, 2, 1], 5: [1, 2, 3, 2, 1]}


def _fir2d_kernels(R: int, C: int):
    """(name, taps, frac, acc) over one tap shape: one kernel per arithmetic form launch2d_reg
    (fir2d.hip) can pick.  Rank-1 kernels (R, C > 1): the separable forms by the size of the row
    sums (sep16: 255 * sum|row| <= 32767) and the accumulator (nowrap), and for the u8 stage the
    packed-16 strip forms (unsigned, high byte: frac - s == 8, signed).  Kernels of full rank: the
    general v_dot2 forms (nowrap or not) and the general packed-16 forms."""
    col, row = np.array(_VEC[R]), np.array(_VEC[C])
    out = []
    if R > 1 and C > 1:
        wide = row * 100  # row taps of gcd 1 (rank1_factor divides the gcd out) whose sums pass int16
        wide[0] += 1
        wide[-1] += 1
        out += [("sep16_nowrap", np.outer(col * 300, row * 10), 12, 32), ("sep16_wrap", np.outer(col * 300, row * 10), 4, 20),
                ("sep_nowrap", np.outer(col * 3, wide), 12, 32), ("sep_wrap", np.outer(col * 3, wide), 4, 20),
                ("strip_unsigned", np.outer(col, row), 4, 32), ("strip_hi8", np.outer(col, row), 8, 32),
                ("strip_signed", np.outer(col * np.where(np.arange(R) % 2, -1, 1), row), 4, 32)]
    rng = np.random.default_rng(R * 10 + C)
    full = rng.integers(-3000, 3001, (R, C))
    full[0, 0], full[-1, -1] = 2999, -2998  # never rank 1 (for R, C > 1)
    small = rng.integers(1, 4, (R, C))
    small[0, 0], small[-1, -1] = 1, 3 if R * C > 1 else 1
    if R > 1 and C > 1:
        small[0, -1], small[-1, 0] = 3, 1  # rows not proportional
    signed = small * np.where(np.arange(R * C).reshape(R, C) % 2, 1, -1)  # (a 1 x 1 kernel: its one tap negative)
    out += [("dot2_nowrap", full, 12, 32), ("dot2_wrap", full * 10, 4, 20), ("pk_unsigned", small, 4, 32),
            ("pk_hi8", small, 8, 32), ("pk_signed", signed, 4, 32)]
    return out


class _env:
    """FIR2D_PATH for the length of a call (the library reads it at each call)."""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        import os
        self.old = os.environ.get("FIR2D_PATH")
        os.environ["FIR2D_PATH"] = self.value

    def __exit__(self, *exc):
        import os
        if self.old is None:
            del os.environ["FIR2D_PATH"]
        else:
            os.environ["FIR2D_PATH"] = self.old


def fir2d_reg_cases():
    """fir2d_reg_kernel and fir2d_pk16_strip_kernel: every tap shape {1, 3, 5}^2 x stage x the
    kernels of _fir2d_kernels, under FIR2D_PATH=reg, over 35 x 8208 frames (two 16-row strips and
    some, one past the 32-row strips; two 4096-pixel workgroups and a vector), two frames."""
    for R in (1, 3, 5):
        for C in (1, 3, 5):
            for stage in (U8, I32):
                def run(R=R, C=C, stage=stage):
                    co = _oracle()
                    x = samples(np.random.default_rng(R + C), (2, 35, 8208), np.uint8)
                    for name, hq2, frac, acc in _fir2d_kernels(R, C):
                        with _env("reg"):
                            got = fir_hip.fir2d_fixed(x, hq2, frac, acc, stage)
                        want = np.stack([co.fir2d(f, hq2, frac, acc, stage) for f in x])
                        _same(got, want, (R, C, stage, name))
                yield run
    # frames of 2^31 pixels keep the separable packed-16 form on fir2d_reg_kernel (fir2d.hip:189; smaller
    # ones take the strip kernel): one 32768 x 65536 frame made on the device, the rows at the top, at
    # the bottom and across strip seams compared with the oracle run on row bands of it (the shape and
    # the check of test_gpu_fir2d_ideal.py::test_fir2d_pk16_frame_past_2p31_pixels)
    for R in (3, 5):
        for C in (3, 5):
            for name in ("strip_unsigned", "strip_hi8", "strip_signed"):
                def huge(R=R, C=C, name=name):
                    import torch
                    from fir_hip import torch_ops
                    hq2, frac, acc = next(k[1:] for k in _fir2d_kernels(R, C) if k[0] == name)
                    H, W = 32768, 65536
                    xd = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=torch.device("cuda:0"))
                    with _env("reg"):
                        yd = torch_ops.fir2d_fixed_dev(xd, hq2, frac, acc, U8)
                    torch.cuda.synchronize()
                    co = _oracle()
                    for a, b in ((0, 40), (16000, 16070), (H - 40, H)):
                        lo, hi = max(a - 2, 0), min(b + 2, H)
                        want = co.fir2d(xd[lo:hi].cpu().numpy(), hq2, frac, acc, U8)[a - lo:a - lo + (b - a)]
                        _same(yd[a:b].cpu().numpy(), want, ("2^31 pixels", R, C, name, a, b))
                    del xd, yd
                yield huge


# ---- 128-bit sums (WIDE): taps of +-(2^31 - 1), enough of them that sum|h| * xmax reaches 2^63 -----
def _wide_taps(dtype, rng) -> np.ndarray:
    """needs_wide (fir1d.hip) looks at the taps alone: 2^17 + 9 of them for int16 samples, 2^24 + 2^17
    for u8.  The samples of a wide case are small, so every true sum stays inside 64 bits and the C
    oracle is exact."""
    L = (1 << 17) + 9 if np.dtype(dtype) == np.int16 else (1 << 24) + (1 << 17)
    return np.where(rng.integers(0, 2, L) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)


def _small(rng, shape, dtype):
    """Small samples; the u8 cases (2^24 taps each output) keep to one row of 40."""
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 4, (1, 40) if len(shape) == 2 else shape, dtype=np.uint8)
    return rng.integers(-100, 101, shape, dtype=np.int16)


def _wide_rows_cases():
    for dtype in (np.uint8, np.int16):
        for frac, acc, stage in ((30, 64, I32), (40, 80, U8)):
            def run(dtype=dtype, frac=frac, acc=acc, stage=stage):
                rng = np.random.default_rng(63)
                x, hq = _small(rng, (2, 150), dtype), _wide_taps(dtype, rng)
                _same(fir_hip.fir1d_fixed_rows(x, hq, frac, acc, stage), _oracle().fir1d_rows(x, hq, frac, acc, stage),
                      ("wide", np.dtype(dtype).name, stage))
            yield run


# ---- decimating, interpolating, resampling, complex-tap ---------------------------------------------
_RATE_CFG = [(np.uint8, 1), (np.int16, 1), (np.int16, 2)]


def _rate_taps(L: int) -> np.ndarray:
    h = np.random.default_rng(L).integers(-3000, 3001, L)
    h[0] |= 1
    return h


def decim_cases():
    """fir1d_decim_kernel<InT, STAGE, CH, LP, ODD>: the eight tap buckets (6 .. 127 taps: L + the
    parity tap fits the bucket) x even / odd rate x configuration x stage, rows of two workgroups
    and some; fir1d_decim_generic_kernel: 129 taps, and the 128-bit form."""
    import rate_property_cases as rc
    for dtype, ch in _RATE_CFG:
        for stage in (U8, I32):
            def run(dtype=dtype, ch=ch, stage=stage):
                rng = np.random.default_rng(ch)
                x = samples(rng, (2, 17000 * ch), dtype)
                for L in (6, 14, 22, 30, 46, 62, 94, 127, 129):
                    for D in (2, 3):
                        hq = _rate_taps(L)
                        got = fir_hip.fir1d_fixed_rows_decim(x, hq, D, 1, 12, 32, stage, channels=ch)
                        _same(got, rc.decim_want(x, hq, D, 1, 12, 32, stage, ch).reshape(2, -1), ("decim", L, D, ch, stage))
            yield run
            if ch == 1:
                def wide(dtype=dtype, stage=stage):
                    rng = np.random.default_rng(7)
                    x, hq = _small(rng, (2, 150), dtype), _wide_taps(dtype, rng)
                    got = fir_hip.fir1d_fixed_rows_decim(x, hq, 3, 2, 30, 64, stage)
                    _same(got, rc.decim_want(x, hq, 3, 2, 30, 64, stage, 1).reshape(x.shape[0], -1), ("decim wide", stage))
                yield wide


def interp_cases():
    """fir1d_interp_kernel<InT, STAGE, CH, NP>: tap counts across every pair bucket at U = 2 (and the
    short phases of U = 16) x configuration x stage; fir1d_interp_generic_kernel: 129 taps, and the
    128-bit form."""
    import rate_property_cases as rc
    for dtype, ch in _RATE_CFG:
        for stage in (U8, I32):
            def run(dtype=dtype, ch=ch, stage=stage):
                rng = np.random.default_rng(ch)
                x = samples(rng, (2, 8200 * ch), dtype)
                for U, Ls in ((2, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 19, 27, 35, 64, 67, 128, 129)), (16, (1, 16, 33, 48))):
                    for L in Ls:
                        hq = _rate_taps(L)
                        got = fir_hip.fir1d_fixed_rows_interp(x, hq, U, 12, 32, stage, channels=ch)
                        _same(got, rc.interp_want(x, hq, U, 12, 32, stage, ch), ("interp", L, U, ch, stage))
            yield run
            if ch == 1:
                def wide(dtype=dtype, stage=stage):
                    rng = np.random.default_rng(7)
                    x, hq = _small(rng, (2, 150), dtype), _wide_taps(dtype, rng)
                    _same(fir_hip.fir1d_fixed_rows_interp(x, hq, 2, 30, 64, stage), rc.interp_want(x, hq, 2, 30, 64, stage, 1),
                          ("interp wide", stage))
                yield wide


def resample_cases():
    """fir1d_resample_kernel<InT, STAGE, CH, NP>: tap counts across every pair bucket (up to 64 taps
    per phase) at 2/3 and 3/2 x configuration x stage; fir1d_resample_generic_kernel: 65 taps per
    phase, and the 128-bit form."""
    import rate_property_cases as rc
    for dtype, ch in _RATE_CFG:
        for stage in (U8, I32):
            def run(dtype=dtype, ch=ch, stage=stage):
                rng = np.random.default_rng(ch)
                x = samples(rng, (2, 8200 * ch), dtype)
                for U, D, Ls in ((2, 3, (1, 3, 7, 11, 15, 19, 27, 35, 45, 51, 70, 100, 127, 128, 131)), (3, 2, (1, 5, 20, 60, 190))):
                    for L in Ls:
                        hq = _rate_taps(L)
                        got = fir_hip.fir1d_fixed_rows_resample(x, hq, U, D, 1, 12, 32, stage, channels=ch)
                        _same(got, rc.resample_want(x, hq, U, D, 1, 12, 32, stage, ch), ("resample", L, U, D, ch, stage))
            yield run
            if ch == 1:
                def wide(dtype=dtype, stage=stage):
                    rng = np.random.default_rng(7)
                    x, hq = _small(rng, (2, 150), dtype), _wide_taps(dtype, rng)
                    got = fir_hip.fir1d_fixed_rows_resample(x, hq, 2, 3, 1, 30, 64, stage)
                    _same(got, rc.resample_want(x, hq, 2, 3, 1, 30, 64, stage, 1), ("resample wide", stage))
                yield wide


def cplx_cases():
    """fir1d_cplx_kernel<LP, ACC32>: the ten tap buckets x accumulator (32 bits, 24); the generic
    kernels: the u8 stage (packed 32-bit sums) and 40 accumulator bits, both stages, and the 128-bit
    form (2^16 + 9 complex taps of +-(2^31 - 1))."""
    import rate_property_cases as rc

    def taps(L, amp=3000):
        h = np.random.default_rng(L).integers(-amp, amp + 1, (L, 2))
        h[L // 2, 1] = 77  # never all real: not forwarded
        return h

    def run_fast():
        x = samples(np.random.default_rng(1), (3, 2 * (2 * 1024 + 4)), np.int16)
        for L in (2, 4, 6, 8, 12, 16, 24, 32, 48, 64):
            for frac, acc in ((12, 32), (16, 24)):
                _same(fir_hip.fir1d_fixed_rows_cplx(x, taps(L), frac, acc, I32), rc.cplx_want(x, taps(L), frac, acc, I32),
                      ("cplx", L, acc))
    yield run_fast

    def run_generic():
        x = samples(np.random.default_rng(2), (3, 2 * 700), np.int16)
        for stage in (U8, I32):
            for frac, acc in ((12, 32), (20, 40)):
                L = 9 if stage == U8 else 70  # the fast kernel takes neither the u8 stage nor 70 taps
                _same(fir_hip.fir1d_fixed_rows_cplx(x, taps(L), frac, acc, stage), rc.cplx_want(x, taps(L), frac, acc, stage),
                      ("cplx generic", stage, acc))
    yield run_generic

    def run_wide():
        rng = np.random.default_rng(3)
        L = (1 << 16) + 9
        hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
        x = rng.integers(-50, 51, (2, 2 * 150), dtype=np.int16)
        for frac, acc, stage in ((30, 64, I32), (40, 80, U8)):
            _same(fir_hip.fir1d_fixed_rows_cplx(x, hq, frac, acc, stage), rc.cplx_want(x, hq, frac, acc, stage), ("cplx wide", stage))
    yield run_wide


# ---- shard edges, the halo gate -------------------------------------------------------------------
def edges_cases():
    """fir1d_edges_kernel<InT, STAGE, WIDE = false>: a ragged shard (rows dispatch, then the edges
    redone from both halos) x sample type x stage."""
    for dtype in (np.uint8, np.int16):
        for stage in (U8, I32):
            def run(dtype=dtype, stage=stage):
                import torch
                from fir_hip import torch_ops
                dev = torch.device("cuda:0")
                rng = np.random.default_rng(9)
                L = 31
                hq = rng.integers(-3000, 3001, L)
                x, hl, hr = samples(rng, (5003,), dtype), samples(rng, (L - 1 - L // 2,), dtype), samples(rng, (L // 2,), dtype)
                td = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
                y = torch_ops.fir1d_fixed_segment_dev(td(x), hq, td(hl), td(hr), 12, 32, stage)
                torch.cuda.synchronize()
                _same(y.cpu().numpy(), _oracle().fir1d_rows(x, hq, 12, 32, stage, halo_left=hl, halo_right=hr), ("edges", stage))
            yield run
    for stage in (U8, I32):  # the 128-bit form, int16: a shard one sample longer than its halos
        def wide(stage=stage):
            import torch
            from fir_hip import torch_ops
            dev = torch.device("cuda:0")
            rng = np.random.default_rng(11)
            hq = _wide_taps(np.int16, rng)
            L = len(hq)
            x, hl, hr = _small(rng, (L + 20,), np.int16), _small(rng, (L - 1 - L // 2,), np.int16), _small(rng, (L // 2,), np.int16)
            td = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            y = torch_ops.fir1d_fixed_segment_dev(td(x), hq, td(hl), td(hr), 30, 64, stage)
            torch.cuda.synchronize()
            _same(y.cpu().numpy(), _oracle().fir1d_rows(x, hq, 30, 64, stage, halo_left=hl, halo_right=hr), ("edges wide", stage))
        yield wide


def halo_cases():
    """halo_mailbox_init_kernel and halo_gate_kernel on one device: a ring of one (the segment is its
    own left and right neighbour), two epochs."""
    def run():
        import torch
        from fir_hip import torch_ops
        dev = torch.device("cuda:0")
        hl, hr = 3, 2  # int16 samples
        mb = torch.empty(fir_hip.halo_mailbox_bytes(2 * hl, 2 * hr), dtype=torch.uint8, device=dev)
        torch_ops.halo_mailbox_init_dev(mb, 2 * hl, 2 * hr)
        seg = torch.arange(1000, dtype=torch.int16, device=dev)
        left = torch.empty(hl, dtype=torch.int16, device=dev)
        right = torch.empty(hr, dtype=torch.int16, device=dev)
        st = torch.full((1,), -1, dtype=torch.int32, device=dev)
        for step in range(2):
            seg.add_(step + 5)
            torch.cuda.synchronize()
            torch_ops.halo_gate_dev(seg, 2 * hl, 2 * hr, mb, mb.data_ptr(), mb.data_ptr(), left, right, st, 5.0)
            torch.cuda.synchronize()
            assert st.item() == 0, step
            assert torch.equal(left, seg[-hl:]) and torch.equal(right, seg[:hr]), step
    yield run


# ---- the other 2-D kernels ---------------------------------------------------------------------------
def fir2d_mfma_cases():
    """fir2d_mfma_kernel<R, NP, FAST, ACC32>: 3 and 5 tap rows x one / two tap planes x the three
    accumulator forms, under FIR2D_PATH=mfma."""
    def run():
        co = _oracle()
        rng = np.random.default_rng(4)
        x = samples(rng, (2, 35, 2 * 1024 + 16), np.uint8)
        for R in (3, 5):
            byte = rng.integers(-9, 10, (R, R))
            byte[0, 0], byte[-1, -1], byte[0, -1] = 100, -9, 7
            byte = byte * 256  # one plane: the taps over their common power of two fit a byte
            two = rng.integers(-12000, 12001, (R, R))
            two[0, 0], two[-1, -1] = 32639, -32768
            for hq2 in (byte, two):
                # FAST (no wrap, frac <= 16, the sum shifted to bit 16 below 2^31); 32 bits with frac
                # past 16; 24 bits that wrap (plan_mfma2, fir2d_mfma.hip)
                for frac, acc in ((12, 32), (24, 32), (16, 24)):
                    with _env("mfma"):
                        got = fir_hip.fir2d_fixed(x, hq2, frac, acc, U8)
                    _same(got, np.stack([co.fir2d(f, hq2, frac, acc, U8) for f in x]), ("fir2d mfma", R, int(hq2[0, 0]), frac, acc))
    yield run


def fir2d_generic_cases():
    """fir2d_generic_kernel<STAGE, WIDE>: a 7 x 7 kernel (no register or matrix-core form) x stage; the
    128-bit form: 4096 x 4113 taps of 2^31 - 1 over an all-255 3 x 5 frame, every output the same exact sum."""
    def run():
        co = _oracle()
        rng = np.random.default_rng(5)
        x, hq2 = samples(rng, (2, 35, 1040), np.uint8), rng.integers(-800, 801, (7, 7))
        for stage in (U8, I32):
            _same(fir_hip.fir2d_fixed(x, hq2, 12, 32, stage), np.stack([co.fir2d(f, hq2, 12, 32, stage) for f in x]), ("7x7", stage))
    yield run

    def wide():
        img = np.full((3, 5), 255, np.uint8)
        k2 = np.full((1 << 12, 4113), (1 << 31) - 1, np.int64)  # 255 * sum|h| >= 2^63 takes 16 843 010 such taps
        ssum = 15 * 255 * ((1 << 31) - 1)  # every output sees the whole frame under taps of one value
        q = ((ssum + (1 << 11)) >> 12) & 0xFFFFFFFF
        want32 = q - (1 << 32) if q >= (1 << 31) else q
        _same(fir_hip.fir2d_fixed(img, k2, 12, 100, I32), np.full((3, 5), want32, np.int32), "2-D wide i32")
        _same(fir_hip.fir2d_fixed(img, k2, 40, 100, U8), np.full((3, 5), min(255, (ssum + (1 << 39)) >> 40), np.uint8), "2-D wide u8")
    yield wide


# ---- float64 ideal models, metrics, restore ----------------------------------------------------------
def _same_bits(got, want, tag) -> None:
    """float64 outputs compared as their bytes (the order of the additions is part of the contract)."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    _same(got.view(np.uint64), want.view(np.uint64), tag)


def ideal_cases():
    """fir1d_ideal_reg_kernel<L> for L = 1..9 and the LDS form fir1d_ideal_kernel (11 taps; and three
    taps over rows of a width that is no whole dword, which the register form refuses)."""
    for L, shape in [(L, (3, 2 * 1024 + 4)) for L in range(1, 10)] + [(11, (3, 2 * 1024 + 4)), (3, (3, 2 * 1024 + 5))]:
        def run(L=L, shape=shape):
            rng = np.random.default_rng(L)
            x, h = samples(rng, shape, np.uint8), rng.standard_normal(L)
            _same_bits(fir_hip.fir1d_ideal_rows(x, h), _oracle().fir1d_ideal_rows(x, h), (L, shape))
        yield run


def ideal2d_cases():
    """fir2d_ideal_reg_kernel<R, C> for R, C = 1..5 (35 x 2052: two 16-row strips and two 1024-pixel
    tiles and some) and fir2d_ideal_generic_kernel (7 x 3 taps), against tests/ideal2d_ref.py."""
    from ideal2d_ref import ideal2d
    for R, C in [(r, c) for r in range(1, 6) for c in range(1, 6)] + [(7, 3)]:
        def run(R=R, C=C):
            rng = np.random.default_rng(R * 10 + C)
            x, h = samples(rng, (35, 2052), np.uint8), rng.standard_normal((R, C))
            _same_bits(fir_hip.fir2d_ideal(x, h), ideal2d(x, h), (R, C))
        yield run


def metrics_cases():
    """The metrics kernels over every fixed dtype: the one-pass u8 form (aligned, a full 8192-sample
    block), metrics_blocks_any<T> / metrics_ragged<T> for the others, NumPy's sums as the reference."""
    from conftest import same_metrics
    from oracle import fir_oracle as fo
    for dt in fir_hip.METRIC_DTYPES:
        for n in (2 * 8192 + 129, 100):
            def run(dt=dt, n=n):
                rng = np.random.default_rng(n + dt.itemsize)
                yi = rng.uniform(-64.0, 320.0, n)
                yf = np.rint(yi) + rng.integers(-3, 4, n)
                yf = (np.clip(yf, 0, 255) if dt.kind == "u" else np.clip(yf, -128, 127) if dt == np.int8 else yf).astype(dt)
                got, want = fir_hip.compare_metrics(yi, yf), fo.compute_metrics(yi, yf)
                bad = same_metrics(got, want)
                assert not bad, (dt, n, {k: (got[k], want[k]) for k in bad})
            yield run

    def off16():  # u8 one byte off 16 on the device: the per-part metrics_blocks instead of the one pass
        import torch
        from fir_hip import torch_ops
        rng = np.random.default_rng(5)
        n = 2 * 8192 + 129
        yi = rng.uniform(-64.0, 320.0, n)
        yf = np.clip(np.rint(yi) + rng.integers(-3, 4, n), 0, 255).astype(np.uint8)
        dev = torch.device("cuda:0")
        fd = torch.empty(n + 1, dtype=torch.uint8, device=dev)[1:]
        fd.copy_(torch.from_numpy(yf))
        out = torch_ops.compare_metrics_dev(torch.from_numpy(yi).to(dev), fd)
        torch.cuda.synchronize()
        got, want = fir_hip.metrics_from_sums(out.cpu().numpy(), n), fo.compute_metrics(yi, yf)
        bad = same_metrics(got, want)
        assert not bad, ("u8 off 16", {k: (got[k], want[k]) for k in bad})
    yield off16


def restore_cases():
    """restore_map_kernel<false> (clip) and min / max, parameters, restore_map_kernel<true> (normalize)."""
    from oracle import fir_oracle as fo
    for policy, ref in ((fir_hip.RESTORE_CLIP, fo.to_u8_clip), (fir_hip.RESTORE_NORMALIZE, fo.to_u8_normalized)):
        def run(policy=policy, ref=ref):
            rng = np.random.default_rng(policy)
            a = rng.uniform(-80.0, 340.0, 3 * 4096 + 5)
            a[::50] = np.round(a[::50]) + 0.5  # ties
            _same(fir_hip.restore_u8(a, policy), ref(a), ("restore", policy))
        yield run


_CASES = {
    "decim": decim_cases, "interp": interp_cases, "resample": resample_cases, "cplx": cplx_cases, "edges": edges_cases,
    "halo": halo_cases, "fir2d_mfma": fir2d_mfma_cases, "fir2d_generic": fir2d_generic_cases,
    "fir2d_reg": fir2d_reg_cases, "fir2d_pk16": fir2d_reg_cases,
    "ideal": ideal_cases, "ideal2d": ideal2d_cases, "metrics": metrics_cases, "restore": restore_cases,
    "batch": batch_cases, "mfma_step": mfma_step_cases, "mfma_long": mfma_long_cases, "mfma_run": mfma_run_cases,
    "lds": lds_cases, "generic": generic_cases,
}
GENERATED = ["reg_" + c for c in REG_CONFIGS] + sorted(_CASES)  # the families that have a generator


def cases(family: str):
    if family.startswith("reg_"):
        return reg_cases(family[4:])
    return _CASES[family]()
