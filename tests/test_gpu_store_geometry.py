"""The int16 -> int32 register kernel around the seams of a block's span.

fir1d_reg_kernel stages a wave's int32 rows through LDS and writes them as whole 1 KiB store
instructions.  Its int16 -> int32 instantiations run blocks of REG_BLOCK = 128 threads (kRegBlock,
csrc/fir1d_reg_impl.h), so a block covers a span of S = REG_BLOCK / 64 * 512 = 1024 int16 samples and
writes 4 KiB; every other configuration keeps 256 threads.  The grid, the LDS row buffer and the tile
a wave takes all follow the block size, and a wrong one shows at multiples of S and of the 512-sample
wave tile: in the last block's spare waves, in a partial tile, in a partial vector.  So the shapes
here sit on and one off those seams.  Every case:

* runs through the device entries on a guarded input into a guarded, canary-filled output
  (tests/guarded.py): canaries intact, input unchanged;
* compares every output bit for bit with ``oracle.c_oracle().fir1d_rows``;
* names, through ``fir_hip.launch_log()``, the instantiation it launched: sample type, stage, taps,
  channels, chunks per wave, the flags that name a form, the block size and the grid that goes with it.

Samples are full-range with runs of the extremes (census_cases.samples).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
from census_cases import samples
from fir_hip import torch_ops
from guarded import guarded_input, guarded_output
from oracle import c_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
REG_BLOCK = 128            # threads per block of the int16 -> int32 register kernels (kRegBlock)
S = REG_BLOCK // 64 * 512  # int16 samples of a block's span
SHARPEN5 = (-256, -1024, 6656, -1024, -256)
# every product of a full-range sample with these passes 2^30, so sums of five wrap 32 bits
WRAP5 = (-32768, 32767, -32768, 32767, -32768)
_CT = {np.dtype(np.uint8): "unsigned char", np.dtype(np.int16): "short"}
_FORM = frozenset({"kDot2", "kU8Dot2", "kAcc32", "kRagged", "kMasked", "kHalo"})


def _taps(L: int) -> np.ndarray:
    h = np.random.default_rng(L).integers(-3000, 3001, L)
    h[L // 2] |= 1
    return h


def _launched(log, x, stage, L, ch, U, form, tag):
    """One launch, of fir1d_reg_kernel<type, stage, L, ch, U, flags, 1, block> with the form flags `form`,
    at the block size of its configuration and the grid that covers the buffer's tiles with it."""
    assert [l.kernel for l in log] == ["fir1d_reg_kernel"], (tag, [l.inst for l in log])
    l = log[0]
    assert l.targs[:5] == (_CT[x.dtype], str(stage), str(L), str(ch), str(U)) and l.targs[6] == "1", (tag, l.inst)
    assert {"kCoal", "kNtStore", "kEdgeDword"} <= l.flags and l.flags & _FORM == set(form), (tag, sorted(l.flags))
    block = REG_BLOCK if x.dtype == np.int16 and stage == I32 else 256
    vec = 8 if x.dtype == np.int16 else 16
    up = lambda a, b: (a + b - 1) // b  # noqa: E731
    assert l.targs[7] == str(block) and l.block == (block, 1, 1), (tag, l.inst, l.block)
    assert l.grid == (up(up(up(x.size, vec), 64 * U), block // 64), 1, 1), (tag, l.grid, x.size)


def _run(x, hq, stage=I32, ch=1, U=1, form=("kDot2", "kAcc32", "kMasked"), halos=None, tag=()):
    tag = (x.shape, len(hq), ch) + tuple(tag)
    xg = guarded_input(torch.from_numpy(x), device=DEV)
    y, check = guarded_output(x.shape, torch.int32 if stage == I32 else torch.uint8, device=DEV)
    with fir_hip.launch_log() as log:
        if halos is None:
            torch_ops.fir1d_fixed_rows_dev(xg, hq, 12, 32, stage, ch, out=y)
            want = c_oracle().fir1d_rows(x, hq, 12, 32, stage, channels=ch)
        else:
            hl, hr = halos
            g = [None if h is None else guarded_input(torch.from_numpy(h), device=DEV) for h in halos]
            torch_ops.fir1d_fixed_segment_dev(xg, hq, g[0], g[1], 12, 32, stage, ch, out=y)
            want = c_oracle().fir1d_rows(x, hq, 12, 32, stage, channels=ch, halo_left=hl, halo_right=hr)
    torch.cuda.synchronize()
    _launched(log, x, stage, len(hq), ch, U, form, tag)
    got = y.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{tag}: {bad.size} of {want.size} outputs differ from the oracle; the first at flat index "
                             f"{bad[0]} (span {bad[0] // S}, offset {bad[0] % S}): {got.reshape(-1)[bad[0]]} != "
                             f"{want.reshape(-1)[bad[0]]}")
    check(str(tag))
    assert torch.equal(xg.cpu(), torch.from_numpy(x)), tag  # the input is only read


ONE_ROW = [S - 1, S, S + 1, S + 511, S + 512, S + 513, 2 * S - 1, 2 * S, 3 * S + 8, 8 * S + 3]


@pytest.mark.parametrize("n", ONE_ROW)
@pytest.mark.parametrize("name,hq", [("sharpen", SHARPEN5), ("wrap", WRAP5)])
def test_one_row(name, hq, n):
    """A full span, a span and a partial tile, a partial vector, nothing but a tail."""
    _run(samples(np.random.default_rng(n), (n,), np.int16), hq, tag=(name,))


@pytest.mark.parametrize("L", [1, 2, 3, 5, 6, 9])
def test_tap_counts(L):
    """One halo dword per side up to 5 taps (one wave-wide edge load); 6 and 9 taps need two per side
    (the lane-masked 16-byte edge loads)."""
    _run(samples(np.random.default_rng(L), (2 * S + 8,), np.int16), _taps(L))


@pytest.mark.parametrize("shape", [(3, 1000), (5, S + 8), (2, 2 * S)], ids=str)
def test_whole_vector_rows_across_spans(shape):
    """Row edges inside spans: the halo dwords of the lanes at a row edge are zeroed."""
    _run(samples(np.random.default_rng(shape[1]), shape, np.int16), _taps(5))


def test_ragged_rows():
    """Rows that straddle vectors: the masked pair."""
    _run(samples(np.random.default_rng(7), (3, 1001), np.int16), _taps(5))


@pytest.mark.parametrize("n", [S // 2, S // 2 + 1, S + 4])
def test_two_channels(n):
    """n complex samples, 3 taps: the two-channel kernel (mad24, two samples of halo = one dword)."""
    _run(samples(np.random.default_rng(n), (2 * n,), np.int16), _taps(3), ch=2, form=("kAcc32", "kMasked"))


def test_u8_to_int32():
    """u8 samples, four chunks per wave: the int32 stage at 256 threads per block."""
    _run(samples(np.random.default_rng(8), (4 * 4096 + 3,), np.uint8), _taps(5), U=4, form=("kU8Dot2",))


@pytest.mark.parametrize("which", ["both", "left", "right"])
@pytest.mark.parametrize("n", sorted({512, 1536, S, S + 512}))
def test_segments_with_halos(n, which):
    """Whole tiles with halos in place of the zero padding (the kHalo instantiation)."""
    rng = np.random.default_rng(n)
    x, hl, hr = samples(rng, (n,), np.int16), samples(rng, (2,), np.int16), samples(rng, (2,), np.int16)
    halos = (hl if which != "right" else None, hr if which != "left" else None)
    _run(x, _taps(5), form=("kDot2", "kAcc32", "kMasked", "kHalo"), halos=halos, tag=(which,))
