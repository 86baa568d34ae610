"""GPU: the 1-D kernels where sample and byte offsets pass 2^31 and 2^32 (tests/big_index_cases.py).

Every case of ``table(FULL)`` is the smallest call whose input or output crosses the threshold it
names (element index 2^31 or 2^32, byte offset 2^31 .. 2^34), each followed by its twin at offset 0
(2 P frames, or 2 Q rows) through the same code, so a failure separates "large" from "wrong".  The
input is periodic with a prime period, built on the device; a case

1. fills y with the 0x5A sentinel and runs the device-tensor entry once under fir_hip.launch_log();
2. asserts the one kernel csrc's dispatch conditions prescribe (``dispatch_kernel``, held to the
   table's intent without a GPU by tests/test_big_index_cases.py);
3. compares, on the device and in chunks of 2^28 elements, every interior period of y with period 1
   (every row with row r % Q);
4. copies back periods 0-1, the last two periods and the ragged tail (rows 0 .. Q-1 and the last Q
   rows) and compares them bit for bit with c_oracle().fir1d_rows, fir1d_ideal_rows, rate_property_cases'
   decim_want / interp_want / resample_want and cplx_ref.want on the matching slice of x.

A case holds at most 24 GiB (x, y, 1 GiB of compare temporaries) and frees them before the next;
with less than its footprint plus 2 GiB free it skips, naming both numbers.  No case provokes a
fault: every buffer is in bounds and every size is one the entries accept.

Left out: the ``total = 2^32`` edge of ideal.hip's multi-row register test (the first size off
fir1d_ideal_reg_kernel) needs a 32 GiB float64 output, past the cap; the fixed-point twin of that
bound (reg_path_ok, rows_u8_reg_last / rows_u8_reg_first_off) is here.  The issue's 65-tap int16
case runs the step kernel (65 taps are its last length); fixed_i16_long66 is the chunked kernel's.

The four complex-rate extension libraries (families cdecim, cinterp, cresample, cstream: 18 large
cases and their twins) write nothing to the launch log.  For them step 2 asserts three things equal
-- the family's ``predicted_route`` (tests/c*_cases.py), the library's ``route`` query and
``last_launch()`` after the call -- and that this (route, bucket) is the one the case was built for
("cdecim:FAST/12").  A cstream case is one block behind a hostile history, hist_out between
canaries (tests/guarded.py): y is checked as everywhere, hist_out bit for bit against the last
taps - 1 frames of every row of x.

Measured on an MI355X: every case passes, none skips; the module alone takes 12 s, most cases 0.02
to 0.07 s and the slowest 2 to 5 s (which ones varies from run to run: allocation, not the kernel).  With ``(uint32_t)g0 % rowlen32`` made a signed cast in
fir1d_reg.h and ideal_reg.h, rows_u8_reg_last, bank4_u8_rows and ideal_rows fail (the first
differing output at byte offsets 0xffc0effe, 0x80000ffe and 0x400007ff0) and their twins pass.

With the complex-rate families (98 cases instead of 62): every case passes, none skips; the module
alone takes 28 s, of which the 62 earlier cases take 12 s as before; most new cases take 0.02 to 0.5 s
and the slowest 3 to 4 s (cdecim_D2_fast, cstream_D2_generic32, cinterp_U2_fast in one run,
cstream_D2_fast, cinterp_rows_fast, cdecim_D2_g64 in another: again allocation, not the kernel).
Mutations, each run once in a scratch copy: the row offset ``r * width`` of fir1d_cplx_decim.hip's
fast kernel and the output offset ``r * out_width + ig * U`` of fir1d_cplx_interp.hip's through a
``(uint32_t)`` cast change nothing, and cdecim_rows_fast and cinterp_rows_fast pass: both are frame
indices that pass 2^31 here and stay below 2^32 (the footprint cap keeps a row form from reaching
2^32 frames), so the cast is still exact.  Truncated to 31 bits instead (``& 0x7FFFFFFF``, the
unsigned image of a 32-bit signed index: a smaller non-negative index, in bounds), cdecim_rows_fast
fails (rows 2^19 and up read rows 0 .. 2; the first differing output at byte offset 0x155400000)
and cinterp_rows_fast fails (the last rows written over rows 0 .. 2; the first at byte offset 0x0),
and both twins pass.
"""
from __future__ import annotations

import pytest
import torch

import big_index_cases as bic
import fir_hip
from fir_hip import torch_cdecim, torch_cinterp, torch_cplx, torch_cresample, torch_cstream, torch_interp, torch_ops, torch_resample
from guarded import guarded_output

DEV = torch.device("cuda:0")
TABLE = bic.table(bic.FULL)
HEADROOM = 2 * bic.GIB


def _launch(c, x, y, hist_in=None, hist_out=None):
    h = bic.taps_of(c)
    a = (bic.FRAC, bic.ACC, c.stage)
    if c.family == "cdecim":
        return torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(x, h, c.decim, c.phase, *a, out=y)
    if c.family == "cinterp":
        return torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(x, h, c.up, *a, out=y)
    if c.family == "cresample":
        return torch_cresample.fir1d_fixed_rows_cplx_resample_dev(x, h, c.up, c.decim, c.phase, *a, out=y)
    if c.family == "cstream":
        return torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(x, hist_in, hist_out, h, c.decim, c.phase, *a, out=y)
    if c.family == "fixed":
        return torch_ops.fir1d_fixed_rows_dev(x, h, *a, c.ch, out=y)
    if c.family == "bank":
        return torch_ops.fir1d_fixed_rows_multi_dev(x, h, *a, c.ch, out=y)
    if c.family == "ideal":
        return torch_ops.fir1d_ideal_rows_dev(x, h, out=y)
    if c.family == "decim":
        return torch_ops.fir1d_fixed_rows_decim_dev(x, h, c.decim, c.phase, *a, c.ch, out=y)
    if c.family == "interp":
        return torch_interp.fir1d_fixed_rows_interp_dev(x, h, c.up, *a, c.ch, out=y)
    if c.family == "resample":
        return torch_resample.fir1d_fixed_rows_resample_dev(x, h, c.up, c.decim, c.phase, *a, c.ch, out=y)
    return torch_cplx.fir1d_fixed_rows_cplx_dev(x, h, *a, out=y)


@pytest.mark.parametrize("c", TABLE, ids=[c.name for c in TABLE])
def test_big_index(c):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < c.footprint + HEADROOM:
        pytest.skip(f"{c.name} needs {c.footprint + HEADROOM} bytes free on the device ({c.footprint} + 2 GiB), {free} are")
    x = y = hist_in = hist_out = found = None
    hist_guards = None
    try:
        x = bic.make_x(c, DEV)
        y = bic.make_y(c, DEV)
        if c.hist_frames:  # a stream's block: a hostile history before it, hist_out between canaries
            hist_in = bic.make_hist(c, DEV)
            hist_out, hist_guards = guarded_output(tuple(hist_in.shape), torch.int16, device=DEV)
        hist_ptrs = (hist_in.data_ptr(), hist_out.data_ptr()) if c.hist_frames else ()
        want = bic.dispatch_kernel(c, x.data_ptr(), y.data_ptr(), *hist_ptrs)
        assert c.kernel in (None, want), (c.kernel, want)
        if c.family in bic.CEXT:  # no launch log: predicted route == the library's route query == what was launched
            lib = bic.CEXT[c.family][0]
            asked = lib.route(*bic.cext_addrs(c, x.data_ptr(), y.data_ptr(), *hist_ptrs), c.rows, c.width, bic.taps_of(c),
                              *bic.rate_args(c), bic.FRAC, bic.ACC, c.stage)
            assert bic.route_name(c.family, asked) == want, (asked, want)
            out = _launch(c, x, y, hist_in, hist_out)
            launched = bic.route_name(c.family, lib.last_launch())
            torch.cuda.synchronize()
            assert out is y
            assert launched == want, (launched, want)
            what = launched
        else:
            with fir_hip.launch_log() as log:
                out = _launch(c, x, y)
            torch.cuda.synchronize()
            assert out is y
            assert [l.kernel for l in log] == [want], (want, [l.inst for l in log])
            what = f"{log[0].inst} grid {log[0].grid}"
        print(f"\n{c.name}: {what}; {c.in_elems} -> {c.out_elems} elements, footprint {c.footprint / bic.GIB:.2f} GiB")
        try:
            bic.verify(c, x, y, hist_out=hist_out)
        except bic.Mismatch as e:  # its traceback holds x and y: keep the words, let the tensors go
            found = str(e)
        if hist_guards is not None:
            hist_guards(f"{c.name} hist_out")
    finally:
        del x, y, hist_in, hist_out, hist_guards
        torch.cuda.empty_cache()
    assert found is None, found
