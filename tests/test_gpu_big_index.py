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

Measured on an MI355X: every case passes, none skips; the module alone takes 12 s, most cases 0.02
to 0.07 s and the slowest 2 to 5 s (which ones varies from run to run: allocation, not the kernel).  With ``(uint32_t)g0 % rowlen32`` made a signed cast in
fir1d_reg.h and ideal_reg.h, rows_u8_reg_last, bank4_u8_rows and ideal_rows fail (the first
differing output at byte offsets 0xffc0effe, 0x80000ffe and 0x400007ff0) and their twins pass.
"""
from __future__ import annotations

import pytest
import torch

import big_index_cases as bic
import fir_hip
from fir_hip import torch_cplx, torch_interp, torch_ops, torch_resample

DEV = torch.device("cuda:0")
TABLE = bic.table(bic.FULL)
HEADROOM = 2 * bic.GIB


def _launch(c, x, y):
    h = bic.taps_of(c)
    a = (bic.FRAC, bic.ACC, c.stage)
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
    x = y = found = None
    try:
        x = bic.make_x(c, DEV)
        y = bic.make_y(c, DEV)
        want = bic.dispatch_kernel(c, x.data_ptr(), y.data_ptr())
        assert c.kernel in (None, want), (c.kernel, want)
        with fir_hip.launch_log() as log:
            out = _launch(c, x, y)
        torch.cuda.synchronize()
        assert out is y
        assert [l.kernel for l in log] == [want], (want, [l.inst for l in log])
        print(f"\n{c.name}: {log[0].inst} grid {log[0].grid}; {c.in_elems} -> {c.out_elems} elements, "
              f"footprint {c.footprint / bic.GIB:.2f} GiB")
        try:
            bic.verify(c, x, y)
        except bic.Mismatch as e:  # its traceback holds x and y: keep the words, let the tensors go
            found = str(e)
    finally:
        del x, y
        torch.cuda.empty_cache()
    assert found is None, found
