"""The PARTS form of csrc/metrics.hip past one part and one sweep, and the raw sums of both forms.

launch_metrics_t serves aligned u8 with a full block in one launch (metrics_prep +
metrics_leaf_kernel: the pipeline's case, tested from 1 to 4500 blocks elsewhere) and every other
call -- u8 off 16 bytes, the ten other dtypes -- in parts of 8192 blocks (the last 2048, at most
16), the chain of part k - 1 running as workgroup 0 of launch k and carrying the sums through
state[].  Before this module no test ran that form with more than three full blocks: no second
part, no in-launch chain, no state[] carry, no full chain group, no second grid-stride iteration
of a wave.  Everything here goes through torch_ops.compare_metrics_dev with ``out`` and ``work``
(exactly fir_metrics_work_bytes(n)) inside guard bands, the inputs at chosen addresses between
hostile bytes, and asserts per call, in this order: (1) the launch log equals
metrics_cases.launches_of on the real pointers (kernel, template argument, grid.x); (2) out[0..7]
equals the NumPy reference BIT FOR BIT (the raw sums, not the report's sum / n and sqrt, which
hide a last-bit error in 10 % and 46 % of cases) and out[8] == 0; (3) both guard bands intact.

* ``test_pinned``: the seven sizes of metrics_cases.ROWS (what each reaches is printed with -s and
  listed in DESIGN.md) through metrics_blocks (u8, fixed one byte off 16) and
  metrics_blocks_any<short>, the four up to 4097 blocks also through metrics_blocks_any<double>
  and metrics_blocks with the IDEAL 8 bytes off.  The data is a 509-block pattern tiled on the
  device; the reference is NumPy on the materialised array, the periodic chain, or both.  Each case
  is followed by its twin, the same data as aligned u8 through the one-launch form, so a failure
  says whether the form or the data / reference is at fault.
* ``test_byte_pairs``: all 65,536 ordered byte pairs (and shifted by one byte, every pair across a
  dword edge) through the one-launch form's four-bytes-at-once zero / 255 counts, and through
  metrics_blocks.
* ``test_forms_property``: hypothesis, derandomized, the route drawn first (leaf, parts:u8 by
  either pointer, parts:any of every dtype, ragged_only, empty), 0 to 40 blocks, the ragged
  lengths on both sides of every leaf and split edge, four kinds of fill; one pinned example per
  route and dtype runs whatever is drawn.  No non-finite values (tests/test_gpu_nonfinite.py).

The 16-part row holds 8.2 GB of float64 plus the fixed array and its twin's; with less than its
footprint plus 2 GiB free it skips, naming both numbers.  No case touches memory outside its
buffers; every size is one the entry accepts.

Measured on an idle MI355X: all 27 tests pass, none skips; the module alone takes 4.4 s.  The
slowest: test_forms_property 0.9 s (430 calls), the first pinned case 0.7 s (it makes the pattern
and its block sums), the 4097-block rows' first case 0.2 s (NumPy over 33.6 M samples, once per
row); every other case under 0.15 s, the 16-part rows about 10 ms each (8.2 GB tiled and two calls).

Sensitivity, two local builds that change values and no address (not committed), pinned rows only:
(a) chain_range starting every part from 0.0 instead of state[wv]: all 18 cases of the six rows
    with two or more parts fail on out[1..3] (2049 + 1: sum d -0x1.2010f81da614ep+34 against
    -0x1.9563c264296efp+34) while every twin passes; the one-part row and the byte pairs pass.
(b) bounds[] filled in forward order (the 2048-block part first): the 10 cases of rows 2049 + 1,
    2561 + 129 and 10241 + 7 fail on the launch log (grids 512, 2 against 1, 513), their twins
    pass.  out[1..3] is unchanged in every row, and cannot change: whatever the partition, the
    chains run over the blocks in order, so the order of the part sizes decides only which chain
    is exposed (speed), and the launch-log assertion is what holds it.  Rows whose parts all take
    512 workgroups either way (4097, 10240, 124929 blocks) do not see (b).
"""
from __future__ import annotations

import functools
import time
from collections import Counter

import numpy as np
import pytest
import torch
from hypothesis import example, given, settings

import fir_hip
import metrics_cases as mc
from fir_hip import torch_ops
from guarded import GUARD_MIN, guarded_input, guarded_output
from test_gpu_property import SETTINGS

DEV = torch.device("cuda:0")
HEADROOM = 2 << 30
TORCH_DT = {"bool": torch.bool, "uint8": torch.uint8, "int8": torch.int8, "uint16": torch.uint16, "int16": torch.int16,
            "uint32": torch.uint32, "int32": torch.int32, "uint64": torch.uint64, "int64": torch.int64,
            "float16": torch.float16, "float32": torch.float32, "float64": torch.float64}
NP_NAME = {v: k for k, v in TORCH_DT.items()}


def _check(ideal, fixed, refs) -> list:
    """One call; what fails of (1) launches, (2) out[0..7] and out[8], (3) guard bands, in that order."""
    n = ideal.numel()
    out, check_out = guarded_output((9,), torch.float64, device=DEV)
    work, check_work = guarded_output((int(fir_hip.lib().fir_metrics_work_bytes(n)),), torch.uint8, device=DEV)
    with fir_hip.launch_log() as log:
        ret = torch_ops.compare_metrics_dev(ideal, fixed, out=out, work=work)
    torch.cuda.synchronize()
    bad = []
    got = [(l.kernel, l.targs, l.grid[0]) for l in log]
    want = mc.launches_of(n, NP_NAME[fixed.dtype], ideal.data_ptr(), fixed.data_ptr())
    if got != want or ret is not out:
        bad.append(f"launches {got}, want {want}")
    s = out.cpu().numpy()
    for how, ref in refs:
        if mc.differing(s[:8], ref):
            bad.append(f"against {how}: {mc.describe(s[:8], ref)}")
    if not s[8] == 0.0:
        bad.append(f"out[8] = {s[8]!r}")
    for check, what in ((check_out, "out"), (check_work, "work")):
        try:
            check(what)
        except AssertionError as e:
            bad.append(str(e))
    return bad


# ---- the pinned sizes ------------------------------------------------------------------------------
def _slab(nbytes: int, lead: int) -> torch.Tensor:
    """nbytes at `lead` bytes past a 512-byte boundary inside one allocation, 64 KiB of 0xFF on each
    side (NaN as a float, 255 as u8, -1 as an integer): only the guards are filled."""
    buf = torch.empty(512 + GUARD_MIN + 512 + nbytes + GUARD_MIN, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 512 + GUARD_MIN + lead
    buf[:start].fill_(0xFF)
    buf[start + nbytes:].fill_(0xFF)
    return buf[start:start + nbytes]


@functools.lru_cache(maxsize=None)
def _pattern_dev(what: str) -> torch.Tensor:
    yi, yf = mc.pattern()
    return torch.from_numpy(np.array(yi) if what == "ideal" else yf.astype(what)).to(DEV)


def _tiled(what: str, n: int, lead: int) -> torch.Tensor:
    """The pattern tiled to n samples on the device at the given lead (no host array of n)."""
    pat = _pattern_dev(what)
    dst = _slab(n * pat.element_size(), lead).view(pat.dtype)
    full = n // pat.numel()
    if full:
        dst[:full * pat.numel()].view(full, pat.numel()).copy_(pat.expand(full, pat.numel()))
    dst[full * pat.numel():].copy_(pat[:n - full * pat.numel()])
    assert dst.data_ptr() % 512 == lead and dst.numel() == n
    return dst


@pytest.mark.parametrize("row,form", mc.pinned_cases(), ids=[f"{r.id}-{f.name}" for r, f in mc.pinned_cases()])
def test_pinned(row, form):
    n, size = row.n, np.dtype(form.dtype).itemsize
    footprint = (8 + size + 1 + (8 if form.ideal_lead % 16 else 0)) * n + (16 << 20)
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < footprint + HEADROOM:
        pytest.skip(f"{row.id} {form.name} needs {footprint + HEADROOM} bytes free on the device ({footprint} + 2 GiB), {free} are")
    refs = mc.row_refs(row)
    ideal = fixed = None
    t0 = time.perf_counter()
    try:
        ideal = _tiled("ideal", n, form.ideal_lead)
        fixed = _tiled(form.dtype, n, form.fixed_lead)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        bad = _check(ideal, fixed, refs)
        assert not mc.one_launch(n, form.dtype, ideal.data_ptr(), fixed.data_ptr())
        # the twin: the same data, aligned u8, through the one-launch form
        if form.ideal_lead % 16:
            ideal = None
            ideal = _tiled("ideal", n, 0)
        if form.dtype != "uint8" or form.fixed_lead % 16:
            fixed = None
            fixed = _tiled("uint8", n, 0)
        assert mc.one_launch(n, "uint8", ideal.data_ptr(), fixed.data_ptr())
        twin = _check(ideal, fixed, refs)
    finally:
        ideal = fixed = None
        torch.cuda.empty_cache()
    print(f"\n{row.id} {form.name}: {row.reaches}; {len(mc.part_bounds(row.nbf)) - 1} part(s), reference {row.ref}; "
          f"build {(t1 - t0) * 1e3:.1f} ms, the call and its twin's {(time.perf_counter() - t1) * 1e3:.1f} ms")
    assert not bad and not twin, f"{form.name}: {bad or 'passes'}; its aligned-u8 twin: {twin or 'passes'}"


# ---- the byte tricks of the one-launch form ----------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1], ids=["leaf", "blocks"])
@pytest.mark.parametrize("shift", [0, 1])
def test_byte_pairs(shift, lead):
    yi, yf = mc.byte_pairs(shift)
    ideal = guarded_input(torch.from_numpy(yi), device=DEV)
    fixed = guarded_input(torch.from_numpy(yf), lead_bytes=lead, device=DEV)
    assert mc.one_launch(yi.size, "uint8", ideal.data_ptr(), fixed.data_ptr()) == (lead == 0)
    ref = mc.sums_ref(yi, yf)
    assert ref[4] == ref[5] == 512  # every byte value 512 times
    bad = _check(ideal, fixed, (("numpy", ref),))
    assert not bad, bad


# ---- the routes, drawn ---------------------------------------------------------------------------------
def _run(c: mc.Case, seen: Counter) -> None:
    yi, yf = mc.make_data(c)
    ideal = guarded_input(torch.from_numpy(yi), lead_bytes=c.ideal_lead, device=DEV)
    raw = guarded_input(torch.from_numpy(np.ascontiguousarray(yf).view(np.uint8)), lead_bytes=c.fixed_lead, device=DEV)
    fixed = raw.view(TORCH_DT[c.dtype])
    assert fixed.numel() == c.n and fixed.dtype == TORCH_DT[c.dtype]
    assert c.n == 0 or (ideal.data_ptr() % 512, fixed.data_ptr() % 512) == (c.ideal_lead, c.fixed_lead)  # (empty: no address)
    kernels = [k for k, _, _ in mc.launches_of(c.n, c.dtype, ideal.data_ptr(), fixed.data_ptr())]
    assert kernels == mc.route_kernels(c), (c, kernels)  # the call takes the route it was built for
    bad = _check(ideal, fixed, (("numpy", mc.sums_ref(yi, yf)),))
    assert not bad, (c, bad)
    seen[(c.route, c.variant)] += 1


def test_forms_property():
    seen = Counter()

    def call(c):
        _run(c, seen)

    run = given(mc.forms_case())(call)
    for c in mc.pinned_examples():
        run = example(c)(run)
    settings(max_examples=mc.MAX_EXAMPLES, **SETTINGS)(run)()
    total = sum(seen.values())
    print({r: round(sum(v for (q, _), v in seen.items() if q == r) / total, 3) for r in mc.ROUTES}, f"of {total} calls; "
          f"the rarest (route, variant) ran {min(seen.values())} times")
    assert set(seen) == set(mc.variants()), set(mc.variants()) - set(seen)
