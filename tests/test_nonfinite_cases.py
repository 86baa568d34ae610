"""The NaN / infinity / subnormal cases of tests/nonfinite_cases.py, checked without a GPU: every
case holds what its id says and its expected output shows the special; the NumPy and the C oracle
agree on every ideal case, the non-finite taps included; the oracle's outputs are the ones the
reference recorded (tests/golden/nonfinite.*, written by tests/golden/make_nonfinite.py)."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest

import nonfinite_cases as nc
from conftest import GOLDEN, same_metrics
from oracle import c_oracle, fir_oracle as fo


@pytest.fixture(scope="module")
def golden():
    rec = json.loads((GOLDEN / "nonfinite.json").read_text())
    with np.load(GOLDEN / "nonfinite.npz") as d:
        rec["restore"] = {k: d[k] for k in d.files}
    return rec


# ---- the comparison rule itself ------------------------------------------------------------------
def test_comparison_rule():
    nan2 = np.array([0x7FF8000000000000, 0xFFF8000000000123], np.uint64).view(np.float64)  # other sign, payload
    assert nc.same_f64(nan2, np.array([np.nan, np.nan]))
    assert nc.same_f64([np.inf, -0.0, 5e-324], [np.inf, -0.0, 5e-324])
    assert not nc.same_f64([0.0], [-0.0])
    assert not nc.same_f64([np.inf], [-np.inf])
    assert not nc.same_f64([np.nan], [0.0]) and not nc.same_f64([0.0], [np.nan])
    assert not nc.same_f64([5e-324], [0.0])
    assert not nc.same_f64([1.0], [1.0, 1.0])
    assert nc.first_diff([1.0, np.nan, 0.0], [1.0, np.nan, -0.0]) == (2, 0.0, -0.0)
    assert nc.first_diff([np.nan], [np.nan]) is None


# ---- the cases -----------------------------------------------------------------------------------
def test_ids_are_unique_and_every_family_and_branch_is_present():
    cases = nc.cases()
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids))
    assert all(c.reason and c.kernels and c.claims for c in cases)
    kernels = {k for c in cases for k in c.kernels}
    assert kernels == {"restore_map_kernel", "restore_minmax_kernel", "restore_params_kernel", "metrics_prep",
                       "metrics_leaf_kernel", "metrics_blocks", "metrics_blocks_any", "metrics_ragged", "metrics_final",
                       "fir1d_ideal_reg_kernel", "fir1d_ideal_kernel", "fir2d_ideal_reg_kernel",
                       "fir2d_ideal_generic_kernel"}
    # sizes and forms of the issue, each with at least one case
    for n in nc.RESTORE_SIZES:
        assert any(c.entry == "restore_u8" and c.args["a"].size == n and c.args["policy"] == nc.CLIP for c in cases), n
    for n in nc.RESTORE_SIZES[1:]:
        assert any(c.entry == "restore_u8" and c.args["a"].size == n and c.args["policy"] == nc.NORMALIZE for c in cases), n
    for form in nc.METRIC_FORMS:
        for n in nc.METRIC_SIZES:
            assert any(c.entry == "compare_metrics" and c.args["form"] == form and c.args["ideal"].size == n for c in cases)
    for shape in nc.IDEAL_SHAPES:
        for L in nc.IDEAL_REG_L + nc.IDEAL_GENERIC_L:
            mine = [c for c in cases if c.entry == "fir1d_ideal_rows" and c.args["shape"] == shape and len(c.args["h"]) == L]
            assert any(c.args["finite"] for c in mine) and any(not c.args["finite"] for c in mine), (shape, L)
    assert any(c.entry == "fir1d_ideal_rows" and len(c.args["h"]) == nc.IDEAL_LONG[1] for c in cases)
    assert all(np.isfinite(c.args["h2"]).all() for c in cases if c.entry == "fir2d_ideal")  # the header defines no other


def test_every_case_holds_what_its_id_claims():
    for c in nc.cases():
        assert nc._claims_hold(c), c.id
        # ... and its plain twin holds no special at those places
        for name, idx, _ in c.claims:
            v = float(np.asarray(c.plain[name]).reshape(-1)[idx])
            assert math.isfinite(v) and abs(v) < 1e3 and (v == 0.0 or abs(v) > 1e-3), c.id


def test_every_expected_output_shows_the_special():
    """A case whose expected output equals its plain twin's is rejected by the builder; the only
    rejected ones are subnormal taps in filters too long for the input's isolated sample (their
    products are absorbed by the ordinary taps' everywhere)."""
    keep, dropped = nc.built()
    assert all(nc.shows(c) for c in keep)
    assert all("-subnormal-" in d and ("-L33-" in d or "-L1030-" in d) for d in dropped), dropped
    assert len(dropped) == 9


def test_expected_outputs_hold_the_values_the_issue_predicts():
    by_id = {c.id: c for c in nc.cases()}
    e = nc.expected(by_id["restore-norm-n257-one-nan-mid"])
    assert not e.any()  # one NaN among finite values: every pixel is cast(NaN) = 0
    e = nc.expected(by_id["restore-norm-n257-subnormal-range"])
    assert e[:3].tolist() == [255, 0, 255] and set(e.tolist()) == {0, 255}
    assert not nc.expected(by_id["restore-norm-n257-overflow-subnormal"]).any()
    m = nc.expected(by_id["metrics-u8-n16461-pinf-ninf-blocks"])
    assert m["max_abs_err"] == math.inf and m["mae"] == math.inf and math.isnan(m["mean_err"])
    m = nc.expected(by_id["metrics-u8off1-n73728-d2-overflow"])
    assert m["rmse"] == math.inf and math.isfinite(m["mae"])
    m = nc.expected(by_id["metrics-i16-n1000-nzero-nsub"])
    assert m["clip_needed_ratio"] == 1 / 1000  # -5e-324 is < 0, -0.0 is not
    m = nc.expected(by_id["metrics-f32-n1000-above-255"])
    assert m["clip_needed_ratio"] == 1 / 1000
    m = nc.expected(by_id["metrics-f64-n73728-nan-last-workgroup"])
    assert all(math.isnan(m[k]) for k in ("max_abs_err", "mae", "rmse", "mean_err"))


# ---- the two oracles -----------------------------------------------------------------------------
def test_numpy_and_c_oracle_agree_on_every_ideal_case():
    """oracle/fir_oracle.c adds a zero term for padding as the header defines the entry, so an
    infinite or NaN tap gives NaN at the row ends in both oracles (the issue's example first)."""
    co = c_oracle()
    x = np.array([[0, 1, 255, 0, 255, 7, 0, 3]], np.uint8)
    h = [np.inf, 1.0, 0.5]
    want = np.array([[np.inf, np.inf, np.nan, np.inf, np.inf, np.nan, np.inf, np.nan]])
    with np.errstate(all="ignore"):
        assert nc.same_f64(fo.fir1d_ideal_rows(x, h), want)
    assert nc.same_f64(co.fir1d_ideal_rows(x, h), want)
    for c in nc.cases("fir1d_ideal_rows"):
        got = co.fir1d_ideal_rows(nc.ideal_x(c.args["shape"]), c.args["h"])
        assert nc.same_f64(got, nc.expected(c)), (c.id, nc.first_diff(got, nc.expected(c)))


def test_c_oracle_is_unchanged_for_finite_taps():
    """The zero term leaves every finite-tap sum as it was: the reference's recorded random cases,
    bit for bit (skipping the term is what the reference's loop does)."""
    from conftest import iter_ragged

    co = c_oracle()
    for x, h, _, y in iter_ragged("ideal"):
        if x.size:
            assert co.fir1d_ideal_rows(fo.prep_x(x), h).tobytes() == y.tobytes()


# ---- the oracle against the reference's recorded outputs -----------------------------------------
def test_fixture_covers_the_cases(golden):
    assert set(golden["restore"]) == {c.id for c in nc.cases("restore_u8")}
    assert set(golden["metrics"]) == {c.id for c in nc.cases("compare_metrics")}
    small = {c.id for c in nc.cases("fir1d_ideal_rows") if c.args["finite"] and c.args["shape"] in ((3, 68), (5, 67))}
    assert set(golden["ideal"]) == small


def test_restore_oracle_equals_the_reference(golden):
    for c in nc.cases("restore_u8"):
        want = golden["restore"][c.id]
        assert want.dtype == np.uint8 and np.array_equal(nc.expected(c), want), c.id
    # the reference's cast of NaN (NumPy leaves it unspecified): 0, the value the kernels pin
    assert golden["restore"]["restore-clip-n1-nan"].tolist() == [0]
    assert not golden["restore"]["restore-norm-n257-one-nan-first"].any()
    assert not golden["restore"]["restore-norm-n257-all-nan"].any()


def test_metrics_oracle_equals_the_reference(golden):
    for c in nc.cases("compare_metrics"):
        want = {k: (v if isinstance(v, int) else (float("nan") if v == "nan" else float.fromhex(v)))
                for k, v in golden["metrics"][c.id].items()}
        got = nc.expected(c)
        assert not same_metrics(got, want), (c.id, {k: (got[k], want[k]) for k in same_metrics(got, want)})


def test_ideal_oracle_equals_the_reference(golden):
    """fir_1d_ideal accepts the subnormal and min-normal tap sets and refuses the overflow sets
    (|h| > 8 is an error of the drop-in model, which is why only the C ABI sees them)."""
    by_id = {c.id: c for c in nc.cases("fir1d_ideal_rows")}
    outputs = 0
    for cid, rec in golden["ideal"].items():
        c = by_id[cid]
        if "error" in rec:
            assert rec["error"] == "ValueError" and rec["message"].endswith("|h| must be <= 8.0."), cid
            assert "overflow" in cid and np.abs(c.args["h"]).max() > 8.0
            continue
        outputs += 1
        assert "subnormal" in cid or "min-normal" in cid
        want = np.array([float.fromhex(v) for v in rec["expect"]])
        got = nc.expected(c)[rec["row"]]
        assert nc.same_f64(got, want), (cid, nc.first_diff(got, want))
    assert outputs >= 40
