"""Record tests/golden/nonfinite.npz / nonfinite.json by running the REFERENCE on the cases of
tests/nonfinite_cases.py.

Runs only where the read-only reference is present (its root: FIR_REFERENCE, default
/root/reference); the tests only read the files written here.  No reference source text is copied:
the script imports the reference's own functions and stores their outputs as data (the inputs are
rebuilt by tests/nonfinite_cases.py and not stored).

Reference entry points exercised (paths relative to the reference root):
  fir_1d/sim/vector/restore_images.py:51,57        _to_u8_clip, _to_u8_normalized
  fir_1d/sim/vector/gen_3tap_compare_report.py:67  _compute_metrics
  fir_1d/model/python/fir_1d_ref.py:43             fir_1d_ideal

Files written:
  nonfinite.npz   restore: the uint8 output of every restore case, keyed by the case id
  nonfinite.json  {"metrics": {case id: the reference's metrics, floats as exact hex, NaN as "nan"},
                   "ideal": {case id: {"row": r, "expect": [hex floats]} or {"error", "message"}}}
                  ideal: fir_1d_ideal on row IDEAL_ROW of the case's image, for the finite-tap cases
                  of the two small shapes.  The reference refuses |h| > 8 (fir_1d_ref.py:21), so the
                  overflow tap sets are recorded as its error; only the subnormal and min-normal
                  sets have outputs.

Usage:  python tests/golden/make_nonfinite.py
"""
from __future__ import annotations

import json
import math
import os
import sys
import warnings
from pathlib import Path

import numpy as np

REF = Path(os.environ.get("FIR_REFERENCE", "/root/reference"))
OUT = Path(__file__).resolve().parent
ROOT = OUT.parents[1]
IDEAL_ROW = 1                      # the row of the case's image given to fir_1d_ideal
IDEAL_SHAPES = ((3, 68), (5, 67))  # "one short row each"


def _hex(v):
    return v if isinstance(v, int) else ("nan" if math.isnan(v) else float(v).hex())


def main():
    for p in (ROOT, ROOT / "warmup-fir-filter_amd", ROOT / "tests", REF):
        if str(p) not in sys.path:
            sys.path.insert(0, str(p))
    import nonfinite_cases as nc
    from fir_1d.model.python import fir_1d_ref
    from fir_1d.sim.vector import gen_3tap_compare_report as rep
    from fir_1d.sim.vector import restore_images as ri

    arrays, metrics, ideal = {}, {}, {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")  # NumPy's invalid-value / overflow warnings: the cases' subject
        for c in nc.cases("restore_u8"):
            fn = ri._to_u8_clip if c.args["policy"] == nc.CLIP else ri._to_u8_normalized
            arrays[c.id] = fn(c.args["a"])
        for c in nc.cases("compare_metrics"):
            metrics[c.id] = {k: _hex(v) for k, v in rep._compute_metrics(c.args["ideal"], c.args["fixed"]).items()}
        for c in nc.cases("fir1d_ideal_rows"):
            if not c.args["finite"] or c.args["shape"] not in IDEAL_SHAPES:
                continue
            x = nc.ideal_x(c.args["shape"])[IDEAL_ROW]
            try:
                y = fir_1d_ref.fir_1d_ideal(x.tolist(), c.args["h"].tolist())
                ideal[c.id] = {"row": IDEAL_ROW, "expect": [_hex(v) for v in y]}
            except Exception as exc:  # the exception type and text, as make_golden.py records them
                ideal[c.id] = {"error": type(exc).__name__, "message": str(exc)}
    np.savez_compressed(OUT / "nonfinite.npz", **arrays)
    (OUT / "nonfinite.json").write_text(json.dumps({"metrics": metrics, "ideal": ideal}, indent=0) + "\n")
    print("restore", len(arrays), "metrics", len(metrics), "ideal", len(ideal),
          "of which errors", sum("error" in v for v in ideal.values()))


if __name__ == "__main__":
    main()
