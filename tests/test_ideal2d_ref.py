"""The NumPy checker of the float64 ideal 2-D FIR (tests/ideal2d_ref.py) is itself checked:
against the formula in plain Python floats, against the 1-D oracle and the reference's recorded
1-D outputs (a kernel with one non-zero row or column is a 1-D filter), and for its ability to
see a reordered sum.  No GPU, no library."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

from ideal2d_ref import ideal2d, ideal2d_loop
from oracle import fir_oracle as fo


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("shape,kernel", [((7, 9), (3, 3)), ((5, 5), (5, 5)), ((4, 6), (2, 4)), ((1, 1), (3, 3)),
                                          ((3, 17), (1, 5)), ((9, 2), (5, 1))])
def test_vectorised_equals_plain_loop(shape, kernel):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] * 10 + kernel[0] + kernel[1])
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    h = rng.uniform(-8, 8, kernel)
    assert ideal2d(x, h).tobytes() == ideal2d_loop(x, h).tobytes()


def test_centre_row_and_centre_column_are_the_1d_oracle():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (23, 41), dtype=np.uint8)
    h1 = rng.uniform(-8, 8, 5)
    k = np.zeros((5, 5))
    k[2] = h1
    want = fo.fir1d_ideal_rows(x, h1)
    assert ideal2d(x, k).tobytes() == want.tobytes()
    xt = np.ascontiguousarray(x.T)
    assert np.ascontiguousarray(ideal2d(xt, k.T).T).tobytes() == want.tobytes()


def test_smallest_golden_image_matches_the_recorded_hashes(images, image_outputs):
    stem = min(images, key=lambda s: (images[s].size, s))
    x = images[stem]
    seen = 0
    for o in image_outputs["outputs"]:
        if o["tap"] != "5tap" or o["case_stem"] != stem:
            continue
        k = np.zeros((5, 5))
        k[2] = image_outputs["banks"]["5tap"][o["coeff_name"]]
        assert _sha(ideal2d(x, k)) == o["ideal_f64_sha256"], o["coeff_name"]
        assert _sha(ideal2d(np.ascontiguousarray(x.T), k.T).T) == o["ideal_f64_sha256"], o["coeff_name"]
        seen += 1
    assert seen == len(image_outputs["banks"]["5tap"])


def test_row_order_of_the_sum_is_observable():
    rng = np.random.default_rng(33070)
    x = rng.integers(0, 256, (33, 70), dtype=np.uint8)
    h = rng.uniform(-8, 8, (5, 5))
    fwd = ideal2d(x, h)
    rev = ideal2d(x, h, row_order=range(4, -1, -1))
    assert np.allclose(fwd, rev, rtol=0, atol=1e-9)  # the same sum ...
    assert (fwd.view(np.uint64) != rev.view(np.uint64)).any()  # ... in other bytes
