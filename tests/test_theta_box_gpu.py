"""The objective, the factor and the predictions of the device over the whole theta box: the corners of the box a full
hyper-parameter fit draws its restarts from (C from 1e-4 to 1e6, every length scale from 1e-3 to 10 box widths, alpha = 1e-4;
cond(K) up to 1e13), at (100, 3) the one-launch objective and, with ``lml_small`` = 0, the general chain on one tile, (130, 2)
the first size with two tile rows and the stacked inverse, (333, 5) 384 padded rows, also with the recursive inverse
(``chol_stacked`` = 0) and through ``lml_batch`` under both schedules.

Truth, yardstick and the assertions themselves are in tests/tools/theta_box_model.py and run without a GPU in
tests/test_theta_box_cpu.py (a float64 stand-in passes them; one whose kernel entries are off by 16 ulps does not).  Every
bound is err_device <= max(10 E64, floor): both errors against the long-double truth, E64 the float64 noise level of the
model (two numpy formulations, three row orders), the floors the fixed tolerances of tests/test_hip_parity.py,
tests/tools/fuzz_parity.py and test_factor_chain_at_ragged_block_counts.  The measured ratios: profiles/theta_box.md.
"""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import theta_box_model as tb  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tb.EXTENDED, reason="np.longdouble is no wider than float64 here")]

CASES = [(N, d, kid, ti) for (N, d) in tb.SIZES for kid in range(4) for ti in range(len(tb.THETAS))]
IDS = [f"n{N}_d{d}_k{kid}_{tb.THETAS[ti][0]}" for N, d, kid, ti in CASES]


@pytest.fixture(scope="module")
def dev():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_objective_on_every_path(dev, case):
    tb.check_objective(dev, tb.model(*case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_factor(dev, case):
    tb.check_factor(dev, tb.model(*case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predictions(dev, case):
    tb.check_predictions(dev, tb.model(*case))


@pytest.mark.parametrize("C", [1e-4, 1.0, 1e6])
def test_exact_limit(dev, C):
    tb.check_exact_limit(dev, C)


@pytest.mark.parametrize("N,d", tb.SIZES)
@pytest.mark.parametrize("kid", range(4))
def test_not_positive_definite_corner(dev, N, d, kid):
    tb.check_not_positive_definite(dev, N, d, kid)
