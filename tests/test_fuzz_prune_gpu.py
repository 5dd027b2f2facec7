"""Randomised exactness of the pruned sweep and of the sigma-only sweep (tests/tools/fuzz_prune.py): random N around the
padding quanta, d in 1..32, all four kernels and panel forms, pools resident or uploaded underneath the sweep, masks, device
gates, exclusions, tie blocks, K up to and past the finite count, 3-context groups.  The coverage tally is held to a floor
so that an edit of the generator cannot quietly shrink what is exercised."""
import os
import sys
from collections import Counter

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# item of the tally -> least number of cases over the three seeds
COVERAGE_FLOOR = {
    "kid0": 2, "kid1": 2, "kid2": 2, "kid3": 2,
    "form_mfma": 2, "form_difference": 2, "form_hybrid": 1,
    "outcome_round1": 2, "outcome_survivors": 1, "outcome_completed": 2,
    "multichunk_upload": 2, "multichunk_upload_gates": 1, "gates_no_mask": 1,
    "K_ge_finite": 2, "tie_at_K": 2, "group": 2, "sigma_only_pruned": 10,
    "N_le_128": 2, "d_1": 1, "d_gt_20": 2,
}


@pytest.mark.timeout(1200)
def test_pruned_and_sigma_only_sweeps_are_exact_on_random_configurations():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import fuzz_prune
    from gpry_amd import _lib
    dev = _lib.Device(0)
    total = Counter()
    for seed in (21, 22, 23):
        bad, worst, cov = fuzz_prune.run(n_cases=14, seed=seed, dev=dev)
        print(f"seed {seed}: worst {worst}; coverage {dict(sorted(cov.items()))}")
        assert bad == 0, (seed, worst)
        assert worst["mean"] < 1e-7 and worst["var"] < 1e-8
        total += cov
    print(f"coverage: {dict(sorted(total.items()))}")
    short = {k: (total[k], v) for k, v in COVERAGE_FLOOR.items() if total[k] < v}
    assert not short, short
