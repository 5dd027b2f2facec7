"""NORA.multi_add over a device whose shortlist comes from a pruned sweep (option "sweep_prune"): the records are exact, but
the bound may be any value >= the full sweep's -- the largest acquisition bound of a candidate that was never contracted.
The extension loop of multi_add must still arrive at the reference's proposals.  The double below restates the library's
answer rule in numpy (sweep_topk.hip: prune_topk; its contracted set only grows x 8, without the survivor round) with a
deliberately loose bound: the acquisition at the largest sigma of the pool."""
import numpy as np
import pytest

from oracle import gpry_oracle as orc
from test_host_logic_cpu import FakeDevice, FakeGPR, _golden_model


class PrunedFakeDevice(FakeDevice):
    """Records of the top K' candidates by bound are exact, every other candidate carries its bound; the shortlist is
    the top K of that mixed array when all of it is exact, otherwise K' grows x 8 or the full sweep runs."""

    def __init__(self, model):
        super().__init__(model)
        self.options = {"sweep_prune": 0}
        self.calls = []
        self.sweep_epoch = 0

    def set_option(self, key, value):
        self.options[key] = int(value)

    def sweep_logexp(self, X, zeta, baseline, sigma_n, mask=None, M=None, want=()):
        out = super().sweep_logexp(X, zeta, baseline, sigma_n, mask=mask, M=M, want=want)
        self.sweep_epoch += 1
        self.pruned = self.options["sweep_prune"] == 1 and not want
        if self.pruned:
            s0 = np.full_like(self.s, np.max(self.s))          # >= every sigma: an upper bound of every acquisition
            self.ub = orc.logexp_f(self.y, s0, baseline, sigma_n, zeta)
            self.n_eval, self.completed, self.rounds = 0, 0, 0
        return out

    def _mixed(self):
        order = np.lexsort((-np.arange(len(self.ub)), -self.ub))
        exact = np.zeros(len(self.ub), bool)
        exact[order[:self.n_eval]] = True
        return np.where(exact, self.acq, self.ub), exact

    def sweep_topk(self, K, exclude=None):
        self.calls.append(K)
        if not self.pruned:
            return super().sweep_topk(K, exclude)
        M = len(self.acq)
        while True:
            if self.n_eval:
                mixed, exact = self._mixed()
                ok = np.ones(M, bool)
                if exclude is not None:
                    ok[np.asarray(exclude, dtype=int)] = False
                order = np.lexsort((-np.arange(M), -mixed))
                order = order[ok[order]]
                if exact[order[:K]].all():
                    top, _ = super().sweep_topk(K, exclude)
                    np.testing.assert_array_equal(top["idx"], order[:K])
                    bound = mixed[order[K]] if len(order) > K else -np.inf
                    return top, bound
            kq = max(4 * K, 8, 8 * self.n_eval)
            if kq > M // 4:
                self.pruned, self.completed = False, 1
                return super().sweep_topk(K, exclude)
            self.n_eval, self.rounds = kq, self.rounds + 1

    def sweep_fetch(self, want=("y", "sigma")):
        if self.pruned:
            self.pruned, self.completed = False, 1
        return {"y": self.y, "sigma": self.s, "acq": self.acq}

    def sweep_prune_info(self):
        return {"pruned": int(self.pruned), "K_prime": self.n_eval, "rounds": self.rounds, "completed": self.completed}


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("shortlist", [4, 64])
def test_multi_add_over_inflated_bounds_returns_the_reference_proposals(tag, shortlist):
    from gpry_amd.gp_acquisition import NORA
    g, p, bounds, Xc, m = _golden_model(tag)
    gpr = FakeGPR(m)
    gpr.device = PrunedFakeDevice(m)
    npts = len(g[p + "acq_cond"]) - 1
    acq = NORA(bounds, sampler="uniform", mc_every=1, verbose=0, shortlist_size=shortlist, devices=[0])
    acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    np.testing.assert_array_equal(Xp, g[p + "X_pool"])
    np.testing.assert_allclose(yp, g[p + "y_pool"], rtol=1e-9)
    np.testing.assert_allclose(ap, g[p + "acq_pool"], rtol=1e-8)
    np.testing.assert_allclose(acq.pool.acq_cond, g[p + "acq_cond"], rtol=1e-6)
    assert gpr.device.options["sweep_prune"] == 0            # switched on around the sweep only
    assert acq.stats["prune"][0]["K_prime"] > 0 or acq.stats["prune"][0]["completed"]


def test_exact_prune_off_leaves_the_option_alone():
    from gpry_amd.gp_acquisition import NORA
    g, p, bounds, Xc, m = _golden_model("a")
    gpr = FakeGPR(m)
    gpr.device = PrunedFakeDevice(m)
    npts = len(g[p + "acq_cond"]) - 1
    acq = NORA(bounds, sampler="uniform", mc_every=1, verbose=0, shortlist_size=4, devices=[0], exact_prune=False)
    acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)
    Xp, _, _ = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    np.testing.assert_array_equal(Xp, g[p + "X_pool"])
    assert not gpr.device.pruned and "prune" not in acq.stats
