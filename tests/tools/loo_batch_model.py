"""Stand-in of ``gpry_amd._lib.Device`` with the batched leave-one-out objective, for the tests without a GPU:
``loo_fit_model.LooDevice`` plus ``loo_objective_batch`` as a loop over the numpy closed form (formulation (b)), so that a
row of a batch has the bits of the single call, as on the device.  Counts the batch calls and their rows; the single
calls keep their own counter (``n_loo``).  Test infrastructure only.
"""
import numpy as np

from loo_fit_model import LooDevice, loo_one_product


class LooBatchDevice(LooDevice):
    n_loo_batch = 0         # calls
    n_loo_rows = 0          # thetas they carried

    def loo_objective_batch(self, thetas, eval_gradient=True):
        thetas = np.atleast_2d(np.asarray(thetas, dtype=float))
        B, w = thetas.shape
        assert w == self.n_theta
        self.n_loo_batch += 1
        self.n_loo_rows += B
        val, grad, info = np.empty(B), np.zeros((B, w)), np.zeros(B, dtype=np.int32)
        for j in range(B):
            out = loo_one_product(self.X_, self.y_, self.alpha, thetas[j], self.kid, self.white, eval_gradient)
            val[j] = out[0] if eval_gradient else out
            if eval_gradient:
                grad[j] = out[1]
            info[j] = int(not np.isfinite(val[j]))
        return (val, grad, info) if eval_gradient else (val, info)
