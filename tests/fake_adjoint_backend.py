"""The oracle-backed backend double (tests/fake_backend.py) with the adjoint call added: ``ns2d_adjoint`` runs the NumPy
restatement of tests/adjoint_restatement.py on CPU tensors and records the order of the calls ``NSAdjointOptimizer`` makes."""
import torch

from tests import adjoint_restatement as R
from tests.fake_backend import FakeBackend


class FakeAdjointBackend(FakeBackend):
    def __init__(self):
        super().__init__()
        self.calls = []

    def ns2d_reset(self, P, T, u0, v0, p0, mask, B):
        self.calls.append(("reset", float(u0.sum()), float(v0.sum()), float(p0.sum())))
        super().ns2d_reset(P, T, u0, v0, p0, mask, B)

    def ns2d_rollout(self, P, T, obs, actions, rewards, terminated, B):
        self.calls.append(("rollout", tuple(actions.shape)))
        super().ns2d_rollout(P, T, obs, actions, rewards, terminated, B)

    def ns2d_adjoint(self, P, T, obs, a_nom, ratio, width, grad, actions, lam=None, t0=0):
        self.calls.append(("adjoint", tuple(obs.shape), t0, lam is not None))
        orc = self._orc_ns(T)
        l, g, a = R.march(orc, obs.numpy(), T["U_ref"].numpy(), a_nom.numpy(), ratio=ratio, width=width, t0=t0)
        grad.copy_(torch.from_numpy(g))
        actions.copy_(torch.from_numpy(a))
        if lam is not None:
            lam.copy_(torch.from_numpy(l))
