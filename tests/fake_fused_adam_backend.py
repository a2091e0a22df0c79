"""A CPU double of ``HipBackend.fused_adam`` / ``fused_adam_workspace`` built on the NumPy restatement
(tests/fused_adam_restatement.py): it drives ``pde_control_gym.FusedAdam`` on CPU tensors, so the optimiser's host logic -- mirrors,
version bookkeeping, state dictionaries -- is tested without a GPU.  Same signature, the descriptor's checks as assertions; results
are written into the tensors in place (``.numpy()`` shares memory with a CPU tensor).  It also stands in for the MLP kernels of a
``FusedMLP`` that is only constructed and refreshed (no launch is made)."""
from __future__ import annotations

import numpy as np
import torch

from tests import fused_adam_restatement as R

F32 = torch.float32


class FakeFusedAdamBackend:
    name = "fused-adam-restatement"

    def __init__(self):
        self.calls = 0
        self.polyak_calls = 0
        self.seen = []

    def fused_adam_workspace(self, sizes):
        assert 1 <= len(sizes) <= 32 and all(int(s) >= 1 for s in sizes)
        return 8 * sum(min((int(s) + 1023) // 1024, 256) for s in sizes)

    def fused_adam(self, entries, state, workspace, lr, beta1, beta2, eps, max_grad_norm=None, tau=None, polyak=False, total_norm=None,
                   cache=None):
        assert 1 <= len(entries) <= 32
        assert state.dtype == torch.float64 and tuple(state.shape) == (3,)
        assert workspace.dtype == torch.uint8 and workspace.numel() >= self.fused_adam_workspace([e["p"].numel() for e in entries])
        tensors = []
        for e in entries:
            p = e["p"]
            n = p.numel()
            t = {}
            for k in ("p", "g", "m", "v", "copy", "pt", "pt_copy"):
                x = e.get(k)
                if x is None:
                    assert k not in ("p", "g", "m", "v")
                    continue
                assert x.dtype == F32 and x.is_contiguous() and x.numel() == n and not x.requires_grad, (k, x.dtype, tuple(x.shape))
                t[k] = x.numpy()
            for k in ("wt", "pt_wt"):
                if e.get(k) is not None:
                    wt, out_total, row0 = e[k]
                    out, in_ = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, n)
                    assert wt.dtype == F32 and wt.is_contiguous() and row0 + out <= out_total and wt.numel() >= (in_ + 3) // 4 * out_total * 4
                    t[k] = (wt.numpy(), int(out_total), int(row0))
            assert "pt" in t or ("pt_copy" not in t and "pt_wt" not in t)
            t["g"] = t["g"].copy()          # (read only)
            tensors.append(t)
        lr_value = float(lr.reshape(-1)[0]) if torch.is_tensor(lr) else float(lr)
        if torch.is_tensor(lr):
            assert lr.dtype == F32
        total = R.step(tensors, state.numpy(), lr_value, beta1, beta2, eps, max_grad_norm, tau, polyak, dtype=np.float32)
        if total_norm is not None and total is not None:
            total_norm[0] = float(total)
        self.calls += 1
        self.polyak_calls += int(bool(polyak))
        self.seen.append(tuple(e["g"].data_ptr() for e in entries))
