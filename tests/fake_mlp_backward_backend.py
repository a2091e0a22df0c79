"""CPU double of ``HipBackend.mlp_forward`` / ``mlp_backward`` built on tests/mlp_backward_exact.py: drives ``FusedMLP.with_grad`` on CPU
tensors.  The forward reads what the kernel would read -- the BLOCKED weight copies and the biases behind the descriptor's pointers --
so a stale copy shows; the backward checks that copy against the row-major weights it is handed.  Plain helper module."""
from __future__ import annotations

import ctypes as C

import numpy as np

from pdecontrolgym_amd import _native as N
from tests import mlp_backward_exact as R

ACTS = {N.MLP_IDENTITY: None, N.MLP_TANH: "tanh", N.MLP_RELU: "relu"}


def _floats(ptr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr)).astype(np.float64)


def layers_from_descriptor(net):
    """[(W float64 [out, in], b or None, act)] from the blocked copies [ceil(in / 4), out, 4] a ``pdegym_mlp`` points to."""
    out = []
    for l in range(net.n_layers):
        L = net.layer[l]
        k4 = (L.in_dim + 3) // 4
        blocked = _floats(L.w, k4 * L.out_dim * 4).reshape(k4, L.out_dim, 4)
        assert (blocked.transpose(1, 0, 2).reshape(L.out_dim, 4 * k4)[:, L.in_dim:] == 0).all(), "the padding of the blocked copy is not zero"
        W = blocked.transpose(1, 0, 2).reshape(L.out_dim, 4 * k4)[:, :L.in_dim].copy()
        out.append((W, None if not L.b else _floats(L.b, L.out_dim), ACTS[L.act]))
    return out


class FakeMlpBackend:
    def __init__(self):
        self.forward_calls, self.backward_calls = 0, []

    @staticmethod
    def _plain(net):
        assert net.head == N.MLP_HEAD_PLAIN and net.clamp == 0 and not net.noise, "with_grad evaluates the bare layers"

    def mlp_forward(self, net, x, y, B):
        self.forward_calls += 1
        h = R.forward_all(layers_from_descriptor(net), x.detach().numpy().astype(np.float32))[-1]
        if net.clamp:
            h = np.clip(h, net.lo, net.hi)
        y.copy_(__import__("torch").from_numpy(h).to(y.dtype))

    def mlp_backward(self, net, x, dy, weights, dw, db, dx=None, slabs=0):
        import torch
        self._plain(net)
        L = layers_from_descriptor(net)
        for (W, _, _), w in zip(L, weights):
            assert np.array_equal(W, w.detach().numpy().astype(np.float64)), "the blocked copy is not the row-major weight"
        self.backward_calls.append({"dx": dx is not None, "B": int(x.shape[0]), "slabs": slabs})
        want, _ = R.reference_backward(L, x.detach().numpy().astype(np.float32), dy.detach().numpy())
        for l in range(net.n_layers):
            dw[l].copy_(torch.from_numpy(want["dw"][l]).float())
            assert (db[l] is None) == (want["db"][l] is None)
            if db[l] is not None:
                db[l].copy_(torch.from_numpy(want["db"][l]).float())
        if dx is not None:
            dx.copy_(torch.from_numpy(want["dx"]).float())
