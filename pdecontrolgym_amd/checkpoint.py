"""The base of the batched engines: what the four of them share on the host side (backend hand-over, observation ping-pong, fused
auto-reset bookkeeping, host-facing packs) and checkpoint / resume (``state_dict()`` / ``load_state_dict()``).

The reference's training scripts checkpoint every N steps (examples/transportPDE/transport1Dppo.py:80-86 saves the model; its
single environment is rebuilt from its parameter dictionary).  A batch of thousands of instances in mid-episode is not
rebuildable that way, so every engine can hand out and take back its device state:

    sd = venv.state_dict()            # torch tensors (clones) + a few Python scalars: ``torch.save(sd, path)`` works
    ...
    venv.load_state_dict(sd)          # same construction parameters required; copies IN PLACE (captured hipGraphs stay valid)

What is state: everything in the engine's tensor dictionary that a step reads and that is not a constructor constant or a
per-call input -- live rows / fields, plant parameters, time indices, the reward's running sums, the fused auto-reset pools and
their restart counters, the last outputs.  What is not: user callbacks and their random generators (Python objects of the
caller), the contents of ``DeviceRollout`` buffers.
"""
from __future__ import annotations

# 1: rounds 3-4 (meta without the reward / sensing keys of the 1D engine, no "format" entry); 2: round 5 on
CHECKPOINT_FORMAT = 2

# per-call inputs, scratch and constructor constants: not part of a checkpoint
_SKIP = {"action", "state_in", "scratch", "U_ref", "action_ref", "xscale", "active", "reset_profile", "p_out", "control", "kill"}


class EngineCheckpoint:
    """Base of the batched engines (``self.t``: name -> tensor | None, ``self.num_envs``, ``self.device``): what they share
    besides the checkpoint -- the backend hand-over, the double-buffered observation, the fused auto-reset's bookkeeping and the
    host-facing hand-over (``hostio.PackLayout``)."""

    _hio = None            # the pinned host pack of ``enable_host_io`` and its prepared call (1D and Navier-Stokes engines)
    _host_views = None     # (fetched copy of ``host_pack``, its NumPy views) of ``host_views`` (traffic and tumour engines)

    def _bind_backend(self, backend):
        """``self.backend``: the given one (a test double is told its engine through ``bind``), by default the process-wide HIP backend."""
        if backend is None:
            from .backend import default_backend
            backend = default_backend()
        self.backend = backend.bind(self) if hasattr(backend, "bind") else backend

    def _as_mask(self, mask):
        """A per-instance selection (bool / uint8 / anything array-like) as the uint8 device tensor the kernels read."""
        import torch
        return torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()

    def _flip_obs(self, out_obs=None, avoid=None):
        """Name the tensor the next launch writes its observation to.  Observations are double-buffered (``self._obs``, ``self._flip``):
        the tensor step k returned stays valid during step k + 1.  ``out_obs``: the caller's buffer (e.g. slot t + 1 of a rollout)
        receives it instead; ``avoid``: the tensor that holds the state the launch reads, never written over."""
        if out_obs is not None:
            self.t["obs"] = out_obs.view(self._obs[0].shape)
            return
        self._flip ^= 1
        if self._obs[self._flip] is avoid:
            self._flip ^= 1
        self.t["obs"] = self._obs[self._flip]

    # ---- fused auto-reset: pools, restart counters, terminal observations ------------------------------------------------------
    def _set_auto_reset(self, pools: dict, keep_final_obs: bool):
        import torch
        own = self._obs[0]
        self.t.update(pools)
        self.t["reset_count"] = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.t["final_obs"] = torch.zeros(own.shape, dtype=own.dtype, device=self.device) if keep_final_obs else None
        self._drop_prepared_call()

    def _clear_auto_reset(self, pool_keys):
        for k in (*pool_keys, "reset_count", "final_obs"):
            self.t[k] = None
        self._drop_prepared_call()

    # ---- host-facing hand-over ---------------------------------------------------------------------------------------------------
    def _enable_host_io(self, spec, align):
        """The batch-of-one faces' hand-over: the command and everything a host caller reads after a step live in ONE pinned host
        allocation that is mapped into the device's address space (hipHostMalloc), laid out by ``spec`` (``hostio.PackLayout``).
        The kernels read the command from it and write their results into it directly, so an env-step is the step's launches + ONE
        stream synchronisation: no copies in either direction, no torch dispatch.  The engine's tensor dictionary names the
        segments; returns their NumPy views (``self._hio["np"]``)."""
        from .hostio import PackLayout
        layout = PackLayout(spec, align)
        pack, views = layout.allocate(self.device, host=True)
        self.t.update(views)
        self._obs = [views["obs"], views["obs"]]
        self._hio = {"pack": pack, "np": layout.numpy_views(pack.numpy()), "call": None}
        return self._hio["np"]

    def _drop_prepared_call(self):
        """Forget the prepared call of the host-io face (``step_host``): its argument structures hold the addresses of the tensors
        in ``self.t``, so every method that replaces one of them drops it and the next step rebuilds it."""
        if self._hio is not None:
            self._hio["call"] = None

    def sync_host(self):
        """Wait until the results of the last launch are in the host views."""
        if self.device.type == "cuda":
            import torch
            torch.cuda.current_stream(self.device).synchronize()

    def host_views(self, fetch):
        """The NumPy views (``pack_layout`` names) of a copy of ``host_pack`` fetched with ``fetch`` (a ``hostio.HostFetch``): ONE
        device-to-host copy and one synchronisation for everything a step produced.  Valid until the next call."""
        raw = fetch([self.host_pack])[0]
        if self._host_views is None or self._host_views[0] is not raw:
            self._host_views = (raw, self.pack_layout.numpy_views(raw))
        return self._host_views[1]

    # ---- checkpoint / resume -----------------------------------------------------------------------------------------------------
    def _checkpoint_meta(self):
        return {"engine": type(self).__name__, "num_envs": int(self.num_envs)}

    def state_dict(self):
        import torch
        sd = {"format": CHECKPOINT_FORMAT, "meta": self._checkpoint_meta(), "tensors": {}}
        for k, v in self.t.items():
            if torch.is_tensor(v) and k not in _SKIP:
                sd["tensors"][k] = v.detach().clone()
        return sd

    def load_state_dict(self, sd):
        import torch
        meta = self._checkpoint_meta()
        fmt = int(sd.get("format", 1))
        if fmt > CHECKPOINT_FORMAT:
            raise ValueError(f"checkpoint format {fmt} is newer than this library's ({CHECKPOINT_FORMAT}): upgrade the library")
        saved = sd.get("meta") or {}
        # every key the checkpoint recorded must agree; keys this library has added since (format 1 checkpoints of the 1D engine
        # know nothing of the reward / sensing configuration) are absent from an older checkpoint and are not held against it
        wrong = {k: (saved[k], meta.get(k)) for k in saved if saved[k] != meta.get(k)}
        if wrong or saved.get("engine") != meta.get("engine"):
            raise ValueError(f"checkpoint was written by {saved}, this engine is {meta} (mismatch: {wrong})")
        for k, v in sd["tensors"].items():
            cur = self.t.get(k)
            if torch.is_tensor(cur) and cur.shape == v.shape and cur.dtype == v.dtype:
                cur.copy_(v)                               # in place: addresses baked into captured graphs stay valid
            else:                                          # a pool / optional tensor this engine has not allocated (yet)
                self.t[k] = v.to(self.device).clone()
        self._after_load(sd)
        self._drop_prepared_call()

    def _after_load(self, sd):
        pass
