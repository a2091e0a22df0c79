"""HIP backend: turns (params struct, dict of torch tensors) into C-ABI calls on libpdegym_hip.so.

The batched environment cores (batch1d.py / batch2d.py) talk to a backend object with this small
interface.  ``HipBackend`` is the only backend the product ships; it refuses CPU tensors.  (The CPU test
suite injects an oracle-backed double from tests/ to exercise host logic without a GPU.)
"""
from __future__ import annotations

import ctypes as C

from . import _native as N


def _on_device_of(key):
    """Decorator: run the C-ABI call with the device of tensor-dict entry ``key`` (or of the tensor argument at that position)
    current.  The kernels launch on the thread's current HIP device and the stream handle passed is that device's current
    stream, so an engine built on cuda:1 while cuda:0 is current must switch first."""
    def deco(fn):
        def wrapped(self, *args, **kw):
            import torch
            dev = None
            for a in args:
                if isinstance(a, dict) and key in a:
                    dev = a[key].device
                    break
                if torch.is_tensor(a):
                    dev = a.device
                    break
            if dev is None or dev.type != "cuda" or dev.index == torch.cuda.current_device():
                return fn(self, *args, **kw)          # already current (the common case): no device switch, no context manager
            with torch.cuda.device(dev):
                return fn(self, *args, **kw)
        wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
        wrapped.device_guard_key = key          # (tests/test_host_api.py checks that every C-ABI entry point carries the guard)
        return wrapped
    return deco


def _prepared(fn, pP, pB, B, dev, what, keep):
    """A zero-argument callable that launches ``fn(pP, pB, B, stream)`` on the current stream of ``dev`` (made current first when
    another device is) and raises on failure.  ``keep``: what the argument structures point into, kept alive with the call."""
    import torch
    current_stream, current_device = torch.cuda.current_stream, torch.cuda.current_device

    def call(_keep=keep):
        if current_device() != dev.index:
            with torch.cuda.device(dev):
                rc = fn(pP, pB, B, current_stream(dev).cuda_stream)
        else:
            rc = fn(pP, pB, B, current_stream(dev).cuda_stream)
        if rc:
            N.check(rc, what)
    return call


def _final_obs_steps(prefix, x, shape, dtype, like):
    """The per-step terminal observations of a one-launch rollout (PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP), checked where the other rollout
    buffers are: a contiguous ``dtype`` tensor of ``shape`` on the device of ``like``.  Returns the flag word of the descriptor."""
    if x is None:
        return 0
    _check_shapes(prefix, {"final_obs_steps": (x, shape, dtype)})
    if x.device != like.device:
        raise N.NativeError(f"{prefix} final_obs_steps must live on {like.device}, got {x.device}")
    return N.ROLLOUT_FINAL_OBS_PER_STEP


def _check_shapes(prefix, wanted):
    """``wanted``: name -> (tensor | None, shape[, dtype]).  Every tensor given must be contiguous and have that shape (and dtype)."""
    for name, (x, shape, *dtype) in wanted.items():
        if x is not None and (tuple(x.shape) != tuple(shape) or not x.is_contiguous() or (dtype and x.dtype != dtype[0])):
            kind = "contiguous " + str(dtype[0]).replace("torch.", "") if dtype else "contiguous"
            raise N.NativeError(f"{prefix} {name} must be a {kind} {list(shape)} tensor, got {tuple(x.shape)}")


class HipBackend:
    name = "hip-gfx950"

    def __init__(self):
        self.lib = N.load()

    # ---- 1D -------------------------------------------------------------------------------------
    @staticmethod
    def _bufs1d(T) -> N.Bufs1D:
        import torch
        b = N.Bufs1D()
        si = T.get("state_in")
        if si is not None:       # the rows live in the (double-buffered) observation tensors: read from the previous one
            b.state_in, b.u = N.dptr(si, torch.float32), None
        else:
            b.u = N.dptr(T.get("u"), torch.float32)
        b.beta = N.dptr(T["beta"])                 # float32, or float64 in the reference's mixed-precision mode (P.beta_f64)
        b.beta_stride = 0 if T["beta"].dim() == 1 else T["beta"].stride(0)
        b.action = N.dptr(T["action"])             # float32, or float64 when P.action_kind != ACTION_F32
        b.time_index = N.dptr(T["time_index"], torch.int32)
        b.bsum = N.dptr(T["bsum"], torch.float64)
        b.ring = N.dptr(T["ring"], torch.float32)
        b.obs = N.dptr(T["obs"], torch.float32)
        b.reward = N.dptr(T["reward"], torch.float32)
        b.norm_now = N.dptr(T["norm_now"], torch.float32)
        b.norm_back = N.dptr(T["norm_back"], torch.float32)
        b.terminated = N.dptr(T["terminated"], torch.uint8)
        b.truncated = N.dptr(T["truncated"], torch.uint8)
        b.history = N.dptr(T.get("history"), torch.float32)
        ri, rb = T.get("reset_init"), T.get("reset_beta")
        b.reset_init, b.final_obs = N.dptr(ri, torch.float32), N.dptr(T.get("final_obs"), torch.float32)
        b.reset_beta, b.reset_count = N.dptr(rb, T["beta"].dtype), N.dptr(T.get("reset_count"), torch.int32)
        b.reset_pool_rows = int(ri.shape[0]) if ri is not None else 0
        if rb is not None and (T["beta"].dim() == 1 or rb.shape != ri.shape):
            raise N.NativeError("reset_beta needs a per-instance beta [B, n] and the shape of reset_init")
        return b

    @_on_device_of("bsum")        # (a state tensor: the outputs of a host-facing engine may live in pinned host memory)
    def step1d(self, kind: str, P: N.Params1D, T: dict, B: int):
        import torch
        fn = self.lib.pdegym_transport_step if kind == "transport" else self.lib.pdegym_parabolic_step
        if T["beta"].dtype != (torch.float64 if P.beta_f64 else torch.float32):
            raise N.NativeError(f"beta is {T['beta'].dtype} but params.beta_f64 = {P.beta_f64}")
        if T["action"].dtype != (torch.float32 if P.action_kind == N.ACTION_F32 else torch.float64):
            raise N.NativeError(f"action is {T['action'].dtype} but params.action_kind = {P.action_kind}")
        bufs = self._bufs1d(T)
        N.check(fn(C.byref(P), C.byref(bufs), B, N.current_stream_ptr(T["bsum"].device)), f"pdegym_{kind}_step")

    def prepare_step1d(self, kind: str, P: N.Params1D, T: dict, B: int):
        """The step call with its argument structures built ONCE: returns a zero-argument callable that launches
        pdegym_{kind}_step on the current stream of the state's device.  ``P`` is passed by reference (fields such as
        ``action_kind`` may change between calls); the tensors of ``T`` must stay alive and in place."""
        import torch
        fn = self.lib.pdegym_transport_step if kind == "transport" else self.lib.pdegym_parabolic_step
        if T["beta"].dtype != (torch.float64 if P.beta_f64 else torch.float32):
            raise N.NativeError(f"beta is {T['beta'].dtype} but params.beta_f64 = {P.beta_f64}")
        bufs = self._bufs1d(T)
        dev = T["bsum"].device                     # (outputs may live in pinned host memory: the state names the device)
        return _prepared(fn, C.byref(P), C.byref(bufs), B, dev, f"pdegym_{kind}_step", (bufs, T))
    prepare_step1d.device_guard_key = "bsum"     # the guard is inside the prepared call (the state's device made current)

    @staticmethod
    def _rollout1d_desc(obs, actions, rewards, terminated, truncated, obs_noise=None, obs_seen=None, policy=None) -> N.Rollout1D:
        """The descriptor of a 1D rollout over ``actions.shape[0]`` env-steps, from tensors whose shapes the caller has checked."""
        import torch
        ro = N.Rollout1D()
        ro.T = int(actions.shape[0])
        ro.obs, ro.actions, ro.rewards = N.dptr(obs, torch.float32), N.dptr(actions, torch.float32), N.dptr(rewards, torch.float32)
        ro.terminated, ro.truncated = N.dptr(terminated, torch.uint8), N.dptr(truncated, torch.uint8)
        ro.policy = C.addressof(policy) if policy is not None else None
        ro.obs_noise, ro.obs_seen = N.dptr(obs_noise, torch.float32), N.dptr(obs_seen, torch.float32)
        return ro

    @_on_device_of("obs")
    def rollout1d(self, kind: str, P: N.Params1D, T: dict, obs, actions, rewards, terminated, truncated, B: int, policy=None,
                  obs_noise=None, obs_seen=None, final_obs_steps=None):
        """T env-steps in one launch (pdegym_*_rollout): ``obs`` [T+1, B, obs_dim] (slot 0 = input rows with full-state sensing;
        with scalar sensing the state is ``T["u"]``, advanced in place), ``actions`` / ``rewards`` / ``terminated`` /
        ``truncated`` [T, B].  ``policy``: an ``N.Mlp`` descriptor evaluated inside the launch (``actions`` is then an output;
        its ``noise``, if set, is [T, B]); ``obs_noise`` / ``obs_seen`` [T, B, obs_dim]: the policy reads obs[t] + obs_noise[t],
        which obs_seen[t] receives.  ``final_obs_steps`` [T, B, obs_dim]: row (t, b) receives the last observation of the episode
        that step t ended (no other row is written, and ``T["final_obs"]`` is not)."""
        import torch
        fn = self.lib.pdegym_transport_rollout if kind == "transport" else self.lib.pdegym_parabolic_rollout
        steps = int(actions.shape[0])
        full = P.sensing == N.SENSE_FULL
        od = P.n if full else 1
        _check_shapes("rollout", {"obs": (obs, (steps + 1, B, od)), "actions": (actions, (steps, B)), "rewards": (rewards, (steps, B)),
                                  "terminated": (terminated, (steps, B)), "truncated": (truncated, (steps, B)),
                                  "obs_noise": (obs_noise, (steps, B, od), torch.float32),
                                  "obs_seen": (obs_seen, (steps, B, od), torch.float32)})
        flags = _final_obs_steps("rollout", final_obs_steps, (steps, B, od), torch.float32, obs)
        bufs = self._bufs1d({**T, "state_in": None, "u": None if full else T["u"], "history": None,
                             **({"final_obs": final_obs_steps} if flags else {})})
        ro = self._rollout1d_desc(obs, actions, rewards, terminated, truncated, obs_noise, obs_seen, policy)
        ro.reserved_ = flags
        N.check(fn(C.byref(P), C.byref(bufs), C.byref(ro), B, N.current_stream_ptr(obs.device)), f"pdegym_{kind}_rollout")

    @_on_device_of("bsum")
    def reset1d(self, P: N.Params1D, T: dict, init, mask, B: int):
        import torch
        bufs = self._bufs1d(T)
        m = N.dptr(mask, torch.uint8)
        N.check(self.lib.pdegym_reset1d_masked(C.byref(P), C.byref(bufs), N.dptr(init, torch.float32), m, B,
                                               N.current_stream_ptr(T["bsum"].device)), "pdegym_reset1d_masked")

    @_on_device_of("u")
    def rownorm2(self, rows, out):
        import torch
        B, n = rows.shape
        N.check(self.lib.pdegym_rownorm2_f32(N.dptr(rows, torch.float32), N.dptr(out, torch.float32), n, B,
                                             N.current_stream_ptr(rows.device)), "pdegym_rownorm2_f32")

    # ---- NS2D -----------------------------------------------------------------------------------
    @staticmethod
    def _bufs_ns(T, dtype) -> N.BufsNS2D:
        import torch
        b = N.BufsNS2D()
        for k in ("p", "scratch", "action", "U_ref", "action_ref", "obs", "reward"):
            setattr(b, k, N.dptr(T[k], dtype))
        for k in ("u", "v", "state_in", "p_out", "reset_u0", "reset_v0", "reset_p0", "final_obs"):
            setattr(b, k, N.dptr(T.get(k), dtype))
        b.reset_count = N.dptr(T.get("reset_count"), torch.int32)
        b.reset_pool_rows = int(T["reset_u0"].shape[0]) if T.get("reset_u0") is not None else 0
        b.time_index = N.dptr(T["time_index"], torch.int32)
        b.terminated = N.dptr(T["terminated"], torch.uint8)
        b.nt_ref = int(min(T["U_ref"].shape[0], T["action_ref"].shape[0]))
        return b

    @staticmethod
    def _sfx(dtype):
        import torch
        return "f32" if dtype == torch.float32 else "f64"

    @_on_device_of("p")
    def ns2d_step(self, P: N.ParamsNS2D, T: dict, B: int):
        dtype = T["p"].dtype
        bufs = self._bufs_ns(T, dtype)
        fn = getattr(self.lib, "pdegym_ns2d_step_" + self._sfx(dtype))
        N.check(fn(C.byref(P), C.byref(bufs), B, N.current_stream_ptr(T["p"].device)), "pdegym_ns2d_step")

    def prepare_ns2d_step(self, P: N.ParamsNS2D, T: dict, B: int):
        """pdegym_ns2d_step_* with its argument structures built once (see prepare_step1d): a zero-argument callable."""
        dtype = T["p"].dtype
        bufs = self._bufs_ns(T, dtype)
        fn = getattr(self.lib, "pdegym_ns2d_step_" + self._sfx(dtype))
        return _prepared(fn, C.byref(P), C.byref(bufs), B, T["p"].device, "pdegym_ns2d_step", (bufs, T))
    prepare_ns2d_step.device_guard_key = "p"

    @_on_device_of("p")
    def ns2d_rollout(self, P: N.ParamsNS2D, T: dict, obs, actions, rewards, terminated, B: int):
        """T env-steps in one launch (pdegym_ns2d_rollout_*, small grids): ``obs`` [T+1, B, ny, nx, 2] (slot 0 = the input
        state), ``actions`` [T, B, action_dim], ``rewards`` / ``terminated`` [T, B]."""
        import torch
        dtype = T["p"].dtype
        steps = int(actions.shape[0])
        _check_shapes("rollout", {"obs": (obs, (steps + 1, B, P.ny, P.nx, 2)), "actions": (actions, (steps, B, P.action_dim)),
                                  "rewards": (rewards, (steps, B)), "terminated": (terminated, (steps, B))})
        bufs = self._bufs_ns({**T, "u": None, "v": None, "state_in": None, "p_out": None, "obs": obs[0], "action": actions[0],
                              "reward": rewards[0], "terminated": terminated[0]}, dtype)
        ro = N.RolloutNS2D()
        ro.T = steps
        ro.obs, ro.actions, ro.rewards = N.dptr(obs, dtype), N.dptr(actions, dtype), N.dptr(rewards, dtype)
        ro.terminated = N.dptr(terminated, torch.uint8)
        fn = getattr(self.lib, "pdegym_ns2d_rollout_" + self._sfx(dtype))
        N.check(fn(C.byref(P), C.byref(bufs), C.byref(ro), B, N.current_stream_ptr(T["p"].device)), "pdegym_ns2d_rollout")

    @_on_device_of("p")
    def ns2d_reset(self, P: N.ParamsNS2D, T: dict, u0, v0, p0, mask, B: int):
        import torch
        dtype = T["p"].dtype
        bufs = self._bufs_ns(T, dtype)
        fn = getattr(self.lib, "pdegym_ns2d_reset_masked_" + self._sfx(dtype))
        m = N.dptr(mask, torch.uint8)
        N.check(fn(C.byref(P), C.byref(bufs), N.dptr(u0, dtype), N.dptr(v0, dtype), N.dptr(p0, dtype), m, B,
                   N.current_stream_ptr(T["p"].device)), "pdegym_ns2d_reset_masked")

    @_on_device_of("p")
    def ns2d_solve_pressure(self, P: N.ParamsNS2D, u, v, p_in, p_out, scratch, B: int):
        dtype = u.dtype
        fn = getattr(self.lib, "pdegym_ns2d_solve_pressure_" + self._sfx(dtype))
        N.check(fn(C.byref(P), N.dptr(u, dtype), N.dptr(v, dtype), N.dptr(p_in, dtype), N.dptr(p_out, dtype),
                   N.dptr(scratch, dtype), B, N.current_stream_ptr(u.device)), "pdegym_ns2d_solve_pressure")

    @_on_device_of("p")
    def ns2d_adjoint(self, P: N.ParamsNS2D, T: dict, obs, a_nom, ratio: float, width: float, grad, actions, lam=None, t0: int = 0):
        """The backward march of the adjoint-optimisation baseline in one launch (pdegym_ns2d_adjoint_f64): ``obs``
        [T+1, B, ny, nx, 2] float64 (a forward rollout), ``a_nom`` [T], ``grad`` / ``actions`` [T, B], optional ``lam``
        [T, B, ny, nx, 2]; the targets are ``T["U_ref"]``."""
        import torch
        f64 = torch.float64
        steps, B = int(obs.shape[0]) - 1, int(obs.shape[1])
        _check_shapes("adjoint", {"obs": (obs, (steps + 1, B, P.ny, P.nx, 2)), "a_nom": (a_nom, (steps,)), "grad": (grad, (steps, B)),
                                  "actions": (actions, (steps, B)), "lam": (lam, (steps, B, P.ny, P.nx, 2))})
        a = N.AdjointNS2D()
        a.T, a.t0, a.ratio, a.width = steps, int(t0), float(ratio), float(width)
        a.obs, a.a_nom, a.grad, a.actions = N.dptr(obs, f64), N.dptr(a_nom, f64), N.dptr(grad, f64), N.dptr(actions, f64)
        a.lam = N.dptr(lam, f64)
        N.check(self.lib.pdegym_ns2d_adjoint_f64(C.byref(P), N.dptr(T["U_ref"], f64), int(T["U_ref"].shape[0]), C.byref(a), B,
                                                 N.current_stream_ptr(T["p"].device)), "pdegym_ns2d_adjoint")


    # ---- Traffic ARZ ---------------------------------------------------------------------------
    @staticmethod
    def _bufs_traffic(T) -> N.BufsTraffic:
        import torch
        b = N.BufsTraffic()
        for k in ("r", "y", "action", "time", "rs", "qs_clip", "obs", "reward"):
            setattr(b, k, N.dptr(T[k], torch.float64))
        b.done = N.dptr(T["done"], torch.uint8)
        b.truncated = N.dptr(T["truncated"], torch.uint8)
        b.action_stride = int(T["action"].shape[1]) if T["action"].dim() == 2 else 1
        rr = T.get("reset_rs")
        if rr is not None:           # fused auto-reset (include/pdegym.h)
            b.reset_rs, b.reset_profile = N.dptr(rr, torch.float64), N.dptr(T["reset_profile"], torch.float64)
            b.reset_pool_rows = int(rr.shape[0])
            b.final_obs, b.reset_count = N.dptr(T.get("final_obs"), torch.float64), N.dptr(T.get("reset_count"), torch.int32)
        return b

    @_on_device_of("r")
    def traffic_step(self, P: N.ParamsTraffic, T: dict, B: int):
        bufs = self._bufs_traffic(T)
        N.check(self.lib.pdegym_traffic_step(C.byref(P), C.byref(bufs), B, N.current_stream_ptr(T["r"].device)),
                "pdegym_traffic_step")

    @staticmethod
    def _rollout_traffic_desc(obs, actions, rewards, done, truncated, policy=None) -> N.RolloutTraffic:
        """The descriptor of a traffic rollout over ``actions.shape[0]`` env-steps, from tensors whose shapes the caller has checked."""
        import torch
        ro = N.RolloutTraffic()
        ro.T = int(actions.shape[0])
        ro.obs, ro.actions, ro.rewards = N.dptr(obs, torch.float64), N.dptr(actions, torch.float64), N.dptr(rewards, torch.float64)
        ro.done, ro.truncated = N.dptr(done, torch.uint8), N.dptr(truncated, torch.uint8)
        ro.policy = C.addressof(policy) if policy is not None else None
        return ro

    @_on_device_of("r")
    def traffic_rollout(self, P: N.ParamsTraffic, T: dict, obs, actions, rewards, done, truncated, B: int, policy=None,
                        final_obs_steps=None):
        """T env-steps in one launch (pdegym_traffic_rollout): ``obs`` [T+1, B, 2M], ``actions`` [T, B, A] (A = 1 or 2; an output
        when ``policy`` -- an ``N.Mlp`` descriptor, its ``noise`` [T, B, A] -- is given), ``rewards`` / ``done`` / ``truncated`` [T, B].
        ``final_obs_steps`` float64 [T, B, 2M]: row (t, b) receives the last observation of the episode that step t ended (no other
        row is written, and ``T["final_obs"]`` is not)."""
        import torch
        steps = int(actions.shape[0])
        A = int(actions.shape[2])
        if A not in (1, 2):
            raise N.NativeError(f"rollout actions must be a contiguous [{steps}, {B}, 1 or 2] tensor, got {tuple(actions.shape)}")
        _check_shapes("rollout", {"obs": (obs, (steps + 1, B, 2 * P.M)), "actions": (actions, (steps, B, A)), "rewards": (rewards, (steps, B)),
                                  "done": (done, (steps, B)), "truncated": (truncated, (steps, B))})
        flags = _final_obs_steps("rollout", final_obs_steps, (steps, B, 2 * P.M), torch.float64, obs)
        bufs = self._bufs_traffic({**T, "action": actions[0], **({"final_obs": final_obs_steps} if flags else {})})
        ro = self._rollout_traffic_desc(obs, actions, rewards, done, truncated, policy)
        ro.reserved_ = flags
        N.check(self.lib.pdegym_traffic_rollout(C.byref(P), C.byref(bufs), C.byref(ro), B, N.current_stream_ptr(obs.device)),
                "pdegym_traffic_rollout")

    @_on_device_of("obs")
    def traffic_backstep_control(self, P: N.ParamsTraffic, obs, rs, out, law: N.TrafficBackstep):
        """out[b] = the backstepping command(s) for observation row obs[b] (pdegym_traffic_backstep_control): ``obs`` float64
        [B, 2M] (row stride = stride(0)), ``rs`` float64 [B], ``out`` float64 [B] / [B, 1] ([B, 2] for 'both'); ``law``: an
        ``N.TrafficBackstep`` descriptor with the weight rows, the order, ``noise`` [B, commands] and the clamp
        (what ``TrafficBacksteppingController.forward_into`` builds)."""
        import torch
        if obs.dim() != 2 or obs.stride(1) != 1 or obs.dtype != torch.float64 or not obs.is_cuda or obs.shape[1] != 2 * P.M:
            raise N.NativeError(f"traffic_backstep_control: obs must be a float64 HIP tensor [B, {2 * P.M}] with unit inner stride")
        B = int(obs.shape[0])
        ncmd = 2 if P.sim == N.TRAFFIC_SIM["both"] else 1
        if out.dtype != torch.float64 or out.numel() != B * ncmd or not out.is_contiguous():
            raise N.NativeError(f"traffic_backstep_control: out must be a contiguous float64 tensor of {B} x {ncmd} commands")
        if rs.numel() != B:
            raise N.NativeError(f"traffic_backstep_control: rs must have {B} elements")
        N.check(self.lib.pdegym_traffic_backstep_control(C.byref(P), C.byref(law), obs.data_ptr(), obs.stride(0), N.dptr(rs, torch.float64),
                                                         N.dptr(out, torch.float64), ncmd, B, N.current_stream_ptr(obs.device)),
                "pdegym_traffic_backstep_control")

    @_on_device_of("r")
    def traffic_backstep_rollout(self, P: N.ParamsTraffic, T: dict, obs, actions, rewards, done, truncated, B: int, law: N.TrafficBackstep,
                                 final_obs_steps=None):
        """T env-steps with the backstepping law inside, in one launch (pdegym_traffic_backstep_rollout): the buffers of
        ``traffic_rollout`` with ``actions`` [T, B, commands] an output; ``law``: an ``N.TrafficBackstep`` descriptor
        (``TrafficBacksteppingController.rollout_law``; its ``noise`` [T, B, commands]); ``final_obs_steps`` as there."""
        import torch
        steps = int(actions.shape[0])
        A = 2 if P.sim == N.TRAFFIC_SIM["both"] else 1
        _check_shapes("backstep rollout", {"obs": (obs, (steps + 1, B, 2 * P.M)), "actions": (actions, (steps, B, A)),
                                           "rewards": (rewards, (steps, B)), "done": (done, (steps, B)), "truncated": (truncated, (steps, B))})
        flags = _final_obs_steps("backstep rollout", final_obs_steps, (steps, B, 2 * P.M), torch.float64, obs)
        bufs = self._bufs_traffic({**T, "action": actions[0], **({"final_obs": final_obs_steps} if flags else {})})
        ro = self._rollout_traffic_desc(obs, actions, rewards, done, truncated)
        ro.reserved_ = flags
        N.check(self.lib.pdegym_traffic_backstep_rollout(C.byref(P), C.byref(bufs), C.byref(ro), C.byref(law), B,
                                                         N.current_stream_ptr(obs.device)), "pdegym_traffic_backstep_rollout")

    @_on_device_of("r")
    def traffic_reset(self, P: N.ParamsTraffic, T: dict, profile, mask, B: int):
        import torch
        bufs = self._bufs_traffic(T)
        m = N.dptr(mask, torch.uint8)
        N.check(self.lib.pdegym_traffic_reset_masked(C.byref(P), C.byref(bufs), N.dptr(profile, torch.float64), m, B,
                                                     N.current_stream_ptr(T["r"].device)), "pdegym_traffic_reset_masked")

    # ---- Brain tumour --------------------------------------------------------------------------
    @staticmethod
    def _bufs_tumor(T) -> N.BufsTumor:
        import torch
        b = N.BufsTumor()
        for k in ("u", "xscale", "control", "remaining", "t_benchmark", "reward", "out"):
            setattr(b, k, N.dptr(T[k], torch.float64))
        b.kill = N.dptr(T.get("kill"), torch.float64)
        for k in ("time_index", "stage", "days"):
            setattr(b, k, N.dptr(T[k], torch.int32))
        b.terminated = N.dptr(T["terminated"], torch.uint8)
        b.truncated = N.dptr(T["truncated"], torch.uint8)
        b.active = N.dptr(T.get("active"), torch.uint8)
        b.history, b.t1_log = N.dptr(T.get("history"), torch.float64), N.dptr(T.get("t1_log"), torch.float64)
        return b

    @_on_device_of("u")
    def tumor_advance(self, P: N.ParamsTumor, T: dict, mode: int, max_days: int, B: int):
        bufs = self._bufs_tumor(T)
        N.check(self.lib.pdegym_tumor_advance(C.byref(P), C.byref(bufs), mode, max_days, B, N.current_stream_ptr(T["u"].device)),
                "pdegym_tumor_advance")

    @_on_device_of("u")
    def tumor_step(self, P: N.ParamsTumor, T: dict, B: int):
        bufs = self._bufs_tumor(T)
        N.check(self.lib.pdegym_tumor_step(C.byref(P), C.byref(bufs), B, N.current_stream_ptr(T["u"].device)),
                "pdegym_tumor_step")

    @_on_device_of("u")
    def tumor_reset(self, P: N.ParamsTumor, T: dict, init, mask, B: int):
        import torch
        bufs = self._bufs_tumor(T)
        m = N.dptr(mask, torch.uint8)
        stride = 0 if init.dim() == 1 else init.shape[-1]
        N.check(self.lib.pdegym_tumor_reset_masked(C.byref(P), C.byref(bufs), N.dptr(init, torch.float64), stride, m, B,
                                                   N.current_stream_ptr(T["u"].device)), "pdegym_tumor_reset_masked")

    @staticmethod
    def _wrap_tumor(T, W: dict, B: int) -> N.WrapTumor:
        """``W``: the wrapper's state -- ``weekends``, ``init`` [nx] or [B, nx], ``consecutive`` int32 [B], ``treatment_calls`` /
        ``soft_constraint_violations`` int64 [B], optional ``final_obs`` / ``obs`` [B, nx]."""
        import torch
        nx = int(T["u"].shape[1])
        init = W["init"]
        if tuple(init.shape) not in ((nx,), (B, nx)):
            raise N.NativeError(f"tumor wrapper: init must be [{nx}] or [{B}, {nx}], got {tuple(init.shape)}")
        _check_shapes("tumor wrapper", {"consecutive": (W["consecutive"], (B,)), "treatment_calls": (W["treatment_calls"], (B,)),
                                        "soft_constraint_violations": (W["soft_constraint_violations"], (B,)),
                                        "final_obs": (W.get("final_obs"), (B, nx)), "obs": (W.get("obs"), (B, nx))})
        w = N.WrapTumor()
        w.weekends = int(bool(W["weekends"]))
        w.init, w.init_stride = N.dptr(init, torch.float64), (0 if init.dim() == 1 else nx)
        w.consecutive = N.dptr(W["consecutive"], torch.int32)
        w.treatment_calls = N.dptr(W["treatment_calls"], torch.int64)
        w.soft_constraint_violations = N.dptr(W["soft_constraint_violations"], torch.int64)
        w.final_obs, w.obs = N.dptr(W.get("final_obs"), torch.float64), N.dptr(W.get("obs"), torch.float64)
        return w

    @_on_device_of("u")
    def tumor_therapy_step(self, P: N.ParamsTumor, T: dict, W: dict, B: int):
        """One TherapyWrapper step of every patient in one launch (pdegym_tumor_therapy_step): the command is ``T["control"]``, the
        wrapper's state ``W`` (``_wrap_tumor``); ``W["obs"]`` receives the returned observation."""
        bufs = self._bufs_tumor({**T, "kill": None, "active": None})
        wrap = self._wrap_tumor(T, W, B)
        N.check(self.lib.pdegym_tumor_therapy_step(C.byref(P), C.byref(bufs), C.byref(wrap), B, N.current_stream_ptr(T["u"].device)),
                "pdegym_tumor_therapy_step")

    @_on_device_of("u")
    def tumor_rollout(self, P: N.ParamsTumor, T: dict, W: dict, obs, actions, rewards, terminated, truncated, B: int, policy=None,
                      final_obs_steps=None):
        """T wrapper steps in one launch (pdegym_tumor_rollout): ``obs`` [T+1, B, nx], ``actions`` [T, B] (an output when ``policy`` --
        an ``N.Mlp`` descriptor, its ``noise`` [T, B] -- is given), ``rewards`` / ``terminated`` / ``truncated`` [T, B].
        ``final_obs_steps`` float64 [T, B, nx]: row (t, b) receives the last row of the episode that step t ended (no other row is
        written, and ``W["final_obs"]`` is not)."""
        import torch
        steps = int(actions.shape[0])
        _check_shapes("rollout", {"obs": (obs, (steps + 1, B, P.nx)), "actions": (actions, (steps, B)), "rewards": (rewards, (steps, B)),
                                  "terminated": (terminated, (steps, B)), "truncated": (truncated, (steps, B))})
        bufs = self._bufs_tumor({**T, "kill": None, "active": None})
        flags = _final_obs_steps("rollout", final_obs_steps, (steps, B, P.nx), torch.float64, obs)
        wrap = self._wrap_tumor(T, {**W, "obs": None, **({"final_obs": None} if flags else {})}, B)
        if flags:
            wrap.final_obs = N.dptr(final_obs_steps, torch.float64)
        ro = N.RolloutTumor()
        ro.T, ro.reserved_ = steps, flags
        ro.obs, ro.actions, ro.rewards = N.dptr(obs, torch.float64), N.dptr(actions, torch.float64), N.dptr(rewards, torch.float64)
        ro.terminated, ro.truncated = N.dptr(terminated, torch.uint8), N.dptr(truncated, torch.uint8)
        ro.policy = C.addressof(policy) if policy is not None else None
        N.check(self.lib.pdegym_tumor_rollout(C.byref(P), C.byref(bufs), C.byref(wrap), C.byref(ro), B, N.current_stream_ptr(obs.device)),
                "pdegym_tumor_rollout")

    # ---- policy network ----------------------------------------------------------------------------
    @_on_device_of("x")
    def mlp_forward(self, net: N.Mlp, x, y, B: int, rows=None, rows_not=None):
        """y[b] = net(x[b]) for b < B: x [B, in_dim], y [B, out_dim] rows (row stride = stride(0)); float32, or float64 with
        net.x_f64 / net.y_f64 set (the caller sets them from the tensors' dtypes).  ``rows`` (uint8 [B], with ``rows_not`` uint8 [B] or
        None): pdegym_mlp_forward_masked -- only rows with rows[b] != 0 and rows_not[b] == 0 are evaluated and stored, the others of
        ``y`` are left as they are."""
        import torch
        for t_, name, f64 in ((x, "x", net.x_f64), (y, "y", net.y_f64)):
            want = torch.float64 if f64 else torch.float32
            if not t_.is_cuda or t_.dtype != want or t_.dim() != 2 or t_.stride(1) != 1:
                raise N.NativeError(f"mlp_forward: {name} must be a {want} HIP tensor [B, width] with unit inner stride")
        if rows is None and rows_not is not None:
            raise N.NativeError("mlp_forward: rows_not knocks rows out of `rows`, which is missing")
        if rows is not None:
            _check_shapes("mlp_forward", {"rows": (rows, (B,), torch.uint8), "rows_not": (rows_not, (B,), torch.uint8)})
            for m, name in ((rows, "rows"), (rows_not, "rows_not")):
                if m is not None and m.device != x.device:
                    raise N.NativeError(f"mlp_forward: {name} must live on {x.device}, got {m.device}")
            N.check(self.lib.pdegym_mlp_forward_masked(C.byref(net), x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0),
                                                       N.dptr(rows, torch.uint8), N.dptr(rows_not, torch.uint8), B,
                                                       N.current_stream_ptr(x.device)), "pdegym_mlp_forward_masked")
            return
        N.check(self.lib.pdegym_mlp_forward(C.byref(net), x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), B,
                                            N.current_stream_ptr(x.device)), "pdegym_mlp_forward")

    @_on_device_of("x")
    def mlp_backward(self, net: N.Mlp, x, dy, weights, dw, db, dx=None, slabs: int = 0):
        """Gradients of the network ``net`` describes (plain head, no clamp, no noise) for ``dy`` = dLoss/dy, in three launches
        (pdegym_mlp_backward): ``x`` [B, in_dim] float32 or float64 (``net.x_f64`` set by the caller), ``dy`` [B, out_dim] float32, both
        with unit inner stride; ``weights[l]`` the contiguous row-major [out, in] float32 weights of layer l (``Linear.weight``);
        ``dw[l]`` / ``db[l]`` (None where the layer has no bias) contiguous float32 outputs of the parameters' shapes, written, not
        accumulated; ``dx`` [B, in_dim] float32 or None.  ``slabs``: include/pdegym.h (0: the library's choice).  The workspace is
        the backend's own, cached per (device, size)."""
        self._mlp_backward_call("mlp_backward", self._mlp_backward_workspace, net, x, dy, weights, dw, db, dx, slabs)

    @_on_device_of("x")
    def mlp_backward_wide(self, net: N.Mlp, x, dy, weights, dw, db, dx=None, slabs: int = 0):
        """``mlp_backward`` for layers of up to 256 units (pdegym_mlp_backward_wide: the tile launch, one accumulation launch over
        every layer's dZ^T H, the slab reduction): the same arguments, checked the same way, and on a network both take with the
        same explicit ``slabs`` the same bits.  ``slabs`` = 0 is this entry's own choice (include/pdegym.h).  Its workspace is a
        cache of its own, per (device, size)."""
        self._mlp_backward_call("mlp_backward_wide", self._mlp_backward_wide_workspace, net, x, dy, weights, dw, db, dx, slabs)

    def _mlp_backward_call(self, entry: str, workspace, net, x, dy, weights, dw, db, dx, slabs):
        """The argument checks and the call of ``pdegym_<entry>`` (``entry``: mlp_backward / mlp_backward_wide; one argument structure)."""
        import torch
        query, call = getattr(self.lib, f"pdegym_{entry}_workspace"), getattr(self.lib, f"pdegym_{entry}")
        B, nl = int(x.shape[0]) if x.dim() == 2 else -1, int(net.n_layers)
        want_x = torch.float64 if net.x_f64 else torch.float32
        rows = (("x", x, want_x, int(net.layer[0].in_dim)), ("dy", dy, torch.float32, int(net.layer[nl - 1].out_dim)),
                ("dx", dx, torch.float32, int(net.layer[0].in_dim)))
        for name, t_, dtype, width in rows:
            if t_ is None and name == "dx":
                continue
            if (not torch.is_tensor(t_) or not t_.is_cuda or t_.device != x.device or t_.dtype != dtype or t_.dim() != 2
                    or tuple(t_.shape) != (B, width) or (width > 1 and t_.stride(1) != 1) or (B > 1 and t_.stride(0) < width)):
                raise N.NativeError(f"{entry}: {name} must be a {dtype} HIP tensor [{B}, {width}] with unit inner stride on x's device")
        if not (len(weights) == len(dw) == len(db) == nl):
            raise N.NativeError(f"{entry}: weights, dw and db must have one entry per layer ({nl})")
        a = N.MlpBackward()
        for l in range(nl):
            shape = (int(net.layer[l].out_dim), int(net.layer[l].in_dim))
            for name, t_, shp in (("weights", weights[l], shape), ("dw", dw[l], shape), ("db", db[l], shape[:1])):
                if t_ is None and name == "db":
                    continue
                if (not torch.is_tensor(t_) or not t_.is_cuda or t_.device != x.device or t_.dtype != torch.float32
                        or tuple(t_.shape) != shp or not t_.is_contiguous()):
                    raise N.NativeError(f"{entry}: {name}[{l}] must be a contiguous float32 HIP tensor {shp} on x's device")
            a.w[l], a.dw[l], a.db[l] = weights[l].data_ptr(), dw[l].data_ptr(), (None if db[l] is None else db[l].data_ptr())
        need = int(query(C.byref(net), B, int(slabs)))
        if need < 0:
            N.check(need, f"pdegym_{entry}_workspace")
        ws = workspace(x.device, need)
        a.x, a.x_stride, a.dy, a.dy_stride = x.data_ptr(), (x.stride(0) if B > 1 else x.shape[1]), dy.data_ptr(), (dy.stride(0) if B > 1 else dy.shape[1])
        if dx is not None:
            a.dx, a.dx_stride = dx.data_ptr(), (dx.stride(0) if B > 1 else dx.shape[1])
        a.slabs, a.workspace, a.workspace_bytes = int(slabs), ws.data_ptr(), ws.numel()
        N.check(call(C.byref(net), C.byref(a), B, N.current_stream_ptr(x.device)), f"pdegym_{entry}")

    @_on_device_of("x")
    def mlp_forward_cat(self, net: N.Mlp, x, x2, y, B: int):
        """``mlp_forward`` on rows in two parts (pdegym_mlp_forward_cat): row b is ``[x[b] | x2[b]]``, ``x`` [B, D] float32 or float64
        (``net.x_f64``), ``x2`` [B, n2] float32 with 1 <= n2 <= 8 and D + n2 == the first layer's in_dim; the bits of ``mlp_forward`` on
        the concatenated rows, without the concatenation."""
        import torch
        for t_, name, want in ((x, "x", torch.float64 if net.x_f64 else torch.float32), (x2, "x2", torch.float32),
                               (y, "y", torch.float64 if net.y_f64 else torch.float32)):
            if (not torch.is_tensor(t_) or not t_.is_cuda or t_.device != x.device or t_.dtype != want or t_.dim() != 2
                    or t_.shape[0] != B or t_.stride(1) != 1):
                raise N.NativeError(f"mlp_forward_cat: {name} must be a {want} HIP tensor [{B}, width] with unit inner stride on x's device")
        n2 = int(x2.shape[1])
        if int(x.shape[1]) + n2 != int(net.layer[0].in_dim):
            raise N.NativeError(f"mlp_forward_cat: x has {int(x.shape[1])} columns and x2 {n2}, the network takes {int(net.layer[0].in_dim)}")
        stride = lambda t_: t_.stride(0) if B > 1 else t_.shape[1]      # noqa: E731
        N.check(self.lib.pdegym_mlp_forward_cat(C.byref(net), x.data_ptr(), stride(x), x2.data_ptr(), stride(x2), n2, y.data_ptr(), stride(y),
                                                B, N.current_stream_ptr(x.device)), "pdegym_mlp_forward_cat")

    @staticmethod
    def _mlp_gather_desc(entry: str, x, x2, index, x2_indexed: bool, B: int) -> N.MlpGather:
        """The checks of ``index`` and the descriptor of the gather calls: ``index`` a contiguous int64 HIP tensor [B] on x's device."""
        import torch
        if (not torch.is_tensor(index) or not index.is_cuda or index.device != x.device or index.dtype != torch.int64 or index.dim() != 1
                or index.shape[0] != B or not index.is_contiguous()):
            raise N.NativeError(f"{entry}: index must be a contiguous int64 HIP tensor [{B}] on x's device")
        if x2_indexed and (x2 is None or x2.shape[0] != x.shape[0]):
            raise N.NativeError(f"{entry}: x2_indexed needs x2 with the {int(x.shape[0])} rows of x")
        g = N.MlpGather()
        g.index, g.M, g.x2_indexed = index.data_ptr(), int(x.shape[0]), int(bool(x2_indexed))
        return g

    @_on_device_of("x")
    def mlp_forward_gather(self, net: N.Mlp, x, x2, index, y, B: int, x2_indexed: bool = False):
        """``mlp_forward`` / ``mlp_forward_cat`` on rows read by index (pdegym_mlp_forward_gather): row b is
        ``[x[index[b]] | x2[index[b] if x2_indexed else b]]``, ``x`` the [M, D] storage (float32, or float64 with ``net.x_f64``), ``x2``
        [B, n2] (or [M, n2] with ``x2_indexed``) float32 or None (the plain row), ``index`` int64 [B], ``y`` [B, out].  The bits of the
        call on the materialised rows; an index entry outside [0, M) gives a NaN row and is never an address."""
        import torch
        M = int(x.shape[0]) if torch.is_tensor(x) and x.dim() == 2 else -1
        for t_, name, want, rows in ((x, "x", torch.float64 if net.x_f64 else torch.float32, M),
                                     (x2, "x2", torch.float32, M if x2_indexed else B),
                                     (y, "y", torch.float64 if net.y_f64 else torch.float32, B)):
            if t_ is None and name == "x2":
                continue
            if (not torch.is_tensor(t_) or not t_.is_cuda or t_.device != x.device or t_.dtype != want or t_.dim() != 2
                    or t_.shape[0] != rows or t_.stride(1) != 1 or rows < 1):
                raise N.NativeError(f"mlp_forward_gather: {name} must be a {want} HIP tensor [{rows}, width] with unit inner stride on x's device")
        n2 = 0 if x2 is None else int(x2.shape[1])
        if int(x.shape[1]) + n2 != int(net.layer[0].in_dim):
            raise N.NativeError(f"mlp_forward_gather: x has {int(x.shape[1])} columns and x2 {n2}, the network takes {int(net.layer[0].in_dim)}")
        g = self._mlp_gather_desc("mlp_forward_gather", x, x2, index, x2_indexed, B)
        stride = lambda t_: t_.stride(0) if t_.shape[0] > 1 else t_.shape[1]      # noqa: E731
        N.check(self.lib.pdegym_mlp_forward_gather(C.byref(net), x.data_ptr(), stride(x), (None if x2 is None else x2.data_ptr()),
                                                   (0 if x2 is None else stride(x2)), n2, C.byref(g), y.data_ptr(), stride(y), B,
                                                   N.current_stream_ptr(x.device)), "pdegym_mlp_forward_gather")

    @_on_device_of("x")
    def mlp_backward_gather(self, net: N.Mlp, x, x2, index, dy, weights, dw=None, db=None, dx2=None, params: bool = True, slabs: int = 0,
                            wide: bool = False, x2_indexed: bool = False):
        """``mlp_backward_cat`` on rows read by index (pdegym_mlp_backward_gather / _wide_gather): ``x`` the [M, D] storage, ``x2``
        [B, n2] (or [M, n2] with ``x2_indexed``) or None, ``index`` int64 [B], ``dy`` [B, out].  No ``dx`` (a gradient of gathered rows is
        a scatter-add); ``dx2`` [B, n2] only without ``x2_indexed``.  Bits: those of ``mlp_backward_cat`` on the materialised rows."""
        self._mlp_backward_cat_call(net, x, x2, dy, weights, dw, db, None, dx2, params, slabs, wide, index=index, x2_indexed=x2_indexed)

    @_on_device_of("x")
    def mlp_backward_cat(self, net: N.Mlp, x, x2, dy, weights, dw=None, db=None, dx=None, dx2=None, params: bool = True,
                         slabs: int = 0, wide: bool = False):
        """``mlp_backward`` (``wide``: ``mlp_backward_wide``) on rows in two parts (pdegym_mlp_backward_cat / _wide_cat): ``x`` [B, D],
        ``x2`` [B, n2] float32 or None (n2 = 0: the plain row), ``dx`` [B, D] and ``dx2`` [B, n2] float32 or None.  ``params`` true:
        the three launches, ``dw`` / ``db`` as for ``mlp_backward``; false: ONE launch for ``dx`` / ``dx2`` alone -- ``dw`` and ``db``
        must be None (or lists of None), no workspace is touched.  Bits: those of the shadowed pass on the concatenated rows."""
        self._mlp_backward_cat_call(net, x, x2, dy, weights, dw, db, dx, dx2, params, slabs, wide)

    def _mlp_backward_cat_call(self, net, x, x2, dy, weights, dw, db, dx, dx2, params, slabs, wide, index=None, x2_indexed=False):
        """The argument checks and the call of pdegym_mlp_backward[_wide]_cat, or with ``index`` of pdegym_mlp_backward[_wide]_gather
        (one argument structure; ``x`` then has M rows, ``x2`` M with ``x2_indexed``, everything else the B of ``dy``)."""
        import torch
        gather = index is not None
        entry = ("mlp_backward_wide" if wide else "mlp_backward") + ("_gather" if gather else "_cat")
        M = int(x.shape[0]) if x.dim() == 2 else -1
        B, nl = (int(dy.shape[0]) if torch.is_tensor(dy) and dy.dim() == 2 else -1) if gather else M, int(net.n_layers)
        n2 = 0 if x2 is None else (int(x2.shape[1]) if torch.is_tensor(x2) and x2.dim() == 2 else -1)
        D = int(net.layer[0].in_dim) - n2
        want_x = torch.float64 if net.x_f64 else torch.float32
        rows = (("x", x, want_x, D, M), ("x2", x2, torch.float32, n2, M if x2_indexed else B),
                ("dy", dy, torch.float32, int(net.layer[nl - 1].out_dim), B), ("dx", dx, torch.float32, D, B), ("dx2", dx2, torch.float32, n2, B))
        for name, t_, dtype, width, n in rows:
            if t_ is None and name in ("x2", "dx", "dx2"):
                continue
            if (not torch.is_tensor(t_) or not t_.is_cuda or t_.device != x.device or t_.dtype != dtype or t_.dim() != 2
                    or tuple(t_.shape) != (n, width) or (width > 1 and t_.stride(1) != 1) or (n > 1 and t_.stride(0) < width)):
                raise N.NativeError(f"{entry}: {name} must be a {dtype} HIP tensor [{n}, {width}] with unit inner stride on x's device")
        g = self._mlp_gather_desc(entry, x, x2, index, x2_indexed, B) if gather else None
        dw = [None] * nl if dw is None else dw
        db = [None] * nl if db is None else db
        if not (len(weights) == len(dw) == len(db) == nl):
            raise N.NativeError(f"{entry}: weights, dw and db must have one entry per layer ({nl})")
        if not params and any(t_ is not None for t_ in list(dw) + list(db)):
            raise N.NativeError(f"{entry}: params=False takes no dw and no db")
        a = N.MlpBackwardCat()
        for l in range(nl):
            shape = (int(net.layer[l].out_dim), int(net.layer[l].in_dim))
            for name, t_, shp in (("weights", weights[l], shape), ("dw", dw[l], shape), ("db", db[l], shape[:1])):
                if t_ is None and (name == "db" or not params):
                    continue
                if (not torch.is_tensor(t_) or not t_.is_cuda or t_.device != x.device or t_.dtype != torch.float32
                        or tuple(t_.shape) != shp or not t_.is_contiguous()):
                    raise N.NativeError(f"{entry}: {name}[{l}] must be a contiguous float32 HIP tensor {shp} on x's device")
            a.w[l] = weights[l].data_ptr()
            a.dw[l], a.db[l] = (None if dw[l] is None else dw[l].data_ptr()), (None if db[l] is None else db[l].data_ptr())
        stride = lambda t_: t_.stride(0) if t_.shape[0] > 1 else t_.shape[1]      # noqa: E731
        a.x, a.x_stride, a.dy, a.dy_stride = x.data_ptr(), stride(x), dy.data_ptr(), stride(dy)
        if x2 is not None:
            a.x2, a.x2_stride, a.n2 = x2.data_ptr(), stride(x2), n2
        if dx is not None:
            a.dx, a.dx_stride = dx.data_ptr(), stride(dx)
        if dx2 is not None:
            a.dx2, a.dx2_stride = dx2.data_ptr(), stride(dx2)
        a.params, a.slabs = int(bool(params)), int(slabs)
        if params:
            shadowed = "mlp_backward_wide" if wide else "mlp_backward"
            need = int(getattr(self.lib, f"pdegym_{shadowed}_workspace")(C.byref(net), B, int(slabs)))
            if need < 0:
                N.check(need, f"pdegym_{shadowed}_workspace")
            ws = (self._mlp_backward_wide_workspace if wide else self._mlp_backward_workspace)(x.device, need)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        extra = (C.byref(g),) if gather else ()
        N.check(getattr(self.lib, f"pdegym_{entry}")(C.byref(net), C.byref(a), *extra, B, N.current_stream_ptr(x.device)), f"pdegym_{entry}")

    def _mlp_backward_workspace(self, device, nbytes: int):
        """The workspace of ``mlp_backward``: one uint8 tensor per (device, size), kept (every launch of one stream uses it in turn)."""
        import torch
        cache = self.__dict__.setdefault("_mlp_bw_ws", {})
        key = (device.index, nbytes)
        if key not in cache:
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return cache[key]

    def _mlp_backward_wide_workspace(self, device, nbytes: int):
        """The workspace of ``mlp_backward_wide``, kept apart from ``mlp_backward``'s: one uint8 tensor per (device, size)."""
        import torch
        cache = self.__dict__.setdefault("_mlp_bw_wide_ws", {})
        key = (device.index, nbytes)
        if key not in cache:
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return cache[key]

    # ---- backstepping baseline -------------------------------------------------------------------
    @_on_device_of("theta")
    def backstep_gain(self, kind: str, theta, gain, dx: float):
        """gain[r] = backstepping gain of theta[r] (pdegym_backstep_gain_*): ``theta`` float32 [R, m], ``gain`` float64 [R, m],
        ``dx`` the Python double."""
        import torch
        fn = self.lib.pdegym_backstep_gain_transport if kind == "transport" else self.lib.pdegym_backstep_gain_parabolic
        if theta.dim() != 2 or tuple(gain.shape) != tuple(theta.shape):
            raise N.NativeError(f"backstep_gain: theta and gain must both be [R, m], got {tuple(theta.shape)} and {tuple(gain.shape)}")
        R, m = theta.shape
        N.check(fn(N.dptr(theta, torch.float32), N.dptr(gain, torch.float64), R, m, float(dx), N.current_stream_ptr(theta.device)),
                f"pdegym_backstep_gain_{kind}")

    @_on_device_of("obs")
    def backstep_control(self, obs, out, gain0, length: int, scale: float, ordered: bool = False, gain_pool=None, reset_count=None,
                         noise=None, clamp=None):
        """out[b] = (sum_{i<length} gain_row(b)[i] * obs[b, i]) * scale (pdegym_backstep_control): ``obs`` float32 [B, >= length]
        (row stride = stride(0)), ``gain0`` float64 [B, m] or [m] (shared), ``out`` float64 [B], or float32 [B] (+ ``noise`` [B],
        clamped to ``clamp`` = (lo, hi)); ``gain_pool`` [P, m] + ``reset_count`` int32 [B]: see include/pdegym.h."""
        import torch
        if obs.dim() != 2 or obs.stride(1) != 1 or obs.dtype != torch.float32 or not obs.is_cuda:
            raise N.NativeError("backstep_control: obs must be a float32 HIP tensor [B, width] with unit inner stride")
        B = int(obs.shape[0])
        if out.dtype not in (torch.float32, torch.float64) or out.numel() != B:
            raise N.NativeError(f"backstep_control: out must be a float32 or float64 tensor of {B} elements")
        if gain0.dim() == 2 and gain0.shape[0] != B:
            raise N.NativeError(f"backstep_control: {gain0.shape[0]} gain rows for {B} instances")
        c = N.Backstep()
        c.gain0, c.gain_stride, c.m = N.dptr(gain0, torch.float64), (0 if gain0.dim() == 1 else gain0.stride(0)), int(gain0.shape[-1])
        if gain_pool is not None:
            if gain_pool.dim() != 2 or gain_pool.shape[1] != c.m or reset_count is None or reset_count.numel() != B:
                raise N.NativeError("backstep_control: gain_pool must be [P, m] and come with reset_count [B]")
            c.gain_pool, c.pool_rows = N.dptr(gain_pool, torch.float64), int(gain_pool.shape[0])
            c.reset_count = N.dptr(reset_count, torch.int32)
        c.obs, c.obs_stride, c.len = obs.data_ptr(), obs.stride(0), int(length)
        c.order, c.scale = (N.BACKSTEP_ORDERED if ordered else N.BACKSTEP_TREE), float(scale)
        if out.dtype == torch.float64:
            c.out64 = N.dptr(out, torch.float64)
        else:
            c.out32 = N.dptr(out, torch.float32)
        if noise is not None:
            if noise.numel() != B:
                raise N.NativeError(f"backstep_control: noise must have {B} elements")
            c.noise = N.dptr(noise, torch.float32)
        if clamp is not None:
            c.clamp, c.lo, c.hi = 1, float(clamp[0]), float(clamp[1])
        N.check(self.lib.pdegym_backstep_control(C.byref(c), B, N.current_stream_ptr(obs.device)), "pdegym_backstep_control")

    @_on_device_of("rewards")
    def gae(self, rewards, values, terminated, truncated, advantages, returns, gamma: float, gae_lambda: float, boot=None,
            ep_return_acc=None, ep_length_acc=None, episode_return=None, episode_length=None):
        """GAE(lambda) advantages and returns of a rollout, and optionally its episode statistics, in one launch (pdegym_gae: SB3's
        ``compute_returns_and_advantage``, bit for bit).  ``rewards`` [T, B] float32 or float64, ``values`` [T + 1, B] float32,
        ``terminated`` / ``truncated`` (or None) / ``boot`` (or None) [T, B]; outputs ``advantages`` / ``returns`` [T, B] float32,
        ``episode_return`` float64 / ``episode_length`` int32 [T, B] with the accumulators ``ep_return_acc`` float64 /
        ``ep_length_acc`` int32 [B].  Every 2-D tensor has unit inner stride and the SAME row stride ``ld = stride(0)`` (column
        shards of a wider batch are plain views); ``gamma`` / ``gae_lambda``: the Python doubles."""
        import torch
        if rewards.dim() != 2 or rewards.dtype not in (torch.float32, torch.float64):
            raise N.NativeError("gae: rewards must be a float32 or float64 [T, B] tensor")
        T, B = (int(s) for s in rewards.shape)
        ld = int(rewards.stride(0)) if T > 1 else max(int(values.stride(0)), B)
        wanted = {"rewards": (rewards, T, rewards.dtype), "values": (values, T + 1, torch.float32),
                  "terminated": (terminated, T, torch.uint8), "truncated": (truncated, T, torch.uint8), "boot": (boot, T, torch.float32),
                  "advantages": (advantages, T, torch.float32), "returns": (returns, T, torch.float32),
                  "episode_return": (episode_return, T, torch.float64), "episode_length": (episode_length, T, torch.int32)}
        for name, (x, rows, dtype) in wanted.items():
            if x is None:
                if name in ("truncated", "boot", "episode_return", "episode_length"):
                    continue
                raise N.NativeError(f"gae: {name} is required")
            if not x.is_cuda or x.device != rewards.device or x.dtype != dtype or tuple(x.shape) != (rows, B):
                raise N.NativeError(f"gae: {name} must be a {dtype} HIP tensor [{rows}, {B}] on the rewards' device, "
                                    f"got {x.dtype} {tuple(x.shape)} on {x.device}")
            if (B > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) != ld):
                raise N.NativeError(f"gae: {name} must have unit inner stride and the row stride {ld} of the other arrays, "
                                    f"got strides {tuple(x.stride())}")
        for name, x, dtype in (("ep_return_acc", ep_return_acc, torch.float64), ("ep_length_acc", ep_length_acc, torch.int32)):
            if x is not None and (not x.is_cuda or x.device != rewards.device or x.dtype != dtype or tuple(x.shape) != (B,)
                                  or (B > 1 and x.stride(0) != 1)):
                raise N.NativeError(f"gae: {name} must be a dense {dtype} HIP tensor [{B}] on the rewards' device")
        g = N.Gae()
        g.T, g.rewards_f64, g.ld = T, int(rewards.dtype == torch.float64), ld
        g.gamma, g.gae_lambda = float(gamma), float(gae_lambda)
        for name in ("rewards", "values", "terminated", "truncated", "boot", "advantages", "returns", "episode_return", "episode_length"):
            x = wanted[name][0]
            setattr(g, name, None if x is None else x.data_ptr())
        g.ep_return_acc = None if ep_return_acc is None else ep_return_acc.data_ptr()
        g.ep_length_acc = None if ep_length_acc is None else ep_length_acc.data_ptr()
        N.check(self.lib.pdegym_gae(C.byref(g), B, N.current_stream_ptr(rewards.device)), "pdegym_gae")

    @staticmethod
    def _ppo_rows(what, name, x, rows, width, dtype, device):
        """``x`` as a [rows, width] (width None: [rows]) tensor of ``dtype`` on ``device`` with unit inner stride: its row stride."""
        import torch
        shape = (rows,) if width is None else (rows, width)
        if (not torch.is_tensor(x) or not x.is_cuda or x.device != device or x.dtype != dtype or tuple(x.shape) != shape
                or (rows > 1 and x.stride(0) < (width or 1)) or (width is not None and width > 1 and x.stride(1) != 1)
                or (width is None and rows > 1 and x.stride(0) != 1)):
            raise N.NativeError(f"{what}: {name} must be a {dtype} HIP tensor {list(shape)} with unit inner stride on the mean's device, "
                                f"got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
        return (x.stride(0) if rows > 1 else width) if width is not None else 1

    @_on_device_of("mean")
    def ppo_loss(self, mean, log_std, values, actions, old_log_prob, advantages, returns, d_mean, d_values, d_log_std, stats,
                 clip_range: float, ent_coef: float, vf_coef: float, normalize_advantage: bool, index=None, workspace=None):
        """The PPO loss of a minibatch and its gradients in at most three launches (pdegym_ppo_loss: SB3's ``PPO.train`` loss for a
        ``DiagGaussianDistribution``).  ``mean`` [N, A] and ``values`` [N] (or None: no value term) in minibatch order, ``log_std``
        [A]; ``actions`` [M, A], ``old_log_prob`` / ``advantages`` / ``returns`` [M] are gathered by ``index`` (int64 [N], entries in
        [0, M)) or, without it, M = N.  Outputs ``d_mean`` [N, A], ``d_values`` [N] (with ``values``), ``d_log_std`` [A], ``stats``
        [8] (``N.PPO_LOSS_STATS``).  Everything float32 with unit inner stride (2-D tensors may have a row stride), on one device.
        ``workspace``: None (the backend's own, cached per device and size, allocated at the first call of a shape) or a uint8
        tensor of at least pdegym_ppo_loss_workspace(N, A) bytes."""
        import torch
        if not torch.is_tensor(mean) or mean.dim() != 2:
            raise N.NativeError("ppo_loss: mean must be a float32 [N, A] tensor")
        n, A = (int(s) for s in mean.shape)
        dev, f32, what = mean.device, torch.float32, "ppo_loss"
        M = n if index is None else (int(actions.shape[0]) if torch.is_tensor(actions) and actions.dim() == 2 else -1)
        g = N.PpoLoss()
        g.A, g.normalize_advantage, g.M = A, int(bool(normalize_advantage)), M
        g.ld_mean = self._ppo_rows(what, "mean", mean, n, A, f32, dev)
        g.ld_actions = self._ppo_rows(what, "actions", actions, M, A, f32, dev)
        g.ld_d_mean = self._ppo_rows(what, "d_mean", d_mean, n, A, f32, dev)
        dense = [("log_std", log_std, A, f32), ("old_log_prob", old_log_prob, M, f32), ("advantages", advantages, M, f32),
                 ("d_log_std", d_log_std, A, f32), ("stats", stats, len(N.PPO_LOSS_STATS), f32)]
        if index is not None:
            dense.append(("index", index, n, torch.int64))
        if (values is None) != (d_values is None):
            raise N.NativeError("ppo_loss: values and d_values are given together")
        if values is not None:
            dense += [("values", values, n, f32), ("d_values", d_values, n, f32), ("returns", returns, M, f32)]
        for name, x, rows, dtype in dense:
            self._ppo_rows(what, name, x, rows, None, dtype, dev)
            setattr(g, name, x.data_ptr())
        g.mean, g.actions, g.d_mean = mean.data_ptr(), actions.data_ptr(), d_mean.data_ptr()
        if workspace is None:
            need = int(self.lib.pdegym_ppo_loss_workspace(n, A))
            if need < 0:
                N.check(need, "pdegym_ppo_loss_workspace")
            workspace = self._mlp_backward_workspace(dev, need)
        elif not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
            raise N.NativeError("ppo_loss: workspace must be a contiguous uint8 tensor on the mean's device")
        g.clip_range, g.ent_coef, g.vf_coef = float(clip_range), float(ent_coef), float(vf_coef)
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel()
        N.check(self.lib.pdegym_ppo_loss(C.byref(g), n, N.current_stream_ptr(dev)), "pdegym_ppo_loss")

    @_on_device_of("mean")
    def diag_gaussian_log_prob(self, mean, log_std, actions, out, index=None):
        """out[i] = log N(actions[index[i] or i]; mean[i], exp(log_std)) summed over the A dimensions, through the device function
        ``ppo_loss`` uses (pdegym_diag_gaussian_log_prob): ``mean`` [N, A], ``actions`` [M, A], ``out`` [N], ``index`` int64 [N]."""
        import torch
        if not torch.is_tensor(mean) or mean.dim() != 2:
            raise N.NativeError("diag_gaussian_log_prob: mean must be a float32 [N, A] tensor")
        n, A = (int(s) for s in mean.shape)
        dev, f32, what = mean.device, torch.float32, "diag_gaussian_log_prob"
        M = n if index is None else (int(actions.shape[0]) if torch.is_tensor(actions) and actions.dim() == 2 else -1)
        ld = self._ppo_rows(what, "mean", mean, n, A, f32, dev)
        ld_a = self._ppo_rows(what, "actions", actions, M, A, f32, dev)
        self._ppo_rows(what, "log_std", log_std, A, None, f32, dev)
        self._ppo_rows(what, "out", out, n, None, f32, dev)
        if index is not None:
            self._ppo_rows(what, "index", index, n, None, torch.int64, dev)
        N.check(self.lib.pdegym_diag_gaussian_log_prob(mean.data_ptr(), ld, log_std.data_ptr(), actions.data_ptr(), ld_a,
                                                       None if index is None else index.data_ptr(), out.data_ptr(), n, A,
                                                       N.current_stream_ptr(dev)), "pdegym_diag_gaussian_log_prob")

    def _sac_workspace(self, what, workspace, n, dev):
        import torch
        if workspace is None:
            need = int(self.lib.pdegym_sac_loss_workspace(n))
            if need < 0:
                N.check(need, "pdegym_sac_loss_workspace")
            return self._mlp_backward_workspace(dev, need)
        if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
            raise N.NativeError(f"{what}: workspace must be a contiguous uint8 tensor on the device of the other tensors")
        return workspace

    @staticmethod
    def _sac_shape(what, name, x):
        import torch
        if not torch.is_tensor(x) or x.dim() != 2:
            raise N.NativeError(f"{what}: {name} must be a float32 2-D tensor")
        return (int(s) for s in x.shape)

    @_on_device_of("raw")
    def squashed_gaussian_sample(self, raw, eps, actions, log_prob, log_std_min: float, log_std_max: float, obs=None):
        """a = tanh(mu + exp(clip(log_std)) * eps) and SB3's squashed-Gaussian log-probability of it in one launch
        (pdegym_squashed_gaussian_sample).  ``raw`` [N, 2A] = [mu; log_std], ``eps`` [N, A]; outputs ``actions`` [N, A] -- or, with
        ``obs`` [N, D], the block [N, D + A] whose first D columns receive the observation -- and ``log_prob`` [N].  Everything float32
        with unit inner stride (2-D tensors may have a row stride), on one device."""
        import torch
        what = "squashed_gaussian_sample"
        n, A2 = self._sac_shape(what, "raw", raw)
        A, dev, f32 = A2 // 2, raw.device, torch.float32
        if A2 != 2 * A or A < 1:
            raise N.NativeError(f"{what}: raw must have 2A columns [mu; log_std], got {A2}")
        D = 0
        if obs is not None:
            _, D = self._sac_shape(what, "obs", obs)
        s = N.SquashedGaussianSample()
        s.A, s.D, s.log_std_min, s.log_std_max = A, D, float(log_std_min), float(log_std_max)
        s.ld_raw = self._ppo_rows(what, "raw", raw, n, 2 * A, f32, dev)
        s.ld_eps = self._ppo_rows(what, "eps", eps, n, A, f32, dev)
        s.ld_actions = self._ppo_rows(what, "actions", actions, n, D + A, f32, dev)
        self._ppo_rows(what, "log_prob", log_prob, n, None, f32, dev)
        if obs is not None:
            s.ld_obs = self._ppo_rows(what, "obs", obs, n, D, f32, dev)
            s.obs = obs.data_ptr()
        s.raw, s.eps, s.actions, s.log_prob = raw.data_ptr(), eps.data_ptr(), actions.data_ptr(), log_prob.data_ptr()
        N.check(self.lib.pdegym_squashed_gaussian_sample(C.byref(s), n, N.current_stream_ptr(dev)), "pdegym_squashed_gaussian_sample")

    @_on_device_of("raw")
    def squashed_gaussian_sample_backward(self, raw, eps, d_actions, d_log_prob, d_raw, log_std_min: float, log_std_max: float):
        """``d_raw`` [N, 2A] from ``d_actions`` [N, A] (any row stride: the action columns of a critic's dx in place) and / or
        ``d_log_prob`` -- a dense [N] tensor, or a 1-element tensor / a [N] tensor of stride 0: one device scalar for all rows --
        in one launch (pdegym_squashed_gaussian_sample_backward); either may be None, not both."""
        import torch
        what = "squashed_gaussian_sample_backward"
        n, A2 = self._sac_shape(what, "raw", raw)
        A, dev, f32 = A2 // 2, raw.device, torch.float32
        if A2 != 2 * A or A < 1:
            raise N.NativeError(f"{what}: raw must have 2A columns [mu; log_std], got {A2}")
        s = N.SquashedGaussianSampleBackward()
        s.A, s.log_std_min, s.log_std_max = A, float(log_std_min), float(log_std_max)
        s.ld_raw = self._ppo_rows(what, "raw", raw, n, 2 * A, f32, dev)
        s.ld_eps = self._ppo_rows(what, "eps", eps, n, A, f32, dev)
        s.ld_d_raw = self._ppo_rows(what, "d_raw", d_raw, n, 2 * A, f32, dev)
        if d_actions is not None:
            s.ld_d_actions = self._ppo_rows(what, "d_actions", d_actions, n, A, f32, dev)
            s.d_actions = d_actions.data_ptr()
        if d_log_prob is not None:
            if torch.is_tensor(d_log_prob) and d_log_prob.dim() == 1 and d_log_prob.dtype == f32 and d_log_prob.device == dev and (
                    d_log_prob.shape[0] == 1 or (d_log_prob.shape[0] == n and d_log_prob.stride(0) == 0)):
                s.d_log_prob_stride = 0
            else:
                self._ppo_rows(what, "d_log_prob", d_log_prob, n, None, f32, dev)
                s.d_log_prob_stride = 1
            s.d_log_prob = d_log_prob.data_ptr()
        s.raw, s.eps, s.d_raw = raw.data_ptr(), eps.data_ptr(), d_raw.data_ptr()
        N.check(self.lib.pdegym_squashed_gaussian_sample_backward(C.byref(s), n, N.current_stream_ptr(dev)),
                "pdegym_squashed_gaussian_sample_backward")

    @_on_device_of("q1")
    def sac_critic_loss(self, q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma: float, d_q1, d_q2,
                        target=None, stats=None, index=None, workspace=None):
        """SAC's critic loss and its gradients in two launches (pdegym_sac_critic_loss).  ``q1`` / ``q2`` / ``q1_target`` /
        ``q2_target`` / ``next_log_prob`` [N] dense (``q2``, ``q2_target``, ``d_q2`` None: one critic); ``rewards`` / ``dones`` [M]
        float32 gathered by ``index`` (int64 [N]) or M = N; ``log_alpha`` a 1-element DEVICE tensor.  Outputs ``d_q1`` / ``d_q2`` [N],
        optional ``target`` [N] and ``stats`` [4] (``N.SAC_CRITIC_STATS``)."""
        import torch
        what = "sac_critic_loss"
        if not torch.is_tensor(q1) or q1.dim() != 1:
            raise N.NativeError(f"{what}: q1 must be a float32 [N] tensor")
        n, dev, f32 = int(q1.shape[0]), q1.device, torch.float32
        M = n if index is None else (int(rewards.shape[0]) if torch.is_tensor(rewards) and rewards.dim() == 1 else -1)
        g = N.SacCriticLoss()
        g.M, g.gamma = M, float(gamma)
        if len({q2 is None, q2_target is None, d_q2 is None}) != 1:
            raise N.NativeError(f"{what}: q2, q2_target and d_q2 are given together")
        named = [("q1", q1, n, f32), ("q1_target", q1_target, n, f32), ("next_log_prob", next_log_prob, n, f32), ("rewards", rewards, M, f32),
                 ("dones", dones, M, f32), ("log_alpha", log_alpha, 1, f32), ("d_q1", d_q1, n, f32)]
        if q2 is not None:
            named += [("q2", q2, n, f32), ("q2_target", q2_target, n, f32), ("d_q2", d_q2, n, f32)]
        if index is not None:
            named.append(("index", index, n, torch.int64))
        if target is not None:
            named.append(("target", target, n, f32))
        if stats is not None:
            named.append(("stats", stats, len(N.SAC_CRITIC_STATS), f32))
        for name, x, rows, dtype in named:
            self._ppo_rows(what, name, x, rows, None, dtype, dev)
            setattr(g, name, x.data_ptr())
        workspace = self._sac_workspace(what, workspace, n, dev)
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel()
        N.check(self.lib.pdegym_sac_critic_loss(C.byref(g), n, N.current_stream_ptr(dev)), "pdegym_sac_critic_loss")

    @_on_device_of("q1_pi")
    def sac_actor_loss(self, q1_pi, q2_pi, log_prob, log_alpha, target_entropy: float, d_q1_pi, d_q2_pi, d_log_prob, d_log_alpha,
                       stats=None, workspace=None):
        """SAC's actor and entropy-coefficient losses and their gradients in two launches (pdegym_sac_actor_loss).  ``q1_pi`` /
        ``q2_pi`` (None with ``d_q2_pi``: one critic) / ``log_prob`` [N], ``log_alpha`` a 1-element DEVICE tensor.  Outputs
        ``d_q1_pi`` / ``d_q2_pi`` [N], ``d_log_prob`` [1] (ONE scalar for all rows), ``d_log_alpha`` [1], optional ``stats`` [4]
        (``N.SAC_ACTOR_STATS``)."""
        import torch
        what = "sac_actor_loss"
        if not torch.is_tensor(q1_pi) or q1_pi.dim() != 1:
            raise N.NativeError(f"{what}: q1_pi must be a float32 [N] tensor")
        n, dev, f32 = int(q1_pi.shape[0]), q1_pi.device, torch.float32
        if (q2_pi is None) != (d_q2_pi is None):
            raise N.NativeError(f"{what}: q2_pi and d_q2_pi are given together")
        g = N.SacActorLoss()
        g.target_entropy = float(target_entropy)
        named = [("q1_pi", q1_pi, n), ("log_prob", log_prob, n), ("log_alpha", log_alpha, 1), ("d_q1_pi", d_q1_pi, n),
                 ("d_log_prob", d_log_prob, 1), ("d_log_alpha", d_log_alpha, 1)]
        if q2_pi is not None:
            named += [("q2_pi", q2_pi, n), ("d_q2_pi", d_q2_pi, n)]
        if stats is not None:
            named.append(("stats", stats, len(N.SAC_ACTOR_STATS)))
        for name, x, rows in named:
            self._ppo_rows(what, name, x, rows, None, f32, dev)
            setattr(g, name, x.data_ptr())
        workspace = self._sac_workspace(what, workspace, n, dev)
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel()
        N.check(self.lib.pdegym_sac_actor_loss(C.byref(g), n, N.current_stream_ptr(dev)), "pdegym_sac_actor_loss")

    @_on_device_of("sizes")      # (no tensors: nothing to switch; the size query launches nothing)
    def fused_adam_workspace(self, sizes) -> int:
        """Bytes of workspace ``fused_adam`` needs for tensors of ``sizes`` elements (pdegym_fused_adam_workspace)."""
        arr = (C.c_int64 * len(sizes))(*[int(s) for s in sizes])
        need = int(self.lib.pdegym_fused_adam_workspace(arr, len(sizes)))
        if need < 0:
            N.check(need, "pdegym_fused_adam_workspace")
        return need

    @_on_device_of("state")
    def fused_adam(self, entries, state, workspace, lr, beta1: float, beta2: float, eps: float, max_grad_norm=None, tau=None,
                   polyak: bool = False, total_norm=None, cache=None):
        """Clip, Adam step, weight mirrors and Polyak targets of up to 32 float32 tensors in two launches (pdegym_fused_adam).
        ``entries``: one dict per tensor with ``p``, ``g``, ``m``, ``v`` and optionally ``copy``, ``wt`` = (blocked tensor, out_total,
        row0), ``pt``, ``pt_copy``, ``pt_wt`` (include/pdegym.h).  ``state``: float64 [3] on the device (step, beta1^t, beta2^t);
        ``workspace``: uint8, ``fused_adam_workspace`` bytes; ``lr``: a float or a 0-d float32 device tensor; ``total_norm``: None or a
        1-element float32 device tensor.  ``cache``: a dict the caller keeps per entry list -- the descriptor is built once and only
        the gradient addresses (and ``polyak``) are rewritten on later calls with the same list."""
        import torch
        a = None if cache is None else cache.get("fused_adam")
        if a is None:
            if not 1 <= len(entries) <= N.FUSED_ADAM_MAX_TENSORS:
                raise N.NativeError(f"fused_adam: 1..{N.FUSED_ADAM_MAX_TENSORS} tensors per call, got {len(entries)}")
            f32, dev = torch.float32, entries[0]["p"].device
            if dev.type != "cuda":
                raise N.NativeError("fused_adam: tensors must be on a HIP device; there is no CPU path")

            def ptr(what, x, numel, dtype=f32):
                if not torch.is_tensor(x) or x.dtype != dtype or x.device != dev or not x.is_contiguous() or x.numel() < numel:
                    raise N.NativeError(f"fused_adam: {what} must be a contiguous {dtype} tensor of {numel} elements on {dev}")
                return x.data_ptr()

            a = N.FusedAdam()
            a.K = len(entries)
            for t, e in zip(a.tensor, entries):
                p = e["p"]
                n = p.numel()
                t.n = n
                t.out, t.in_ = (int(p.shape[0]), int(p.shape[1])) if p.dim() == 2 else (1, n)
                for name in ("p", "m", "v", "copy", "pt", "pt_copy"):
                    if e.get(name) is not None:
                        setattr(t, name, ptr(name, e[name], n))
                for name in ("wt", "pt_wt"):
                    if e.get(name) is not None:
                        blocked, out_total, row0 = e[name]
                        setattr(t, name, ptr(name, blocked, (t.in_ + 3) // 4 * int(out_total) * 4))
                        setattr(t, name + "_out_total", int(out_total))
                        setattr(t, name + "_row0", int(row0))
            a.state = ptr("state", state, 3, torch.float64)
            a.workspace, a.workspace_bytes = ptr("workspace", workspace, 1, torch.uint8), workspace.numel()
            if total_norm is not None:
                a.total_norm = ptr("total_norm", total_norm, 1)
            if torch.is_tensor(lr):
                a.lr_device = ptr("lr", lr, 1)
            a.beta1, a.beta2, a.eps = float(beta1), float(beta2), float(eps)
            a.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
            a.tau = 0.0 if tau is None else float(tau)
            if cache is not None:
                cache["fused_adam"] = a
                cache["device"] = dev
        dev = entries[0]["p"].device
        if not torch.is_tensor(lr):
            a.lr = float(lr)
        a.polyak = int(bool(polyak))
        for t, e in zip(a.tensor, entries):
            g = e["g"]
            if g.dtype != torch.float32 or g.device != dev or not g.is_contiguous() or g.numel() != t.n:
                raise N.NativeError("fused_adam: a gradient must be a contiguous float32 tensor of its parameter's size and device")
            t.g = g.data_ptr()
        N.check(self.lib.pdegym_fused_adam(C.byref(a), N.current_stream_ptr(dev)), "pdegym_fused_adam")

    @_on_device_of("obs")
    def backstep_rollout1d(self, kind: str, P: N.Params1D, T: dict, obs, actions, rewards, terminated, truncated, B: int, law: N.Backstep,
                           obs_noise=None, obs_seen=None, final_obs_steps=None):
        """T env-steps with the backstepping law inside, in one launch (pdegym_*_backstep_rollout): the buffers of ``rollout1d``
        (full-state sensing: ``obs`` [T+1, B, n]); ``actions`` is an output.  ``law``: an ``N.Backstep`` descriptor with gains,
        length, order, scale, ``noise`` [T, B], clamp (``BacksteppingController.rollout_law``; obs / out64 / out32 unset).
        ``final_obs_steps`` [T, B, n]: as in ``rollout1d``."""
        import torch
        fn = self.lib.pdegym_transport_backstep_rollout if kind == "transport" else self.lib.pdegym_parabolic_backstep_rollout
        steps = int(actions.shape[0])
        _check_shapes("backstep rollout", {"obs": (obs, (steps + 1, B, P.n)), "actions": (actions, (steps, B)), "rewards": (rewards, (steps, B)),
                                           "terminated": (terminated, (steps, B)), "truncated": (truncated, (steps, B)),
                                           "obs_noise": (obs_noise, (steps, B, P.n), torch.float32),
                                           "obs_seen": (obs_seen, (steps, B, P.n), torch.float32)})
        flags = _final_obs_steps("backstep rollout", final_obs_steps, (steps, B, P.n), torch.float32, obs)
        bufs = self._bufs1d({**T, "state_in": None, "u": None, "history": None, **({"final_obs": final_obs_steps} if flags else {})})
        ro = self._rollout1d_desc(obs, actions, rewards, terminated, truncated, obs_noise, obs_seen)
        ro.reserved_ = flags
        N.check(fn(C.byref(P), C.byref(bufs), C.byref(ro), C.byref(law), B, N.current_stream_ptr(obs.device)),
                f"pdegym_{kind}_backstep_rollout")


_default = None


def default_backend():
    """The process-wide HIP backend (loads libpdegym_hip.so; raises if it is missing)."""
    global _default
    if _default is None:
        _default = HipBackend()
    return _default
