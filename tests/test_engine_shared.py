"""The host-side pieces the four engines and the backend share: ``hostio.PackLayout`` (device pack and host pack) and the
backend's shape check of the rollout buffers.  CPU only, smallest shapes."""
import numpy as np
import pytest

from tests.fake_backend import FakeBackend

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("align", [64, 8, 1])
def test_pack_layout_views_alias_one_allocation(host, align):
    """Every torch view and every NumPy view of a pack -- in device memory or in host memory -- names bytes of the ONE allocation,
    segments do not overlap and start where ``align`` says, and the two kinds of view see each other's writes."""
    from pdecontrolgym_amd.hostio import PackLayout
    spec = [("a", (2,), torch.float64), ("obs", (2, 3), torch.float32), ("r", (2,), torch.float32), ("n", (3,), torch.int32),
            ("te", (2,), torch.uint8), ("tr", (2,), torch.uint8)]
    layout = PackLayout(spec, align)
    pack, tv = layout.allocate(torch.device("cpu"), host=host)
    assert pack.dtype == torch.uint8 and pack.numel() == layout.nbytes and layout.nbytes % 64 == 0 and not pack.is_pinned()
    assert int(pack.sum()) == 0
    nv = layout.numpy_views(pack.numpy())
    assert list(tv) == list(nv) == [name for name, _, _ in spec]
    end = 0
    for name, shape, dtype in spec:
        t, a = tv[name], nv[name]
        assert t.dtype == dtype and tuple(t.shape) == shape == a.shape
        off = t.data_ptr() - pack.data_ptr()
        assert off == a.__array_interface__["data"][0] - pack.data_ptr()          # the same bytes under both names
        assert off >= end and off % align == 0 and off - end < align               # after the previous segment, on its boundary
        end = off + t.numel() * t.element_size()
    assert end <= layout.nbytes
    for i, name in enumerate(tv):                                                  # torch -> NumPy, NumPy -> torch, nobody else's bytes
        tv[name].fill_(i + 1)
        assert (nv[name] == i + 1).all()
        nv[name][...] = 100 + i
        assert bool((tv[name] == 100 + i).all())
    assert all(bool((tv[name] == 100 + i).all()) for i, name in enumerate(tv))


def test_host_io_command_slot_of_the_1d_engine_is_one_8_byte_slot_under_two_types():
    """``PDEBatch1D.enable_host_io``: the float32 and the float64 view of the command overlay the same 8 bytes of the host pack (a
    float32 command occupies the first four), the engine's ``action`` tensor is that slot, and the results are views of the same
    pack."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    e = PDEBatch1D("transport", T=0.3, dt=1e-3, X=1, dx=0.125, control_sample_rate=5e-3, reward=RewardSpec(N.REWARD_TUNED1D, 300),
                   num_envs=1, device="cpu", backend=FakeBackend(), state_in_obs=False)
    nv = e.enable_host_io()
    io, pack = e._hio, e._hio["pack"]
    assert sorted(nv) == ["norm_now", "obs", "reward", "terminated", "truncated"]
    assert nv["obs"].dtype == np.float32 and nv["obs"].shape == (1, 8) and nv["reward"].shape == nv["norm_now"].shape == (1,)
    assert nv["terminated"].dtype == nv["truncated"].dtype == np.uint8
    a32, a64 = io["a32"], io["a64"]
    assert a32.dtype == np.float32 and a64.dtype == np.float64 and a32.shape == a64.shape == (1,)
    addr = lambda a: a.__array_interface__["data"][0]                      # noqa: E731
    assert addr(a32) == addr(a64) == io["action"].data_ptr() == e.t["action"].data_ptr() == pack.data_ptr()
    a64[:] = -0.5
    assert a32[0] == np.frombuffer(np.float64(-0.5).tobytes(), np.float32)[0] and float(io["action"][0]) == -0.5
    a32[:] = 0.25
    assert np.frombuffer(a64.tobytes(), np.float32)[0] == np.float32(0.25)
    assert np.frombuffer(a64.tobytes(), np.float32)[1] == np.frombuffer(np.float64(-0.5).tobytes(), np.float32)[1]
    lo, hi = pack.data_ptr(), pack.data_ptr() + pack.numel()
    for k in ("obs", "reward", "norm_now", "terminated", "truncated"):
        assert lo + 8 <= addr(nv[k]) < hi and addr(nv[k]) == e.t[k].data_ptr()   # results: behind the command, in the same pack
    assert e._obs[0] is e._obs[1] is e.t["obs"]


class _NoLibrary:
    def __getattr__(self, name):                    # an entry point may be looked up, never called: the shape checks come first
        return None


def _hip_backend_without_library():
    from pdecontrolgym_amd.backend import HipBackend
    bk = HipBackend.__new__(HipBackend)
    bk.lib = _NoLibrary()
    return bk


def test_rollout_entry_points_name_the_buffer_that_has_the_wrong_shape():
    """One failing buffer per rollout entry point of ``HipBackend``: the message names it, the shape it must have and the one it has."""
    from pdecontrolgym_amd import _native as N
    bk = _hip_backend_without_library()
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype)        # noqa: E731

    def message(call):
        with pytest.raises(N.NativeError) as err:
            call()
        return str(err.value)

    P = N.Params1D()
    P.n, P.sensing = 5, N.SENSE_FULL
    ok = dict(obs=z(3, 3, 5), actions=z(2, 3), rewards=z(2, 3), terminated=z(2, 3, dtype=u8), truncated=z(2, 3, dtype=u8))
    run1d = lambda **kw: bk.rollout1d("transport", P, {}, *{**ok, **kw}.values(), 3)      # noqa: E731
    assert message(lambda: run1d(rewards=z(2, 2))) == "rollout rewards must be a contiguous [2, 3] tensor, got (2, 2)"
    assert message(lambda: run1d(obs=z(3, 5, 3).transpose(1, 2))) == "rollout obs must be a contiguous [3, 3, 5] tensor, got (3, 3, 5)"
    noisy = lambda x: bk.rollout1d("transport", P, {}, *ok.values(), 3, obs_noise=x)      # noqa: E731
    assert message(lambda: noisy(z(2, 3, 4))) == "rollout obs_noise must be a contiguous float32 [2, 3, 5] tensor, got (2, 3, 4)"
    assert message(lambda: noisy(z(2, 3, 5, dtype=f64))) == "rollout obs_noise must be a contiguous float32 [2, 3, 5] tensor, got (2, 3, 5)"

    Q = N.ParamsNS2D()
    Q.nx, Q.ny, Q.action_dim = 4, 8, 1
    T = {"p": z(1, 8, 4, dtype=f64)}
    assert message(lambda: bk.ns2d_rollout(Q, T, z(3, 1, 8, 4, 2, dtype=f64), z(2, 1, 2, dtype=f64), z(2, 1, dtype=f64),
                                           z(2, 1, dtype=u8), 1)) == "rollout actions must be a contiguous [2, 1, 1] tensor, got (2, 1, 2)"
    assert message(lambda: bk.ns2d_adjoint(Q, T, z(3, 1, 8, 4, 2, dtype=f64), z(2, dtype=f64), 0.1, 1.0, z(2, 1, dtype=f64),
                                           z(2, 1, dtype=f64), lam=z(2, 1, 8, 4, dtype=f64))) \
        == "adjoint lam must be a contiguous [2, 1, 8, 4, 2] tensor, got (2, 1, 8, 4)"

    R = N.ParamsTraffic()
    R.M = 3
    tr = dict(obs=z(3, 2, 6, dtype=f64), actions=z(2, 2, 1, dtype=f64), rewards=z(2, 2, dtype=f64), done=z(2, 2, dtype=u8),
              truncated=z(2, 2, dtype=u8))
    run_tr = lambda **kw: bk.traffic_rollout(R, {"r": tr["obs"]}, *{**tr, **kw}.values(), 2)      # noqa: E731
    assert message(lambda: run_tr(done=z(3, 2, dtype=u8))) == "rollout done must be a contiguous [2, 2] tensor, got (3, 2)"
    assert message(lambda: run_tr(actions=z(2, 2, 3, dtype=f64))) == "rollout actions must be a contiguous [2, 2, 1 or 2] tensor, got (2, 2, 3)"
