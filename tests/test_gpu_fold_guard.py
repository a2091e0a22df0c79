"""The folded sub-step of the headline step kernel (step1d_kernel<HeadArgsFold, 4, true, false, true>: nx = 256 parabolic, the row fills
the wave; launch_epl takes it when F is a power of two and an env-step has more than one sub-step) against the NumPy oracle, on the
rows that decide which of its loops runs (pdegym_1d_body.h: run_substeps, FOLD; the lemma: tests/test_fold_lemma.py):

  (a) ordinary rows                          the fold loop for the whole call, also with a commanded boundary value of 0;
  (b) even slots of order one, odd tiny      the fold loop at the lemma's edge;
  (c) rows at / inside the denormal range    below the floor after the peeled sub-step: the plain loop, the fold never starts;
  (d) constant rows of 1.5 * 2^-64           above the floor after the peeled sub-step (slot 0: 1.125 * 2^-64), below it a few sub-steps
                                             later: the call starts over in the plain loop -- ring, |u[-1]| sum and the reward's
                                             look-back are what a second pass could get wrong;
  (e) a NaN in the row, a row near 2^126     the exact loop still wins;
  (f) F = 0.2                                not a power of two: the plain loop.

Bars as in tests/test_gpu_1d.py: rows, observations and time_index bit for bit (uint32 views), flags equal, norms rtol 1e-6, rewards
rtol 1e-6 with atol 2e-6 * max norm; the |u[-1]| sum (float64; the kernel adds nsub * |value|, NumPy one term per sub-step) rtol 1e-12.
Every pure output is poisoned before each call (tests/poison.py).
"""
import numpy as np
import pytest

from tests import poison as PZ

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NX = 256
N_NODES = NX + 1
OUT = ("reward", "norm_now", "norm_back", "terminated", "truncated")


def _even_odd(even, odd):
    """rows from per-slot values: even slots = nodes 1, 3, ..., 255; odd slots = nodes 2, 4, ..., 256; node 0 = 0"""
    row = np.zeros((even.shape[0], N_NODES), dtype=np.float32)
    row[:, 1::2] = even
    row[:, 2::2] = odd
    return row


def _rows(family, rng):
    """(init [B, 257], beta [B, 257], actions(step) -> [B]) of a family; B <= 16"""
    n = N_NODES
    x = np.linspace(0, 1, n)
    if family in ("a", "f"):
        B = 8
        init = rng.uniform(1, 10, (B, n)).astype(np.float32)
        beta = (50 * np.cos(rng.uniform(7, 8.5, (B, 1)) * np.arccos(x))).astype(np.float32)

        def actions(i):
            a = rng.uniform(-1, 1, B).astype(np.float32)
            a[0] = 0.0                       # the frozen boundary slot holds 0: an odd slot, not the guard's business
            a[1] = 0.0 if i != 1 else a[1]
            return a
    elif family == "b":
        B = 9
        even = (rng.uniform(1, 2, (B, NX // 2)) * rng.choice([-1, 1], (B, NX // 2))).astype(np.float32)
        odd = np.zeros((B, NX // 2), dtype=np.float32)
        odd[3:6] = np.float32(2.0 ** -125) * rng.choice([-1, 1], (3, NX // 2))
        odd[6:9] = (rng.uniform(-1, 1, (3, NX // 2)) * 1e-39).astype(np.float32)
        init = _even_odd(even, odd)
        beta = np.zeros((B, n), dtype=np.float32)
        beta[1::3] = rng.uniform(-30, 30, (3, n))
        beta[2::3] = (50 * np.cos(rng.uniform(7, 8.5, (3, 1)) * np.arccos(x))).astype(np.float32)
        actions = lambda i: np.where(np.arange(B) % 2 == 0, 0.0, rng.uniform(-1, 1, B)).astype(np.float32)
    elif family == "c":
        B = 8
        init = np.zeros((B, n), dtype=np.float32)
        init[:4] = (rng.uniform(0.5, 1, (4, n)) * 2.0 ** rng.integers(-126, -117, (4, 1))).astype(np.float32)
        init[4:] = (rng.uniform(-1, 1, (4, n)) * 1e-39).astype(np.float32)
        beta = np.zeros((B, n), dtype=np.float32)
        beta[1::2] = rng.uniform(-30, 30, (4, n))
        actions = lambda i: np.array([0, 0, 1e-40, 0.3, 0, 0, 1e-40, 0.3], dtype=np.float32)
    elif family == "d":
        B = 8
        init = np.full((B, n), 1.5 * 2.0 ** -64, dtype=np.float32)
        init[4:] *= rng.uniform(1, 1.3, (4, 1)).astype(np.float32)           # the trip a sub-step or two later
        beta = np.zeros((B, n), dtype=np.float32)
        beta[2:4] = rng.uniform(-30, 30, (2, n))
        beta[6:8] = rng.uniform(-30, 30, (2, n))
        actions = lambda i: np.array([0, 0.5, 0, -0.25, 0, 1.0, 2.0 ** -70, 0], dtype=np.float32)
    elif family == "e":
        B = 4
        init = rng.uniform(1, 10, (B, n)).astype(np.float32)
        init[1, 100] = np.nan
        init[2] = (rng.uniform(0.5, 1, n) * 2.0 ** 126).astype(np.float32)
        init[3, 255] = np.nan                # an even slot (node 255): v_min3_f32 skips it, the norm test must not
        beta = (50 * np.cos(rng.uniform(7, 8.5, (B, 1)) * np.arccos(x))).astype(np.float32)
        actions = lambda i: rng.uniform(-1, 1, B).astype(np.float32)
    else:
        raise KeyError(family)
    init[:, 0] = 0
    return init, beta, actions


def _run(family, S, nt=None, steps=3):
    from oracle import pde_oracle as po
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    rng = np.random.default_rng(ord(family) * 1000 + S + (nt or 0))
    dx = 1.0 / NX
    dt = (0.2 if family == "f" else 0.25) * dx * dx
    nt = nt or steps * S + 1
    kw = dict(T=(nt - 1) * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, control_type="Dirchilet", sensing_loc="full",
              sensing_type=None, normalize=False, max_control_value=20, limit_pde_state_size=True, max_state_value=1e10)
    rargs = (nt, -1e3, 3e2)
    init, beta, actions = _rows(family, rng)
    B = init.shape[0]
    orc = po.ParabolicOracle(reward=po.TunedReward1DOracle(*rargs), keep_history=False, **kw)
    env = PDEBatch1D("parabolic", reward=RewardSpec(N.REWARD_TUNED1D, *rargs), num_envs=B, device="cuda", **kw)      # state_in_obs, as bench.py
    assert env.state_in_obs and env.nt == orc.nt == nt and env.substeps == S
    assert (env.params.F == 0.25) == (family != "f")
    o_ref = orc.reset(init, beta)
    o_gpu = env.reset(torch.tensor(init), torch.tensor(beta))
    np.testing.assert_array_equal(o_gpu.cpu().numpy().view(np.uint32), o_ref.view(np.uint32))
    for i in range(steps):
        a = actions(i)
        with np.errstate(all="ignore"):
            o_ref, r_ref, te_ref, tr_ref = orc.step(a)
        for k in OUT:
            PZ.poison_(env.t[k])
        PZ.poison_(env._obs[env._flip ^ 1])                  # the buffer this step's observation goes to
        o_gpu, r_gpu, te_gpu, tr_gpu = env.step(torch.tensor(a))
        torch.cuda.synchronize()
        where = f"family {family} S={S} nt={nt} step {i}"
        for k in OUT:
            PZ.assert_written(env.t[k], None, f"{where}: {k}")
        rows, obs = env.u.cpu().numpy(), o_gpu.cpu().numpy()
        nn_gpu, nb_gpu, r_gpu = env.t["norm_now"].cpu().numpy(), env.t["norm_back"].cpu().numpy(), r_gpu.cpu().numpy()
        bad = np.nonzero((rows.view(np.uint32) != orc.row.view(np.uint32)).any(axis=1))[0]
        print(f"{where}: rows differing {bad.tolist()}  norm_now gpu {nn_gpu.tolist()} ref {orc.norm_now.tolist()}  "
              f"norm_back gpu {nb_gpu.tolist()} ref {orc.norm_back.tolist()}  reward gpu {r_gpu.tolist()} ref {r_ref.tolist()}")
        np.testing.assert_array_equal(rows.view(np.uint32), orc.row.view(np.uint32), err_msg=where)
        np.testing.assert_array_equal(obs.view(np.uint32), o_ref.view(np.uint32), err_msg=where)
        np.testing.assert_array_equal(env.time_index.cpu().numpy().view(np.uint32), orc.time_index.astype(np.int32).view(np.uint32), err_msg=where)
        np.testing.assert_array_equal(te_gpu.cpu().numpy().astype(bool), te_ref, err_msg=where)
        np.testing.assert_array_equal(tr_gpu.cpu().numpy().astype(bool), tr_ref, err_msg=where)
        finite = orc.norm_now[np.isfinite(orc.norm_now)]
        atol = 2e-6 * float(finite.max()) if finite.size else 0.0
        np.testing.assert_allclose(nn_gpu, orc.norm_now, rtol=1e-6, err_msg=where)
        np.testing.assert_allclose(nb_gpu, orc.norm_back, rtol=1e-6, err_msg=where)
        np.testing.assert_allclose(r_gpu, r_ref, rtol=1e-6, atol=atol, err_msg=where)
        np.testing.assert_allclose(env.t["bsum"].cpu().numpy(), orc.bsum, rtol=1e-12, err_msg=where)
        rec = orc.ring != 0                                  # the slots the oracle recorded: what a later reward reads
        np.testing.assert_allclose(env.t["ring"].cpu().numpy()[rec], orc.ring[rec], rtol=1e-6, err_msg=where)
    return orc


@pytest.mark.parametrize("S", [2, 3, 100])
@pytest.mark.parametrize("family", ["a", "b", "c", "d", "e", "f"])
def test_fold_guard_rows_match_the_oracle(family, S):
    _run(family, S)


def test_mid_call_restart_with_the_look_back_row_inside_the_call():
    """nt = 90 <= 100: the reward of the call that ends the episode (89 sub-steps) looks back at row nt - 1 - 100 -> index 79 of the
    Python-wrapped history, a row recorded INSIDE that call; with nt <= 128 every row's norm goes to the ring, one run of one sub-step
    each.  The (d) rows trip the guard a few sub-steps in, so all of it is written twice; two post-terminal calls follow."""
    orc = _run("d", 100, nt=90)
    assert (orc.time_index == 89).all() and (orc.norm_back != 0).all()
