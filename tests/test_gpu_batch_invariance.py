"""Batch invariance: an instance's outputs depend on that instance alone -- not on the batch size, not on its position in the
batch, not on the kernel the launcher picks for that batch on this device.  Sharding (a batch split into shards gives the bits
of the whole batch) and rollout() == step calls rest on it.

Every comparison here is of bit patterns (-0.0 != +0.0), rewards included.  NavierStokes2D rewards are summed in one canonical
order by every kernel whose selection can depend on the batch size, the workgroup size or the device (ns_generic_step,
ns_col_step, ns_col_step_w1, ns_col_rollout): column j adds du^2 then dv^2 over rows 0 .. ny-1, then the column sums are added
for j = 0 .. nx-1.  The register-tiled kernels (64^2, 128^2, 256^2) keep their own order -- their selection depends only on grid
and dtype -- and are pinned term by term with planted differences instead (test_ns_planted_reward_terms)."""
import math

import numpy as np
import pytest

from tests.fuzz_more import bits_equal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BC_MIX = {"upper": ["Controllable", "Neumann"], "lower": ["Neumann", "Controllable"],
          "left": ["Neumann", "Dirchilet"], "right": ["Controllable", "Neumann"]}
NT = 3          # an episode ends at the second step (time index >= nt - 1): the fused auto-reset runs inside every sweep below
STEPS = 4


def _dbg(key, value):
    from pdecontrolgym_amd import _native as N
    return N.load().pdegym_debug_set(getattr(N, key), int(value))


class _switches:
    """Set kernel dispatch overrides for the duration of a with-block; the defaults come back in any case."""
    DEFAULTS = {"DEBUG_NS_NO_COL": 0, "DEBUG_NS_GENERIC": 0, "DEBUG_NS_COL_MIN_BATCH": -1, "DEBUG_NS_NO_LDS_JACOBI": 0}

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _dbg(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            _dbg(k, self.DEFAULTS[k])


def _col_min_batch():
    """launch_ns_col's float64 minimum, from the device's SIMD count (4 per CU) with the launcher's own formula."""
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    return (400 * simds + 512) // 1024


def _assert_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        if not bits_equal(a, b):
            bad = np.argwhere(a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
                              != b.view(np.uint64 if b.dtype == np.float64 else np.uint32))
            raise AssertionError(f"{what}: {len(bad)} values differ in their bits, first at {bad[0].tolist()}: "
                                 f"{a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")
    else:
        np.testing.assert_array_equal(a, b, err_msg=what)


# ---- NavierStokes2D -------------------------------------------------------------------------------------------------
def _ns_data(ny, nx, M, K, seed, adim=1):
    """M instances (initial fields, a pool row each, STEPS commands each) of a ny x nx problem with episodes of NT steps."""
    rng = np.random.default_rng(seed)
    dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    dt = 0.2 * 0.5 * min(dx, dy) ** 2 / 0.1
    kw = dict(T=NT * dt, dt=dt, X=1, dx=dx, Y=1, dy=dy, boundary_condition=BC_MIX, U_ref=rng.uniform(-1, 1, (NT, ny, nx, 2)),
              action_ref=rng.uniform(1, 3, NT), gamma=0.1, maximum_pressure_iteration=K, action_dim=adim)
    ic = rng.uniform(-1, 1, (3, M, ny, nx))
    pool = rng.uniform(-1, 1, (3, M, ny, nx))
    acts = rng.uniform(2, 4, (STEPS, M, adim))
    return kw, ic, pool, acts


NS_KEYS = ("obs", "p", "reward", "terminated", "time_index", "final_obs", "reset_count")


def _ns_run(kw, ic, pool, acts, sel, dtype):
    """Step the instances ``sel`` (indices into the data) as one batch with the fused auto-reset (pool rows == batch size, so
    instance b always restarts from its own row).  Returns one dict of host arrays per step."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    B = len(sel)
    env = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, **kw)
    env.reset(*(x[sel] for x in ic))
    env.enable_auto_reset(*(x[sel] for x in pool))
    a_dev = torch.as_tensor(acts[:, sel], dtype=dtype, device="cuda")
    out = []
    for t in range(STEPS):
        obs, r, te = env.step(a_dev[t])
        out.append({"obs": obs.cpu().numpy().copy(), "p": env.p.cpu().numpy().copy(), "reward": r.cpu().numpy().copy(),
                    "terminated": te.cpu().numpy().copy(), "time_index": env.t["time_index"].cpu().numpy().copy(),
                    "final_obs": env.t["final_obs"].cpu().numpy().copy(), "reset_count": env.t["reset_count"].cpu().numpy().copy()})
    assert out[1]["terminated"].all() and (out[-1]["reset_count"] == 2).all()     # two episode ends were crossed
    return out


def _probe_positions(B, nx):
    """First instance, every lane group of the first column-kernel wave, the last (partial) wave, the last instance."""
    G = max(1, 64 // nx)
    last_wave = (B - 1) // G * G
    pos = {0, B - 1} | {g for g in range(G) if g < B} | set(range(last_wave, B))
    return sorted(pos)


def _check_probes(whole, pos, single, tag):
    for b in pos:
        for t, (sw, ss) in enumerate(zip(whole, single[b])):
            for k in NS_KEYS:
                _assert_bits(sw[k][b], ss[k][0], f"{tag} instance {b}, step {t}: {k}")


# (ny, nx, dtype, batch sizes beyond 1, K).  21 x 21 float64: the column / workgroup crossover (+ the two-wave column build from
# 1025 waves on); 30 / 24 / 12 square: the generic LDS path whose block size follows the batch (B <= 512 vs larger); 16 x 30 and
# 31 x 64: other column heights; 100 x 100: one LDS copy; 130 x 130: the global-memory Jacobi loop.  A size ("min", d) is the
# column kernel's float64 minimum on this device plus d (_col_min_batch).
_SMALL = (7, 512, 513, 1030)
_AROUND_MIN = (("min", -1), ("min", 0), ("min", 1))
NS_GRIDS = [
    (21, 21, "float64", _SMALL + _AROUND_MIN + (3073,), 6),
    (21, 21, "float32", _SMALL + (("min", -1), ("min", 1)), 6),
    (30, 30, "float32", _SMALL, 5), (30, 30, "float64", _SMALL, 5),
    (24, 24, "float32", (7, 512, 513), 5), (24, 24, "float64", (7, 512, 513), 5),
    (12, 12, "float32", (7, 512, 513), 5), (12, 12, "float64", (7, 512, 513), 5),
    (16, 30, "float32", (7, 512, 513, ("min", 1)), 5), (16, 30, "float64", (7, 512, ("min", -1), ("min", 1)), 5),
    (31, 64, "float32", (7, 513), 4), (31, 64, "float64", (7, ("min", -1), ("min", 1)), 4),
    (100, 100, "float32", (7, 33), 4), (100, 100, "float64", (7, 33), 4),
    (130, 130, "float32", (5, 17), 3), (130, 130, "float64", (5, 17), 3),
]


def _batch_size(spec):
    return _col_min_batch() + spec[1] if isinstance(spec, tuple) else spec


@pytest.mark.parametrize("ny,nx,dts,sizes,K", NS_GRIDS, ids=[f"{ny}x{nx}-{dts}" for ny, nx, dts, _, _ in NS_GRIDS])
def test_ns_outputs_do_not_depend_on_batch_size_or_position(ny, nx, dts, sizes, K):
    dtype = getattr(torch, dts)
    sizes = sorted(set(_batch_size(B) for B in sizes) - {1})
    M = max(sizes)
    kw, ic, pool, acts = _ns_data(ny, nx, M, K, 1000 + 7 * ny + nx)
    probes = sorted(set(b for B in sizes for b in _probe_positions(B, nx)))
    single = {b: _ns_run(kw, ic, pool, acts, np.array([b]), dtype) for b in probes}
    for B in sizes:
        whole = _ns_run(kw, ic, pool, acts, np.arange(B), dtype)
        _check_probes(whole, _probe_positions(B, nx), single, f"{ny}x{nx} {dts} B={B}")


@pytest.mark.parametrize("ny,nx,dts,B,K", [(21, 21, "float64", 9, 30), (21, 21, "float32", 7, 12), (16, 30, "float64", 5, 8),
                                           (31, 64, "float32", 3, 6), (8, 8, "float64", 17, 5), (11, 11, "float32", 6, 9)])
def test_ns_rollout_equals_step_calls_at_default_dispatch(ny, nx, dts, B, K):
    """rollout() (always the column kernel) against step calls at the DEFAULT dispatch: a small float64 batch steps on the
    workgroup kernel, yet every slot, reward and flag is the same bits."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    dtype = getattr(torch, dts)
    T = STEPS + 1
    kw, ic, pool, acts = _ns_data(ny, nx, B, K, 31 * ny + nx)
    acts = torch.as_tensor(np.concatenate([acts, acts[:1]]), dtype=dtype, device="cuda")
    outs = []
    for mode in ("steps", "rollout"):
        env = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, **kw)
        assert env.can_rollout()
        env.reset(*ic)
        env.enable_auto_reset(*pool)
        obs = torch.zeros(T + 1, B, ny, nx, 2, dtype=dtype, device="cuda")
        obs[0].copy_(env.t["obs"])
        rew = torch.zeros(T, B, dtype=dtype, device="cuda")
        te = torch.zeros(T, B, dtype=torch.uint8, device="cuda")
        if mode == "steps":
            env.t["obs"] = obs[0]
            for t in range(T):
                env.step(acts[t], out_obs=obs[t + 1], out_reward=rew[t], out_terminated=te[t])
        else:
            env.rollout(obs, acts, rew, te)
        outs.append([x.cpu().numpy().copy() for x in (obs, rew, te, env.p, env.t["time_index"], env.t["reset_count"],
                                                      env.t["final_obs"])])
    for name, a, b in zip(("obs", "rewards", "terminated", "p", "time_index", "reset_count", "final_obs"), *outs):
        _assert_bits(a, b, f"rollout vs steps {ny}x{nx} {dts}: {name}")
    assert outs[0][2].sum() > 0


# every way the launcher can run a grid; the switches only choose among kernels that exist for it
_KERNELS = {
    "default": {},
    "column": {"DEBUG_NS_COL_MIN_BATCH": 0},
    "workgroup": {"DEBUG_NS_NO_COL": 1},
    "workgroup_global_jacobi": {"DEBUG_NS_NO_COL": 1, "DEBUG_NS_NO_LDS_JACOBI": 1},
    "generic": {"DEBUG_NS_GENERIC": 1},
}


@pytest.mark.parametrize("ny,nx,dts,B,K,adim", [(21, 21, "float64", 10, 7, 1), (21, 21, "float32", 700, 5, 21), (16, 30, "float64", 5, 6, 1),
                                                (31, 64, "float32", 4, 5, 1), (32, 32, "float64", 600, 4, 32), (30, 30, "float32", 520, 5, 30),
                                                (12, 12, "float64", 3, 6, 1), (100, 100, "float64", 3, 5, 1), (40, 40, "float32", 2, 9, 1)])
def test_ns_every_kernel_choice_gives_the_same_bits(ny, nx, dts, B, K, adim):
    dtype = getattr(torch, dts)
    kw, ic, pool, acts = _ns_data(ny, nx, B, K, 5 * ny + 3 * nx + B, adim)
    ref = None
    for name, sw in _KERNELS.items():
        with _switches(**sw):
            got = _ns_run(kw, ic, pool, acts, np.arange(B), dtype)
        if ref is None:
            ref = got
            continue
        for t, (a, b) in enumerate(zip(ref, got)):
            for k in NS_KEYS:
                _assert_bits(b[k], a[k], f"{ny}x{nx} {dts} kernel {name} vs default, step {t}: {k}")


@pytest.mark.parametrize("ny,nx,dts,K", [(21, 21, "float64", 6), (30, 30, "float32", 5)])
def test_ns_shards_equal_the_whole_batch(ny, nx, dts, K):
    """2048 instances in one engine against the same instances as 8 engines of 256 on the same device (pools sliced per shard)."""
    dtype = getattr(torch, dts)
    B, S = 2048, 8
    kw, ic, pool, acts = _ns_data(ny, nx, B, K, 77 + ny)
    whole = _ns_run(kw, ic, pool, acts, np.arange(B), dtype)
    parts = [_ns_run(kw, ic, pool, acts, np.arange(s * B // S, (s + 1) * B // S), dtype) for s in range(S)]
    for t in range(STEPS):
        for k in NS_KEYS:
            _assert_bits(np.concatenate([p[t][k] for p in parts]), whole[t][k], f"{ny}x{nx} {dts} shards, step {t}: {k}")


# ---- the reward arithmetic itself -----------------------------------------------------------------------------------
def _reward_reference(obs, uref, act, aref, gamma, nx, ny, T):
    """NSReward in the canonical order, in precision T with one rounding per operation: per column j the sequential sum over
    rows of du^2 then dv^2 (np.cumsum runs in sequence; np.sum would not), then the column sums in sequence."""
    d = obs.astype(T) - uref.astype(T)                       # [ny, nx, 2]
    sq = d * d
    seq = np.ascontiguousarray(sq.transpose(1, 0, 2)).reshape(nx, 2 * ny)
    col = np.cumsum(seq, axis=1, dtype=T)[:, -1]
    ss = np.cumsum(col, dtype=T)[-1]
    da = act.astype(T) - T(aref)
    asq = np.cumsum(da * da, dtype=T)[-1]
    return ((T(-0.5) * ss) / T(nx)) / T(ny) - T(gamma / 2) * asq


@pytest.mark.parametrize("kernel", ["column", "workgroup"])
@pytest.mark.parametrize("ny,nx,dts,adim,B", [(21, 21, "float64", 1, 4), (21, 21, "float32", 21, 4), (16, 30, "float64", 1, 5),
                                              (31, 17, "float32", 1, 3), (11, 11, "float64", 11, 7), (8, 8, "float32", 8, 9)])
def test_ns_reward_matches_canonical_numpy_sum_bitwise(kernel, ny, nx, dts, adim, B):
    _reward_check(kernel, ny, nx, dts, adim, B)


@pytest.mark.parametrize("ny,nx,dts,adim,B,sw", [(30, 30, "float32", 30, 3, {}), (24, 40, "float64", 1, 2, {}),
                                                 (100, 100, "float64", 1, 2, {}), (70, 45, "float32", 1, 2, {}),
                                                 (30, 30, "float64", 1, 600, {}), (130, 130, "float32", 1, 2, {}),
                                                 (33, 33, "float64", 33, 2, {"DEBUG_NS_NO_LDS_JACOBI": 1})])
def test_ns_generic_reward_matches_canonical_numpy_sum_bitwise(ny, nx, dts, adim, B, sw):
    """The workgroup kernel on grids no column kernel serves: every Jacobi mode, workgroup sizes on both sides of B = 512."""
    _reward_check("generic", ny, nx, dts, adim, B, sw)


def _reward_check(kernel, ny, nx, dts, adim, B, extra=None):
    from pdecontrolgym_amd.batch2d import NSBatch2D
    dtype = getattr(torch, dts)
    T = np.float64 if dts == "float64" else np.float32
    kw, ic, pool, acts = _ns_data(ny, nx, B, 5, 11 * ny + nx + adim, adim)
    kw["action_dim"] = adim
    sw = {"column": {"DEBUG_NS_COL_MIN_BATCH": 0}, "workgroup": {"DEBUG_NS_NO_COL": 1}, "generic": {}}[kernel]
    sw = dict(sw, **(extra or {}))
    Uref = np.asarray(kw["U_ref"]).astype(T)
    aref = np.asarray(kw["action_ref"]).astype(T)
    with _switches(**sw):
        env = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, **kw)
        env.reset(*ic)
        for t in range(1, NT):
            a = acts[t].astype(T)
            obs, r, te = env.step(torch.as_tensor(a, device="cuda"))
            o, rr = obs.cpu().numpy(), r.cpu().numpy()
            for b in range(B):
                want = _reward_reference(o[b], Uref[t], a[b], aref[t], kw["gamma"], nx, ny, T)
                assert bits_equal(np.array([rr[b]]), np.array([want])), (
                    f"{kernel} {ny}x{nx} {dts} adim={adim} B={B} step {t} instance {b}: reward {rr[b]!r} != canonical {want!r} "
                    "(the reward must add column sums over rows, du^2 then dv^2, then the columns in order)")


# ---- planted differences: every term of the reward, for every NS kernel ---------------------------------------------
def _plant_sets(ny, nx, rng, tile):
    ring = [(i, j) for i in range(ny) for j in range(nx) if i in (0, ny - 1) or j in (0, nx - 1)]
    corners = [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)]
    seam_r = sorted({i for i in range(ny) for s in tile if i % s in (0, s - 1)} | {i for k in (94, 162) for i in (k - 1, k) if i < ny})
    seam_c = sorted({j for j in range(nx) for s in tile if j % s in (0, s - 1)})
    seams = {(int(i), int(rng.integers(nx))) for i in seam_r} | {(int(rng.integers(ny)), int(j)) for j in seam_c}
    lane = [(i, j) for i in range(ny) for j in (0, 1, nx - 2, nx - 1)] if nx <= 64 else []    # column kernel: edge lanes of a group
    sample = {(int(rng.integers(ny)), int(rng.integers(nx))) for _ in range(40)}
    out = {"ring": ring, "corners": corners, "seams": sorted(seams), "random": sorted(sample)}
    if lane:
        out["lane_edges"] = lane
    return out


# (ny, nx, dtype, K, B, switches, tile sizes whose seams are planted)
_PLANT = {
    "tile64_f32": (64, 64, "float32", 6, 2, {}, (2, 4)),
    "tile128_f32": (128, 128, "float32", 6, 2, {}, (4, 8)),
    "tile128_f64": (128, 128, "float64", 6, 2, {}, (16,)),
    "ns256_fused_f32": (256, 256, "float32", 6, 2, {}, (8, 16, 32)),
    "ns256_slabs_f64": (256, 256, "float64", 30, 2, {}, (16, 32)),
    "column_21_f64": (21, 21, "float64", 6, 4, {"DEBUG_NS_COL_MIN_BATCH": 0}, (4,)),
    "column_16x30_f32": (16, 30, "float32", 6, 5, {}, (4,)),
    "generic_30_f32": (30, 30, "float32", 6, 3, {}, (4,)),
    "generic_100_f64": (100, 100, "float64", 6, 2, {}, (4,)),
    "generic_forced_128_f32": (128, 128, "float32", 6, 2, {"DEBUG_NS_GENERIC": 1}, (4, 8)),
}


@pytest.mark.parametrize("case", sorted(_PLANT))
def test_ns_planted_reward_terms(case):
    """One step from a fixed state gives the observation at t = 1; U_ref[1] is set to it except at planted cells (u or v offset),
    gamma = 0, and the same step is taken again: every other term of the reward is exactly 0, so the reward is -1/2 of the sum
    of the planted squared differences over nx * ny.  A dropped, doubled or misplaced term is an error of its own size."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    ny, nx, dts, K, B, sw, tile = _PLANT[case]
    dtype = getattr(torch, dts)
    T = np.float64 if dts == "float64" else np.float32
    eps = float(np.finfo(T).eps)
    kw, ic, _, acts = _ns_data(ny, nx, 1, K, 4242 + ny + nx)
    kw["gamma"] = 0.0
    ic = np.repeat(ic, B, axis=1)                               # the same state in every instance (U_ref is shared)
    a = torch.as_tensor(np.repeat(acts[0], B, axis=0), dtype=dtype, device="cuda")
    rng = np.random.default_rng(len(case))
    with _switches(**sw):
        env = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, **kw)
        env.reset(*ic)
        o1 = env.step(a)[0].cpu().numpy()[0].copy()
        for name, cells in _plant_sets(ny, nx, rng, tile).items():
            uref = np.zeros((NT, ny, nx, 2), dtype=T)
            uref[1] = o1
            comp = rng.integers(0, 2, len(cells))
            # |offset| >= 1: every planted term (>= 1) stays above the tolerance below (k + 3) eps(T) * sum (sum <= 4 k) even
            # for the 1020 cells of the 256^2 ring in float32, so a single dropped or misplaced term always fails
            off = rng.uniform(1.0, 2.0, len(cells)) * rng.choice([-1.0, 1.0], len(cells))
            for (i, j), c, d in zip(cells, comp, off):
                uref[1, i, j, c] = T(o1[i, j, c] + d)
            env2 = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, **dict(kw, U_ref=uref.astype(np.float64)))
            env2.reset(*ic)
            obs, r, _ = env2.step(a)
            assert bits_equal(obs.cpu().numpy()[0], o1)
            terms = [float(T(o1[i, j, c] - uref[1, i, j, c]) * T(o1[i, j, c] - uref[1, i, j, c])) for (i, j), c in zip(cells, comp)]
            want = -0.5 * math.fsum(terms) / nx / ny
            got = r.cpu().numpy().astype(np.float64)
            tol = (len(cells) + 3) * eps
            bad = np.abs(got - want) > tol * abs(want)
            assert not bad.any(), (f"{case} plant {name} ({len(cells)} cells): reward {got[bad]} vs fsum {want!r} "
                                   f"(relative error {np.abs(got - want).max() / abs(want):.3g}, tolerance {tol:.3g}; "
                                   f"one term is about {min(terms) / sum(terms):.3g} of the sum)")


# ---- the other families: shards equal the whole batch ---------------------------------------------------------------
def test_parabolic_1d_shards_equal_the_whole_batch():
    """BASELINE config 2's shape (Parabolic1D, nx = 256, float32), 2048 instances against 8 shards of 256."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    B, S, n = 2048, 8, 257
    rng = np.random.default_rng(3)
    x = np.linspace(0, 1, n)
    init = (rng.uniform(1, 10, (B, 1)) * np.ones((1, n))).astype(np.float32)
    beta = (50 * np.cos(rng.uniform(7.5, 8.5, (B, 1)) * np.arccos(x))).astype(np.float32)
    acts = rng.uniform(-1, 1, (4, B)).astype(np.float32)

    def run(lo, hi):
        dx = 1.0 / 256
        dt = 0.25 * dx * dx
        env = PDEBatch1D("parabolic", 300 * dt, dt, 1, dx, 100 * dt, limit_pde_state_size=True,
                         reward=RewardSpec(N.REWARD_TUNED1D, 300, -1e3, 3e2), num_envs=hi - lo, device="cuda")
        env.reset(torch.tensor(init[lo:hi]), torch.tensor(beta[lo:hi]))
        res = []
        for a in acts:
            obs, r, te, tr = env.step(torch.tensor(a[lo:hi], device="cuda"))
            res.append([z.cpu().numpy().copy() for z in (obs, r, te, tr, env.u)])
        return res

    whole = run(0, B)
    parts = [run(s * B // S, (s + 1) * B // S) for s in range(S)]
    for t in range(len(acts)):
        for k, name in enumerate(("obs", "reward", "terminated", "truncated", "u")):
            _assert_bits(np.concatenate([p[t][k] for p in parts]), whole[t][k], f"parabolic shards step {t}: {name}")


def test_traffic_shards_equal_the_whole_batch():
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    B, S = 2048, 8
    rng = np.random.default_rng(11)
    rs = rng.choice([0.115, 0.12, 0.125], B)
    qclip = rng.choice([0.115, 0.12, 0.125], B)
    qclip = qclip * (40 * (1 - qclip / 0.16))
    scale = rng.uniform(0.7, 1.3, (12, B, 1))

    def run(lo, hi):
        env = TrafficBatch(240, 0.25, 500, 10, "outlet", 40, 0.16, 60, True, 2, num_envs=hi - lo, device="cuda")
        env.set_action_bounds(qclip[lo:hi])
        env.reset(rs[lo:hi])
        qs = (rs * 40 * (1 - rs / 0.16))[lo:hi, None]          # the steady flux q_s = r_s v_s
        res = []
        for s in scale:
            o, r, d, tr = env.step(s[lo:hi] * qs)
            res.append([z.cpu().numpy().copy() for z in (o, r, d, tr, env.t["r"], env.t["y"])])
        return res

    whole = run(0, B)
    parts = [run(s * B // S, (s + 1) * B // S) for s in range(S)]
    for t in range(len(scale)):
        for k, name in enumerate(("obs", "reward", "done", "truncated", "r", "y")):
            _assert_bits(np.concatenate([p[t][k] for p in parts]), whole[t][k], f"traffic shards step {t}: {name}")


def test_tumor_shards_equal_the_whole_batch():
    from pdecontrolgym_amd.batch_tumor import TumorBatch
    B, S, T = 2048, 8, 12
    rng = np.random.default_rng(5)
    xs = np.linspace(0, 200, 201)
    init = 0.8 * 1e5 * np.exp(-0.25 * xs ** 2)[None] * rng.uniform(0.9, 1.1, (B, 1))
    tb = np.where(rng.random(B) < 0.2, np.nan, rng.integers(2, 10, B).astype(np.float64))
    acts = rng.uniform(0, 1, (T + 2, B)) * rng.uniform(0.02, 0.3, B)

    def run(lo, hi):
        eng = TumorBatch(T, 1, 200, 1, 61.2, num_envs=hi - lo)
        eng.set_benchmark(tb[lo:hi])
        eng.reset(init[lo:hi])
        res = []
        for a in acts:
            u, r, te, tr = eng.step(a[lo:hi])
            res.append([np.asarray(z.cpu().numpy() if hasattr(z, "cpu") else z).copy() for z in (u, r, te, tr)])
        return res

    whole = run(0, B)
    parts = [run(s * B // S, (s + 1) * B // S) for s in range(S)]
    for t in range(len(acts)):
        for k, name in enumerate(("u", "reward", "terminated", "truncated")):
            _assert_bits(np.concatenate([p[t][k] for p in parts]), whole[t][k], f"tumour shards step {t}: {name}")


def test_transport_1d_float64_beta_shards_equal_the_whole_batch():
    """Transport 1D with a float64 beta (the M64 parity mode), 2048 instances against 8 shards of 256."""
    B, S = 2048, 8
    data = _d1_data("transport", 100, B, 11)
    whole = _d1_run("transport", 100, 5, data, np.arange(B), dict(beta64=True))
    parts = [_d1_run("transport", 100, 5, data, np.arange(s * B // S, (s + 1) * B // S), dict(beta64=True)) for s in range(S)]
    for t in range(len(whole)):
        for k in whole[t]:
            _assert_bits(np.concatenate([p[t][k] for p in parts]), whole[t][k], f"transport M64 shards step {t}: {k}")


# ---- the other families: probe rows alone against a larger batch ---------------------------------------------------
# Rows at 0, 15, 16, 63, 64 and the last: the edges of 16-row tiles and of 64-lane waves, where the batched kernels (FusedMLP's
# row tiles, the policy rollouts' cooperative MFMA path, the wave-packed 1D variants) change what a lane or a tile holds.
PROBE_ROWS = (0, 15, 16, 63, 64)
M_ROWS = 70


def _rows(M):
    return sorted({r for r in PROBE_ROWS if r < M} | {M - 1})


def _compare_rows(whole, single, tag):
    """whole: per step a dict of [M, ...] arrays; single[r]: the same for instance r run alone (B = 1)."""
    for r, one in single.items():
        for t, (sw, s1) in enumerate(zip(whole, one)):
            for k in sw:
                _assert_bits(sw[k][r], s1[k][0], f"{tag} row {r}, step {t}: {k}")


def _d1_data(kind, nx, M, seed):
    rng = np.random.default_rng(seed)
    n = nx + (1 if kind == "parabolic" else 0)
    x = np.linspace(0, 1, n)
    init = (rng.uniform(0.5, 3, (M, 1)) * (1 + 0.3 * np.sin(2 * np.pi * x * rng.uniform(0.5, 3, (M, 1))))).astype(np.float32)
    beta = rng.uniform(-2, 2, (M, n))
    pool_i = rng.uniform(0.5, 2, (M, n)).astype(np.float32)
    pool_b = rng.uniform(-2, 2, (M, n))
    acts = rng.uniform(-1, 1, (5, M)).astype(np.float32)
    return init, beta, pool_i, pool_b, acts


def _d1_kw(kind, nx, S, opt):
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
    kw = dict(T=3 * S * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, control_type=opt.get("control", "Dirchilet"),
              sensing_loc="full", sensing_type=None, normalize=True, max_control_value=5.0, limit_pde_state_size=True,
              max_state_value=1e6)
    return kw, int(round(kw["T"] / dt))


def _d1_run(kind, nx, S, data, sel, opt):
    """Step the instances ``sel`` of ``data`` as one PDEBatch1D (fused auto-reset with per-instance pool rows unless the engine
    records the trajectory).  Returns one dict of host arrays per step."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    init, beta, pool_i, pool_b, acts = data
    kw, nt1 = _d1_kw(kind, nx, S, opt)
    hist = bool(opt.get("history"))
    bdt = torch.float64 if opt.get("beta64") else torch.float32
    env = PDEBatch1D(kind, reward=RewardSpec(N.REWARD_TUNED1D, nt1, -1e3, 3e2), num_envs=len(sel), device="cuda",
                     record_history=hist, **kw)
    env.reset(torch.tensor(init[sel]), torch.tensor(beta[sel], dtype=bdt))
    if not hist:
        env.enable_auto_reset(torch.tensor(pool_i[sel]), keep_final_obs=True, beta_pool=torch.tensor(pool_b[sel], dtype=bdt))
    out = []
    for a in acts:
        obs, r, te, tr = env.step(torch.tensor(a[sel], device="cuda"))
        out.append({"obs": obs.cpu().numpy().copy(), "reward": r.cpu().numpy().copy(), "terminated": te.cpu().numpy().copy(),
                    "truncated": tr.cpu().numpy().copy(), "u": env.u.cpu().numpy().copy()})
    return out


# (kind, nx, S, options): EPL classes 1 .. 24, rows that fill the wave (FULL), the history variants (HFAST), float64 beta (M64),
# a Neumann actuator, and the LDS-wide rows above MAX_N1D (one wave per instance, rows in LDS) up to 8192 nodes
_D1_CASES = [("transport", 40, 5, {}), ("parabolic", 100, 5, {}), ("parabolic", 256, 3, {}), ("transport", 512, 3, {}),
             ("transport", 500, 3, {"history": True}), ("parabolic", 255, 3, {"history": True}), ("parabolic", 256, 3, {"beta64": True}),
             ("transport", 128, 4, {"beta64": True}), ("parabolic", 100, 4, {"control": "Neumann"}), ("parabolic", 1500, 2, {}),
             ("transport", 3000, 2, {}), ("transport", 8192, 1, {})]


@pytest.mark.parametrize("kind,nx,S,opt", _D1_CASES, ids=[f"{k}-{n}-S{s}-{'-'.join(o) or 'plain'}" for k, n, s, o in _D1_CASES])
def test_1d_step_rows_do_not_depend_on_batch(kind, nx, S, opt):
    data = _d1_data(kind, nx, M_ROWS, nx + S)
    whole = _d1_run(kind, nx, S, data, np.arange(M_ROWS), opt)
    single = {r: _d1_run(kind, nx, S, data, np.array([r]), opt) for r in _rows(M_ROWS)}
    _compare_rows(whole, single, f"1D {kind} nx={nx} {opt}")


def _mlp(sizes, seed, act=torch.nn.Tanh):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[i], sizes[i + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (1.5 / np.sqrt(sizes[i])))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.3)
        layers += [lin, act()]
    return torch.nn.Sequential(*layers[:-1]).to("cuda")


@pytest.mark.parametrize("hidden", [32, 128], ids=["narrow-32-units", "wide-128-units-mfma"])
@pytest.mark.parametrize("kind,nx,S", [("parabolic", 100, 5), ("transport", 64, 3)])
def test_1d_policy_rollout_rows_do_not_depend_on_batch(kind, nx, S, hidden):
    """One-launch rollouts with the policy inside: layers of <= 64 units, and > 64 units (the cooperative MFMA path)."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    from pdecontrolgym_amd.policy import FusedMLP
    data = _d1_data(kind, nx, M_ROWS, 3 * nx + hidden)
    init, beta, pool_i, pool_b, _ = data
    kw, nt1 = _d1_kw(kind, nx, S, {})
    T = 5
    noise = torch.tensor(np.random.default_rng(hidden).normal(0, 0.2, (T, M_ROWS)).astype(np.float32), device="cuda")
    pol = None

    def run(sel):
        nonlocal pol
        B = len(sel)
        env = PDEBatch1D(kind, reward=RewardSpec(N.REWARD_TUNED1D, nt1, -1e3, 3e2), num_envs=B, device="cuda", **kw)
        env.reset(torch.tensor(init[sel]), torch.tensor(beta[sel], dtype=torch.float32))
        env.enable_auto_reset(torch.tensor(pool_i[sel]), keep_final_obs=True, beta_pool=torch.tensor(pool_b[sel], dtype=torch.float32))
        if pol is None:
            pol = FusedMLP(_mlp([env.obs_dim, hidden, hidden, 1], hidden), clamp=(-1.0, 1.0))
        assert env.policy_fits_rollout(pol)
        od = env.obs_dim
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")   # noqa: E731
        obs, act, rew, te, tr = z(T + 1, B, od), z(T, B), z(T, B), z(T, B, dt=torch.uint8), z(T, B, dt=torch.uint8)
        obs[0].copy_(env.t["obs"].reshape(B, od))
        env.rollout(obs, act, rew, te, tr, policy=pol, noise=noise[:, sel].contiguous())
        return [{"obs": obs[t + 1].cpu().numpy(), "action": act[t].cpu().numpy(), "reward": rew[t].cpu().numpy(),
                 "terminated": te[t].cpu().numpy(), "truncated": tr[t].cpu().numpy()} for t in range(T)]

    whole = run(np.arange(M_ROWS))
    _compare_rows(whole, {r: run(np.array([r])) for r in _rows(M_ROWS)}, f"1D {kind} policy rollout hidden={hidden}")


def _traffic_make(sel, rs, pool):
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    env = TrafficBatch(2.0, 0.25, 500, 10, "outlet", 40, 0.16, 60, True, 1, num_envs=len(sel), device="cuda")
    env.set_action_bounds(rs[sel] * (40 * (1 - rs[sel] / 0.16)))
    env.reset(rs[sel])
    env.enable_auto_reset(pool[sel], keep_final_obs=True)
    return env


@pytest.mark.parametrize("mode", ["step", "rollout", "rollout-wide-policy"])
def test_traffic_rows_do_not_depend_on_batch(mode):
    from pdecontrolgym_amd.policy import FusedMLP
    rng = np.random.default_rng(21)
    rs = rng.choice([0.115, 0.12, 0.125], M_ROWS)
    pool = rng.choice([0.115, 0.12, 0.125], M_ROWS)
    qs = rs * 40 * (1 - rs / 0.16)
    T = 10
    scale = rng.uniform(0.7, 1.3, (T, M_ROWS, 1))
    pol = None

    def run(sel):
        nonlocal pol
        env = _traffic_make(sel, rs, pool)
        B, D = len(sel), 2 * env.M
        if mode == "step":
            res = []
            for s in scale:
                o, r, d, tr = env.step(s[sel] * qs[sel, None])
                res.append({"obs": o.cpu().numpy().copy(), "reward": r.cpu().numpy().copy(), "done": d.cpu().numpy().copy(),
                            "truncated": tr.cpu().numpy().copy()})
            return res
        f64 = torch.float64
        obs, act = torch.zeros(T + 1, B, D, dtype=f64, device="cuda"), torch.zeros(T, B, 1, dtype=f64, device="cuda")
        rew = torch.zeros(T, B, dtype=f64, device="cuda")
        dn, tr = torch.zeros(T, B, dtype=torch.uint8, device="cuda"), torch.zeros(T, B, dtype=torch.uint8, device="cuda")
        obs[0].copy_(env.t["obs"])
        if mode == "rollout":
            act.copy_(torch.tensor(scale[:, sel] * qs[sel, None], device="cuda"))
            env.rollout(obs, act, rew, dn, tr)
        else:
            if pol is None:
                net = _mlp([D, 128, 1], 5)
                with torch.no_grad():
                    net[-1].bias.add_(4.5)
                pol = FusedMLP(net, clamp=(3.0, 6.0))
            assert env.policy_fits_rollout(pol)
            env.rollout(obs, act, rew, dn, tr, policy=pol)
        return [{"obs": obs[t + 1].cpu().numpy(), "action": act[t].cpu().numpy(), "reward": rew[t].cpu().numpy(),
                 "done": dn[t].cpu().numpy(), "truncated": tr[t].cpu().numpy()} for t in range(T)]

    whole = run(np.arange(M_ROWS))
    _compare_rows(whole, {r: run(np.array([r])) for r in _rows(M_ROWS)}, f"traffic {mode}")


@pytest.mark.parametrize("mode", ["step", "advance"])
def test_tumor_rows_do_not_depend_on_batch(mode):
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch_tumor import TumorBatch
    rng = np.random.default_rng(8)
    xs = np.linspace(0, 200, 201)
    init = 0.8 * 1e5 * np.exp(-0.25 * xs ** 2)[None] * rng.uniform(0.9, 1.1, (M_ROWS, 1))
    tb = np.where(rng.random(M_ROWS) < 0.2, np.nan, rng.integers(2, 10, M_ROWS).astype(np.float64))
    acts = rng.uniform(0, 1, (6, M_ROWS)) * rng.uniform(0.02, 0.3, M_ROWS)

    def run(sel):
        eng = TumorBatch(40, 1, 200, 1, 61.2, num_envs=len(sel))
        eng.set_benchmark(tb[sel])
        eng.reset(init[sel])
        res = []

        def grab(u, r, te, tr):
            res.append({"u": u.cpu().numpy().copy(), "reward": r.cpu().numpy().copy(), "terminated": te.cpu().numpy().copy(),
                        "truncated": tr.cpu().numpy().copy()})
        if mode == "step":
            for a in acts:
                grab(*eng.step(a[sel]))
        else:
            grab(*eng.advance(N.TUMOR_RUN_GROWTH))
            for a in acts[:3]:
                grab(*eng.step(a[sel]))
            grab(*eng.advance(N.TUMOR_RUN_TO_END))
        return res

    whole = run(np.arange(M_ROWS))
    _compare_rows(whole, {r: run(np.array([r])) for r in _rows(M_ROWS)}, f"tumour {mode}")


@pytest.mark.parametrize("in_dim,hidden", [(7, 32), (100, 64), (257, 128), (600, 256), (8192, 64)],
                         ids=["in7-h32", "in100-h64", "in257-h128", "in600-h256-several-chunks", "in8192-h64"])
def test_fused_mlp_rows_do_not_depend_on_batch(in_dim, hidden):
    """FusedMLP.forward_into: row r of a batch of 70 equals the same row alone, at the 16-row tile and 64-row wave edges; first
    layers wider than one 512-entry staging chunk and the largest observation (8192)."""
    from pdecontrolgym_amd.policy import FusedMLP
    pol = FusedMLP(_mlp([in_dim, hidden, hidden, 2], in_dim + hidden), clamp=None)
    x = torch.tensor(np.random.default_rng(in_dim).normal(0, 1, (M_ROWS, in_dim)).astype(np.float32), device="cuda")
    whole = torch.zeros(M_ROWS, 2, device="cuda")
    pol.forward_into(x, whole)
    for r in _rows(M_ROWS):
        one = torch.zeros(1, 2, device="cuda")
        pol.forward_into(x[r:r + 1].contiguous(), one)
        _assert_bits(whole[r].cpu().numpy(), one[0].cpu().numpy(), f"FusedMLP in={in_dim} hidden={hidden} row {r}")
