#!/usr/bin/env python3
"""Differential fuzz of the NS2D (float64 bit-exact; float32 tiled == generic), traffic and brain-tumour kernels against the
oracle (test infrastructure; run on a GPU box):   python tests/fuzz_more.py [seconds] [seed]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pde_oracle as po  # noqa: E402

BCS = ["Neumann", "Dirchilet", "Controllable"]


def _dbg(key, value):
    """Test-only kernel dispatch override (pdegym_debug_set, include/pdegym.h); takes ints or the "0"/"1" strings looped over."""
    from pdecontrolgym_amd import _native as N
    N.load().pdegym_debug_set(getattr(N, key), int(value))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    ui = np.uint64 if a.dtype == np.float64 else np.uint32
    fin = ~(np.isnan(a) & np.isnan(b))
    return np.array_equal(a.view(ui)[fin], b.view(ui)[fin])


def draw_plant(idx, salt):
    """About one case in ten carries a non-finite value (tests/test_gpu_nonfinite.py holds the fixed cases): returns None, or a
    generator of its own from which the case draws what to plant and where -- the case's main stream is left as it was."""
    prng = np.random.default_rng([idx, salt])
    return prng if prng.random() < 0.1 else None


PLANTS = [float("nan"), float("inf"), float("-inf")]


def ns_case(rng, idx):
    from pdecontrolgym_amd.batch2d import NSBatch2D
    n = int(rng.choice([3, 4, 5, 8, 16, 21, 32, 33, 40, 63, 64, 65, 70, 100, 128])) if rng.random() < 0.7 else int(rng.integers(3, 90))
    K = int(rng.choice([0, 1, 2, 3, 7, 20, 50, 51]))
    B = int(rng.choice([1, 2, 3, 5]))
    adim = int(rng.choice([1, 1, n]))
    bc = {e: [str(rng.choice(BCS)), str(rng.choice(BCS))] for e in ("upper", "lower", "left", "right")}
    # non-square grids and cells: nx = round(X/dx + 1) columns, ny = round(Y/dy + 1) rows (base_env_2d.py:27-36)
    m = n if rng.random() < 0.5 else int(rng.choice([3, 4, 5, 8, 9, 11, 16, 21, 21, 26, 31, 32, 33, 64, 65]))
    dx = 1.0 / (n - 1)
    dy = (1.0 if rng.random() < 0.6 else 0.5) / (m - 1)
    Yl = dy * (m - 1)
    nu = float(rng.choice([0.1, 0.01, 1.0]))
    dt = 0.2 * 0.5 * min(dx, dy) ** 2 / nu * float(rng.choice([1.0, 0.5]))
    nt = int(rng.integers(3, 7))
    inter = bool(rng.random() < 0.5)
    adim = int(rng.choice([1, 1, max(n, m)])) if n == m else 1
    Xg, Yg = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, Yl, m))
    style = rng.choice(["smooth", "const", "zero", "rand"])
    def field():
        if style == "smooth":
            return np.stack([np.sin(2 * np.pi * Xg * rng.uniform(0.5, 2)) * np.cos(np.pi * Yg) * rng.uniform(0.5, 2) + rng.uniform(-1, 1) for _ in range(B)])
        if style == "const":
            return np.stack([np.full((m, n), rng.uniform(-5, 5)) for _ in range(B)])
        if style == "zero":
            return np.zeros((B, m, n))
        return rng.uniform(-1, 1, (B, m, n))
    u0, v0, p0 = field(), field(), field()
    plant = draw_plant(idx, 1)
    nan_cmd = None
    if plant is not None:          # a NaN cell in the initial u or p of one instance, or a NaN command at the first step
        what = int(plant.integers(3))
        where = (int(plant.integers(B)), int(plant.integers(m)), int(plant.integers(n)))
        if what < 2:
            (u0, p0)[what][where] = np.nan
        else:
            nan_cmd = where[0]
    kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=Yl, dy=dy, boundary_condition=bc, U_ref=rng.uniform(-1, 1, (nt, m, n, 2)),
              action_ref=rng.uniform(1, 3, nt), gamma=float(rng.choice([0.1, 0.0, 2.0])), maximum_pressure_iteration=K, viscosity=nu,
              density=float(rng.choice([1.0, 2.0])))
    desc = f"#{idx} ns nx={n} ny={m} K={K} B={B} adim={adim} nt={nt} inter={inter} ic={style} bc={bc} plant={plant is not None}"
    # grids of 8 / 11 / 16 / 21 / 26 / 31 / 32 rows and up to 64 columns: half of the cases on the column-per-lane kernel (which float64
    # batches this small would not reach by themselves), half on the workgroup kernel -- the switch is read at every launch
    col = rng.random() < 0.5
    _dbg("DEBUG_NS_COL_MIN_BATCH", "0" if col else "1000000")
    desc += f" col={col}"
    orc = po.NavierStokesOracle(**kw)
    env = NSBatch2D(num_envs=B, device="cuda", dtype=torch.float64, interleaved_state=inter, action_dim=adim, **kw)
    orc.reset(u0, v0, p0)
    env.reset(u0, v0, p0)
    for i in range(nt - 1):      # U_ref[t] is read after the increment: the reference cannot step further either
        a = rng.uniform(2, 4, (B, adim)) * float(rng.choice([1.0, 0.0, -1.0]))
        if nan_cmd is not None and i == 0:
            a[nan_cmd, 0] = np.nan
        with np.errstate(invalid="ignore"):
            o_ref, r_ref, te_ref, _ = orc.step(a)
        obs, r, te = env.step(a)
        assert bits_equal(obs.cpu().numpy(), o_ref), desc + f" step {i}: obs"
        assert bits_equal(env.p.cpu().numpy(), orc.p), desc + f" step {i}: p"
        assert np.allclose(r.cpu().numpy(), r_ref, rtol=1e-12, atol=1e-300, equal_nan=True), desc + f" step {i}: reward {r.cpu().numpy()} {r_ref}"
        assert np.array_equal(te.cpu().numpy().astype(bool), te_ref), desc + f" step {i}: terminate"
    _dbg("DEBUG_NS_COL_MIN_BATCH", -1)
    # the column kernel and the workgroup kernel: every output bit for bit, rewards included (one summation order)
    if m in (8, 11, 16, 21, 26, 31, 32) and n <= 64:
        outs = []
        for mb in ("0", "1000000"):
            _dbg("DEBUG_NS_COL_MIN_BATCH", mb)
            try:
                e2 = NSBatch2D(num_envs=B, device="cuda", dtype=torch.float64, interleaved_state=inter, action_dim=adim, **kw)
                e2.reset(u0, v0, p0)
                acts = np.random.default_rng(idx + 1).uniform(2, 4, (nt - 1, B, adim))
                res = []
                for a in acts:
                    obs, r, te = e2.step(a)
                    res.append((obs.cpu().numpy().copy(), e2.p.cpu().numpy().copy(), r.cpu().numpy().copy()))
                outs.append(res)
            finally:
                _dbg("DEBUG_NS_COL_MIN_BATCH", -1)
        for (o1, p1, r1), (o2, p2, r2) in zip(*outs):
            assert bits_equal(o1, o2) and bits_equal(p1, p2), desc + " column != workgroup (fields)"
            assert bits_equal(r1, r2), desc + f" column != workgroup (rewards {r1} {r2})"
    # float32: tiled kernel == generic kernel for the sizes the tiled path exists for
    if n == m and n in (64, 128):
        outs = []
        for force in ("0", "1"):
            _dbg("DEBUG_NS_GENERIC", force)
            e32 = NSBatch2D(num_envs=B, device="cuda", dtype=torch.float32, interleaved_state=inter, action_dim=adim, **kw)
            e32.reset(u0, v0, p0)
            acts = np.random.default_rng(idx).uniform(2, 4, (2, B, adim))
            res = []
            for a in acts:
                obs, r, te = e32.step(a)
                res.append((obs.cpu().numpy().copy(), e32.p.cpu().numpy().copy()))
            outs.append(res)
        _dbg("DEBUG_NS_GENERIC", "0")
        for (o1, p1), (o2, p2) in zip(*outs):
            assert bits_equal(o1, o2) and bits_equal(p1, p2), desc + " f32 tile != generic"
    return desc


def ns256_case(rng, idx):
    """256 x 256 (BASELINE config 5): the float64 slab-pass pipeline against the oracle and the float32 fused launch against the
    workgroup kernel, bit for bit -- random boundary sets, per-node actions, sweep counts around the pass boundaries (17, 34),
    zero / constant / random fields (a zero field puts denormals and signed zeros through the sweeps)."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    n = 256
    K = int(rng.choice([0, 1, 2, 3, 16, 17, 18, 33, 34, 35, 50, 51]))
    B = int(rng.choice([1, 2, 3]))
    adim = int(rng.choice([1, 1, n]))
    bc = {e: [str(rng.choice(BCS)), str(rng.choice(BCS))] for e in ("upper", "lower", "left", "right")}
    dx = 1.0 / (n - 1)
    nu = float(rng.choice([0.1, 0.01, 1.0]))
    dt = 0.2 * 0.5 * dx ** 2 / nu * float(rng.choice([1.0, 0.5]))
    nt = 4
    inter = bool(rng.random() < 0.6)
    Xg, Yg = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n))
    style = rng.choice(["smooth", "const", "zero", "rand", "tiny"])
    def field():
        if style == "smooth":
            return np.stack([np.sin(2 * np.pi * Xg * rng.uniform(0.5, 2)) * np.cos(np.pi * Yg) * rng.uniform(0.5, 2) + rng.uniform(-1, 1) for _ in range(B)])
        if style == "const":
            return np.stack([np.full((n, n), rng.uniform(-5, 5)) for _ in range(B)])
        if style == "zero":
            return np.zeros((B, n, n))
        if style == "tiny":
            return rng.uniform(-1, 1, (B, n, n)) * 1e-300
        return rng.uniform(-1, 1, (B, n, n))
    u0, v0, p0 = field(), field(), field()
    kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=1, dy=dx, boundary_condition=bc, U_ref=rng.uniform(-1, 1, (nt, n, n, 2)),
              action_ref=rng.uniform(1, 3, nt), gamma=float(rng.choice([0.1, 0.0, 2.0])), maximum_pressure_iteration=K, viscosity=nu,
              density=float(rng.choice([1.0, 2.0])))
    desc = f"#{idx} ns256 K={K} B={B} adim={adim} inter={inter} ic={style} bc={bc}"
    orc = po.NavierStokesOracle(**kw)
    env = NSBatch2D(num_envs=B, device="cuda", dtype=torch.float64, interleaved_state=inter, action_dim=adim, **kw)
    orc.reset(u0, v0, p0)
    env.reset(u0, v0, p0)
    with np.errstate(all="ignore"):
        for i in range(2):
            a = rng.uniform(2, 4, (B, adim)) * float(rng.choice([1.0, 0.0, -1.0]))
            o_ref, r_ref, te_ref, _ = orc.step(a)
            obs, r, te = env.step(a)
            assert bits_equal(obs.cpu().numpy(), o_ref), desc + f" step {i}: obs (float64)"
            assert bits_equal(env.p.cpu().numpy(), orc.p), desc + f" step {i}: p (float64)"
            assert bits_equal(env.u.cpu().numpy(), o_ref[..., 0]), desc + f" step {i}: u (float64)"
            assert np.allclose(r.cpu().numpy(), r_ref, rtol=1e-12, atol=1e-300), desc + f" step {i}: reward"
    outs = []
    u32, v32, p32 = (x.astype(np.float32) if style != "tiny" else (x * 1e262).astype(np.float32) for x in (u0, v0, p0))
    for force in ("0", "1"):
        _dbg("DEBUG_NS_GENERIC", force)
        try:
            e32 = NSBatch2D(num_envs=B, device="cuda", dtype=torch.float32, interleaved_state=inter, action_dim=adim, **kw)
            e32.reset(u32, v32, p32)
            acts = np.random.default_rng(idx).uniform(2, 4, (2, B, adim))
            res = []
            for a in acts:
                obs, r, te = e32.step(a)
                res.append((obs.cpu().numpy().copy(), e32.p.cpu().numpy().copy(), e32.u.cpu().numpy().copy()))
            outs.append(res)
        finally:
            _dbg("DEBUG_NS_GENERIC", "0")
    for (o1, p1, u1), (o2, p2, u2) in zip(*outs):
        assert bits_equal(o1, o2) and bits_equal(p1, p2) and bits_equal(u1, u2), desc + " float32 fused launch != workgroup kernel"
    return desc


def traffic_case(rng, idx):
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    sim = str(rng.choice(["inlet", "outlet", "both", "outlet-train"]))
    cf = int(rng.choice([1, 2, 3, 5]))
    B = int(rng.choice([1, 2, 7, 33, 64, 65]))
    dxs = float(rng.choice([10, 20, 12.5, 8, 5, 4, 2, 1, 0.5]))
    X = float(rng.choice([500, 400, 250]))
    dt = float(rng.choice([0.25, 0.1])) if dxs >= 8 else float(rng.choice([0.02, 0.01])) * dxs
    limit = bool(rng.random() < 0.7)
    T = float(rng.choice([240, 5, 2]))
    M = len(np.arange(0, X + dxs, dxs))
    if M > 1024:
        return None
    desc = f"#{idx} traffic {sim} cf={cf} B={B} X={X} dx={dxs} dt={dt} T={T} limit={limit} plant={draw_plant(idx, 2) is not None}"
    orc = po.TrafficOracle(T, dt, X, dxs, sim, 40, 0.16, 60, limit, cf)
    env = TrafficBatch(T, dt, X, dxs, sim, 40, 0.16, 60, limit, cf, num_envs=B, device="cuda")
    rs = rng.choice([0.115, 0.12, 0.125, 0.1], B)
    qclip = rng.choice([0.115, 0.12, 0.125], B)
    qclip = qclip * (40 * (1 - qclip / 0.16))
    env.set_action_bounds(qclip)
    o_ref = orc.reset(rs, qclip)
    o = env.reset(rs)
    assert bits_equal(o.cpu().numpy(), o_ref), desc + " reset"
    nact = 2 if sim == "both" else 1
    plant = draw_plant(idx, 2)
    for k in range(int(rng.integers(3, 30))):
        a = rng.uniform(0.5, 1.5, (B, nact)) * orc.qs[:, None]
        if plant is not None and k == 1:          # a NaN / +Inf / -Inf command of one instance
            a[int(plant.integers(B)), int(plant.integers(nact))] = PLANTS[int(plant.integers(3))]
        with np.errstate(all="ignore"):
            o_ref, r_ref, d_ref, t_ref = orc.step(a)
        o, r, d, t = env.step(a)
        assert bits_equal(o.cpu().numpy(), o_ref), desc + f" step {k}: obs"
        assert bits_equal(env.t["r"].cpu().numpy(), orc.r) and bits_equal(env.t["y"].cpu().numpy(), orc.y), desc + f" step {k}: fields"
        assert np.allclose(r.cpu().numpy(), r_ref, rtol=1e-12, equal_nan=True), desc + f" step {k}: reward"
        assert np.array_equal(d.cpu().numpy().astype(bool), d_ref) and np.array_equal(t.cpu().numpy().astype(bool), t_ref), desc + f" step {k}: flags"
    return desc


def tumor_case(rng, idx):
    from pdecontrolgym_amd.batch_tumor import TumorBatch
    from pdecontrolgym_amd import _native as N
    X = int(rng.choice([200, 100, 64, 300]))
    dx = float(rng.choice([1, 1, 0.5, 2]))
    T = int(rng.choice([600, 300, 260, 100]))
    B = int(rng.choice([1, 3, 4, 5, 9]))
    tot = float(rng.choice([61.2, 30.0, 100.0]))
    kwp = dict(t1_detection_threshold=float(rng.choice([0.8, 0.6])), t2_detection_threshold=float(rng.choice([0.16, 0.3])),
               dosage_termination_threshold=float(rng.choice([0.1, 1.0])), D=float(rng.choice([0.2, 0.1, 0.05])), rho=float(rng.choice([0.03, 0.05])),
               alpha=float(rng.choice([0.04, 0.1])), alpha_beta_ratio=float(rng.choice([10, 3])), k=float(rng.choice([1e5, 1.0, 3e4])),
               t1_detection_radius=float(rng.choice([15, 10])), t1_death_radius=float(rng.choice([35, 25])))
    if kwp["D"] * 1 / dx ** 2 > 0.45:
        return None
    desc = f"#{idx} tumor X={X} dx={dx} T={T} B={B} tot={tot} {kwp}"
    orc = po.BrainTumorOracle(T, 1, X, dx, tot, **kwp)
    eng = TumorBatch(T, 1, X, dx, tot, num_envs=B, **kwp)
    xs = np.linspace(0, X, orc.nx)
    init = (0.8 * kwp["k"] * np.exp(-0.25 * xs ** 2))[None] * rng.uniform(0.8, 1.0, (B, 1))
    tb = np.where(rng.random(B) < 0.3, np.nan, rng.integers(100, 400, B).astype(np.float64))
    plant = draw_plant(idx, 3)
    dose_day = -1
    if plant is not None:          # a NaN cell in one initial profile, or a NaN / +Inf / -Inf request on one of the daily steps
        if plant.random() < 0.5:
            init[int(plant.integers(B)), int(plant.integers(orc.nx))] = np.nan
        else:
            dose_day = int(plant.integers(0, 5))
        desc += " plant"
    eng.set_benchmark(tb)
    eng.reset(init)
    orc.reset(init, tb)
    mode = rng.choice(["daily", "loops"])
    hi = rng.uniform(0.02, 0.4, B)
    if mode == "loops":          # growth in one launch, then daily therapy, then post in one launch
        eng.advance(N.TUMOR_RUN_GROWTH)
        for _ in range(T):
            part = (orc.stage == po.GROWTH) & (orc.time_index < orc.nt - 1)
            if not part.any():
                break
            keep = [np.copy(x) for x in (orc.u, orc.time_index, orc.stage, orc.remaining, orc.growthDays, orc.therapyDays, orc.postDays, orc.simulationDays, orc.cDeathDay)]
            with np.errstate(invalid="ignore"):
                orc.step(np.zeros(B))
            new = [orc.u, orc.time_index, orc.stage, orc.remaining, orc.growthDays, orc.therapyDays, orc.postDays, orc.simulationDays, orc.cDeathDay]
            merged = [np.where(part.reshape((-1,) + (1,) * (k.ndim - 1)), n_, k) for k, n_ in zip(keep, new)]
            (orc.u, orc.time_index, orc.stage, orc.remaining, orc.growthDays, orc.therapyDays, orc.postDays, orc.simulationDays, orc.cDeathDay) = merged
        assert bits_equal(eng.t["u"].cpu().numpy(), orc.u), desc + " growth run: rows"
        assert np.array_equal(eng.t["time_index"].cpu().numpy(), orc.time_index) and np.array_equal(eng.t["stage"].cpu().numpy(), orc.stage), desc + " growth run: state"
    for n in range(int(rng.integers(5, 60))):
        a = rng.uniform(0, 1, B) * hi
        if n == dose_day:
            a[int(plant.integers(B))] = PLANTS[int(plant.integers(3))]
        try:
            with np.errstate(invalid="ignore", over="ignore"):
                o, ro, teo, tro = orc.step(a)
        except ZeroDivisionError:      # treatment radius 0 (tumour invisible on T2): the reference's reward raises
            return desc + " (reference raises)"
        u, r, te, tr = eng.step(a)
        assert np.allclose(u.cpu().numpy(), o, rtol=1e-12, atol=0, equal_nan=True), desc + f" day {n}: rows"
        assert np.allclose(r.cpu().numpy(), ro, rtol=1e-11, atol=0, equal_nan=True), desc + f" day {n}: reward {r.cpu().numpy()} {ro}"
        assert np.array_equal(te.cpu().numpy().astype(bool), teo) and np.array_equal(tr.cpu().numpy().astype(bool), tro), desc + f" day {n}: flags"
        assert np.array_equal(eng.t["stage"].cpu().numpy(), orc.stage), desc + f" day {n}: stage"
        d = eng.t["days"].cpu().numpy()
        assert np.array_equal(d, np.stack([orc.growthDays, orc.therapyDays, orc.postDays, orc.simulationDays, orc.cDeathDay], axis=1)), desc + f" day {n}: days"
        # keep both sides on identical rows (the in-kernel exp may differ from libm's in the last bit)
        orc.u = u.cpu().numpy().copy()
    return desc


if __name__ == "__main__":
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    which = sys.argv[3].split(",") if len(sys.argv) > 3 else ["ns", "ns256", "traffic", "tumor"]
    fns = {"ns": ns_case, "ns256": ns256_case, "traffic": traffic_case, "tumor": tumor_case}
    rng = np.random.default_rng(seed)
    t0, k = time.time(), 0
    counts = {w: 0 for w in which}
    while time.time() - t0 < seconds:
        w = which[k % len(which)]
        d = fns[w](rng, k)
        counts[w] += d is not None
        k += 1
        if k % 30 == 0:
            print(f"{k} cases ok {counts}  last: {d}"[:300], flush=True)
    print(f"FUZZ OK: {counts}, seed {seed}")
