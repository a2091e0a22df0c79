"""What the squashed-Gaussian (SAC) actor head costs, and what it saves: three measurements on ONE device, medians of repeated regions.

    python tools/measure_gaussian_head.py --parent-tree DIR [--rounds 3] [--window 0.3] [--out profiles/<tag>_gaussian_head.json]

1. ``plain``: the plain-head workloads that have a policy inside -- bench.py's policy-in-the-loop secondaries (257-64-64-1 tanh and the
   256-256 ReLU actor, forward + step and 25 env-steps per launch) -- in the PARENT build (``--parent-tree``: a checkout of the parent
   commit with its library built) and in this one, ALTERNATING, a fresh process per build and round.  The feature adds one wave-uniform
   branch per env-step to the rollout kernels; the yardstick is the parent, the margin the parent's own spread over its rounds.
2. ``gaussian_vs_deterministic``: the Gaussian head (eps given) against the deterministic 256-256 actor of the same build -- latent + mu +
   tanh, today's ``from_sb3`` -- inside the one-launch rollouts: C2-shaped reaction-diffusion, two-command traffic, brain tumour.
3. ``gaussian_vs_composed``: the one-launch Gaussian rollout against what a user composes without the head -- a ``FusedMLP`` forward
   producing the 2A raw outputs, the elementwise torch ops of the formula and the step launch, all in one hipGraph -- for the 64-64
   and the 256-256 actor on the C2-shaped environment.
A region is N consecutive calls between two HIP events, N chosen so that it lasts at least ``--window`` seconds; five regions per path,
the paths of one comparison alternating.  Needs a GPU: there is no CPU path.  A measurement that fails is recorded with its error
and the others go on."""
import argparse
import json
import os
import subprocess
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("parabolic_c2_policy_loop", "parabolic_c2_rollout", "parabolic_c2_policy_loop_256", "parabolic_c2_rollout_256")
REGIONS = 5


def region(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def alternate(paths, seconds, unit_per_call):
    """{name: fn} -> {name: microseconds per unit}, the paths' regions alternating."""
    for fn in paths.values():
        for _ in range(3):
            fn()
    per_call = min(region(fn, 3) / 3 for fn in paths.values())
    n = max(3, int(np.ceil(seconds / per_call)))
    times = {k: [] for k in paths}
    for _ in range(REGIONS):
        for k, fn in paths.items():
            times[k].append(region(fn, n) / (n * unit_per_call) * 1e6)
    return {k: dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in times.items()}, n


# ---- worker: the plain-head workloads of bench.py in the build of --tree ------------------------------------------------------------------
def worker_plain(tree, seconds):
    sys.path.insert(0, tree)
    import torch
    import bench
    from pdecontrolgym_amd import build as B_
    out = {"tree": tree, "library_stamp": B_.library_stamp()[:16], "device": torch.cuda.get_device_name(0)}
    for name in PLAIN:
        try:
            wl = bench.WORKLOADS[name](torch.device("cuda", 0), 1234)
            wl.prepare(64)
            chunk = getattr(wl, "CHUNK", 1)
            res, n = alternate({name: wl.step}, seconds, chunk)
            out[name] = dict(res[name], calls_per_region=n, unit="microseconds per env-step of the batch of 4096")
            del wl
        except Exception:      # noqa: BLE001
            out[name] = {"error": traceback.format_exc(limit=3)}
    print("RESULT " + json.dumps(out), flush=True)


# ---- worker: the Gaussian head in this build ----------------------------------------------------------------------------------------------
def _actor(n_in, hidden, A, first_scale):
    import torch
    torch.manual_seed(0)
    lat = torch.nn.Sequential(torch.nn.Linear(n_in, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden), torch.nn.ReLU()).cuda()
    mu, ls = torch.nn.Linear(hidden, A).cuda(), torch.nn.Linear(hidden, A).cuda()
    with torch.no_grad():
        lat[0].weight.mul_(first_scale)
        ls.bias.fill_(-1.0)
    return lat, mu, ls


def _c2(B):
    import pde_control_gym
    from pde_control_gym.src import TunedReward1D
    nx, S = 256, 100
    dx = 1.0 / nx
    dt = 0.25 * dx * dx
    rng = np.random.default_rng(0)

    def reset(idx, n):
        x = np.linspace(0, 1, nx + 1)
        beta = 50.0 * np.cos(rng.uniform(7.5, 8.5, (len(idx), 1)) * np.arccos(x))
        return (rng.uniform(1, 10, (len(idx), 1)) * np.ones((1, nx + 1))).astype(np.float32), beta.astype(np.float32)
    venv = pde_control_gym.make_vec("PDEControlGym-ReactionDiffusionPDE1D", num_envs=B, T=1000 * S * dt, dt=dt, X=1, dx=dx,
                                    reward_class=TunedReward1D(1000 * S, -1e3, 3e2), normalize=True, sensing_loc="full", control_type="Dirchilet",
                                    sensing_type=None, sensing_noise_func=None, limit_pde_state_size=True, max_state_value=1e10,
                                    max_control_value=20, control_sample_rate=S * dt, batched_reset_func=reset)
    venv.reset_tensor()
    venv.enable_fused_auto_reset()
    return venv, 257, 1, (-1.0, 1.0), 0.1


def _traffic(B):
    import random
    import pde_control_gym
    from pde_control_gym.src import TrafficARZReward
    random.seed(0)
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, reward_class=TrafficARZReward(), simulation_type="both",
                                    limit_pde_state_size=True, control_freq=2, T=240, dt=0.25, X=500, dx=10, v_steady=10, ro_steady=0.12,
                                    v_max=40, ro_max=0.16, tau=60)
    venv.reset_tensor()
    return venv, 102, 2, (3.0, 6.0), 0.3


def _tumor(B):
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import measure_tumor_rollout as mt
    return mt.build(B, True, False), 201, 1, (0.0, 1.0), 1e-5


class Composed:
    """What a user composes without the head: a FusedMLP forward producing the 2A raw outputs, then the formula in torch ops; call k of a
    captured rollout reads row k mod T of eps."""

    def __init__(self, lat, mu, ls, eps, box):
        import torch
        from pde_control_gym import FusedMLP
        A = mu.weight.shape[0]
        fused = torch.nn.Linear(mu.weight.shape[1], 2 * A).cuda()
        with torch.no_grad():
            fused.weight.copy_(torch.cat([mu.weight, ls.weight]))
            fused.bias.copy_(torch.cat([mu.bias, ls.bias]))
        self.raw_net, self.A, self.eps, self.box, self.k = FusedMLP(torch.nn.Sequential(*lat, fused)), A, eps, box, 0
        self.raw = torch.empty(eps.shape[1], 2 * A, device="cuda")

    def __call__(self, obs):
        import torch
        A, (lo, hi) = self.A, self.box
        e = self.eps[self.k % self.eps.shape[0]].reshape(-1, A)
        self.k += 1
        self.raw_net.forward_into(obs, self.raw)
        z = self.raw[:, :A] + self.raw[:, A:].clamp(-20.0, 2.0).exp() * e
        return lo + (0.5 * (torch.tanh(z) + 1.0)) * (hi - lo)


def worker_gaussian(seconds, B):
    sys.path.insert(0, HERE)
    import torch
    from pde_control_gym import DeviceRollout, FusedMLP
    out = {"device": torch.cuda.get_device_name(0), "batch": B}
    T = 25

    def rollout(make, pol, noise, one_launch, box=None):
        venv, n_in, A, bx, _ = make(B)
        ro = DeviceRollout(venv, pol, T, use_graph=True, action_low=(box or bx)[0], action_high=(box or bx)[1], action_noise=noise, one_launch=one_launch)
        assert ro.one_launch is bool(one_launch)
        if noise:
            ro.action_noise.normal_()
        return ro
    for name, make in (("c2", _c2), ("traffic_both", _traffic), ("tumor", _tumor)):
        try:
            _, n_in, A, box, scale = make(2)
            lat, mu, ls = _actor(n_in, 256, A, scale)
            det = FusedMLP(torch.nn.Sequential(*lat, mu, torch.nn.Tanh()), clamp=box)
            gau = FusedMLP.squashed_gaussian(lat, mu, ls)
            paths = {"deterministic_256_256": rollout(make, det, False, True).run, "gaussian_256_256": rollout(make, gau, True, True).run}
            res, n = alternate(paths, seconds, T)
            res["ratio_gaussian_over_deterministic"] = round(res["gaussian_256_256"]["median"] / res["deterministic_256_256"]["median"], 4)
            out["gaussian_vs_deterministic_" + name] = dict(res, calls_per_region=n, unit="microseconds per env-step of the batch")
        except Exception:      # noqa: BLE001
            out["gaussian_vs_deterministic_" + name] = {"error": traceback.format_exc(limit=3)}
        torch.cuda.synchronize()
    for hidden in (64, 256):
        try:
            _, n_in, A, box, scale = _c2(2)
            lat, mu, ls = _actor(n_in, hidden, A, scale)
            one = rollout(_c2, FusedMLP.squashed_gaussian(lat, mu, ls), True, True)
            comp = rollout(_c2, Composed(lat, mu, ls, one.action_noise, box), False, False)
            res, n = alternate({"one_launch": one.run, "composed_graph": comp.run}, seconds, T)
            res["ratio_composed_over_one_launch"] = round(res["composed_graph"]["median"] / res["one_launch"]["median"], 4)
            # the same eps, the same start: the first commands agree to float32 rounding
            res["first_commands_max_abs_diff"] = float((one.actions[0] - comp.actions[0]).abs().max()) if hidden > 64 else None
            out[f"gaussian_vs_composed_c2_{hidden}_{hidden}"] = dict(res, calls_per_region=n, unit="microseconds per env-step of the batch")
        except Exception:      # noqa: BLE001
            out[f"gaussian_vs_composed_c2_{hidden}_{hidden}"] = {"error": traceback.format_exc(limit=3)}
        torch.cuda.synchronize()
    print("RESULT " + json.dumps(out), flush=True)


# ---- driver ---------------------------------------------------------------------------------------------------------------------------------
def child(args, limit):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise RuntimeError(f"worker {args} ended with {p.returncode}: {p.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit with its library built (measurement 1)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="least seconds per timed region")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=("plain", "gaussian"), default=None)
    ap.add_argument("--tree", default=HERE)
    args = ap.parse_args()
    if args.worker == "plain":
        return worker_plain(os.path.abspath(args.tree), args.window)
    if args.worker == "gaussian":
        return worker_gaussian(args.window, args.batch)
    report = {"tool": "tools/measure_gaussian_head.py", "rounds": args.rounds, "window_seconds": args.window}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")
    if args.parent_tree:
        runs = {"parent": [], "child": []}
        for _ in range(args.rounds):      # a fresh process per build and round, one at a time
            for key, tree in (("parent", args.parent_tree), ("child", HERE)):
                runs[key].append(child(["--worker", "plain", "--tree", tree, "--window", str(args.window)], 600))
        plain = {}
        for name in PLAIN:
            med = {k: [r[name]["median"] for r in v if "median" in r[name]] for k, v in runs.items()}
            if not med["parent"] or not med["child"]:
                plain[name] = {"error": [r[name].get("error") for v in runs.values() for r in v]}
                continue
            p, c = float(np.median(med["parent"])), float(np.median(med["child"]))
            spread = (max(med["parent"]) - min(med["parent"])) / p
            plain[name] = dict(parent_us=med["parent"], child_us=med["child"], parent_median=round(p, 3), child_median=round(c, 3),
                               child_over_parent=round(c / p, 4), parent_spread=round(spread, 4), inside_parent_spread=bool(abs(c / p - 1) <= spread))
        report["plain"] = dict(plain, stamps={k: v[0]["library_stamp"] for k, v in runs.items()}, device=runs["child"][0]["device"],
                               unit="microseconds per env-step of the batch of 4096, median of 5 regions per process")
        print(json.dumps(report["plain"]), flush=True)
        save()
    else:
        report["plain"] = "not measured: no --parent-tree"
    report["gaussian"] = child(["--worker", "gaussian", "--window", str(args.window), "--batch", str(args.batch)], 900)
    print(json.dumps(report["gaussian"]), flush=True)
    save()


if __name__ == "__main__":
    main()
