"""What the one-launch GAE (pdegym_gae behind ``DeviceRolloutBuffer.compute``) costs against the torch loop it replaces, on ONE device,
medians of repeated regions.

    python tools/measure_gae.py [--window 0.3] [--parent-tree DIR] [--out profiles/<tag>_gae.json]

1. ``shapes``: in one process, for T x B = 64 x 2048 (examples/train_ppo_device.py) and 2048 x 4096 (SB3's default ``n_steps`` at the
   headline batch), ALTERNATING
     ``compute``     ``buffer.compute(values=...)``: the copy of the values into the buffer + the one launch (boot and statistics off);
     ``launch``      the launch alone (``HipBackend.gae`` on the same tensors);
     ``compute_stats``  the same with the episode statistics on (a second row of workgroups in the same launch);
     ``loop_eager``  the loop of the example before the buffer -- T iterations of ~8 elementwise torch launches over [B];
     ``loop_graph``  that loop captured in one hipGraph and replayed: its best case.
   The outputs of the loop and of the launch are compared bit for bit in the same run.  Beside the times: the algorithmic bytes of
   a call -- 4 (T+1) B values + (4 + 1 + 1) T B rewards and flags read + 8 T B advantages and returns written -- and the rate they
   give over the time of ``launch``.
2. ``example``: the ``updates`` wall time examples/train_ppo_device.py prints (critic, targets and the PPO epochs of 30 iterations),
   in this tree and in ``--parent-tree`` (a checkout of the parent commit with its library built), alternating, a fresh process each.
A region is N consecutive calls between two HIP events, N chosen so that it lasts at least ``--window`` seconds; five regions per
path.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import re
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, 2048), (2048, 4096))
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


def alternate(paths, seconds):
    """{name: fn} -> {name: microseconds per call}, the paths' regions alternating; every path gets its own N."""
    counts = {}
    for k, fn in paths.items():
        for _ in range(2):
            fn()
        counts[k] = max(3, int(np.ceil(seconds / (region(fn, 3) / 3))))
    times = {k: [] for k in paths}
    for _ in range(REGIONS):
        for k, fn in paths.items():
            times[k].append(region(fn, counts[k]) / counts[k] * 1e6)
    return {k: dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3), calls_per_region=counts[k])
            for k, v in times.items()}


def algorithmic_bytes(T, B):
    return 4 * (T + 1) * B + (4 + 1 + 1) * T * B + 8 * T * B


def measure_shape(T, B, seconds):
    import torch
    from pde_control_gym import DeviceRolloutBuffer
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T)
    rew = torch.randn(T, B, generator=g, device=dev)
    val = torch.randn(T + 1, B, generator=g, device=dev) * 2
    terminated = (torch.rand(T, B, generator=g, device=dev) < 0.01).to(torch.uint8)
    truncated = (torch.rand(T, B, generator=g, device=dev) < 0.01).to(torch.uint8)
    ro = types.SimpleNamespace(T=T, rewards=rew, terminated=terminated, truncated=truncated, obs=None, obs_seen=None, actions=None)
    gamma, lam = 0.99, 0.95
    buf = DeviceRolloutBuffer(ro, gamma, lam, episode_stats=False)
    buf_stats = DeviceRolloutBuffer(ro, gamma, lam, episode_stats=True)
    done = (terminated | truncated).float()      # (the example forms it once per rollout as well; not part of the loop)
    adv, ret = torch.zeros(T, B, device=dev), torch.zeros(T, B, device=dev)

    def loop():
        last = torch.zeros(B, device=dev)
        for t in reversed(range(T)):
            nonterm = 1.0 - done[t]
            delta = rew[t] + gamma * val[t + 1] * nonterm - val[t]
            last = delta + gamma * lam * nonterm * last
            adv[t] = last
        torch.add(adv, val[:T], out=ret)

    loop()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop()
    buf.compute(values=val)
    torch.cuda.synchronize()
    same = bool(torch.equal(adv.view(torch.int32), buf.advantages.view(torch.int32))
                and torch.equal(ret.view(torch.int32), buf.returns.view(torch.int32)))
    adv.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same_graph = bool(torch.equal(adv.view(torch.int32), buf.advantages.view(torch.int32)))
    paths = {"compute": lambda: buf.compute(values=val),
             "launch": lambda: buf.backend.gae(rew, buf.values, terminated, truncated, buf.advantages, buf.returns, gamma, lam),
             "compute_stats": lambda: buf_stats.compute(values=val), "loop_eager": loop, "loop_graph": graph.replay}
    res = alternate(paths, seconds)
    nbytes = algorithmic_bytes(T, B)
    rate = nbytes / (res["launch"]["median"] * 1e-6)
    loop_spread = max((res[k]["max"] - res[k]["min"]) / res[k]["median"] for k in ("loop_eager", "loop_graph"))
    best_loop = min(res["loop_eager"]["median"], res["loop_graph"]["median"])
    return dict(res, T=T, B=B, unit="microseconds per call", bitwise_equal_to_loop=same, bitwise_equal_to_graphed_loop=same_graph,
                algorithmic_bytes=nbytes, launch_bytes_per_second=round(rate, 0), launch_fraction_of_hbm_peak_8e12=round(rate / 8e12, 4),
                waves=(B + 63) // 64, steps_per_microsecond_per_wave=round(T / res["launch"]["median"], 2),
                loop_over_compute=round(best_loop / res["compute"]["median"], 1), loop_spread=round(loop_spread, 4),
                not_slower_than_either_loop=bool(res["compute"]["median"] <= best_loop * (1 + loop_spread)))


def example_updates(tree, limit=900):
    """The seconds after ``updates`` in the last line examples/train_ppo_device.py prints, run in ``tree`` as a fresh process."""
    p = subprocess.run([sys.executable, os.path.join(tree, "examples", "train_ppo_device.py")], capture_output=True, text=True, timeout=limit,
                       cwd=tree)
    m = re.search(r"rollouts ([0-9.]+) s .*updates ([0-9.]+) s", p.stdout)
    if p.returncode != 0 or not m:
        raise RuntimeError(f"the example in {tree} ended with {p.returncode}: {p.stderr[-1500:]}")
    return {"rollouts_s": float(m.group(1)), "updates_s": float(m.group(2))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--window", type=float, default=0.3, help="least seconds per timed region")
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit with its library built (measurement 2)")
    ap.add_argument("--rounds", type=int, default=2, help="runs of the example per tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/measure_gae.py needs a GPU: there is no CPU path")
    report = {"tool": "tools/measure_gae.py", "window_seconds": args.window, "regions": REGIONS, "device": torch.cuda.get_device_name(0),
              "shapes": []}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")
    for T, B in SHAPES:
        report["shapes"].append(measure_shape(T, B, args.window))
        print(json.dumps(report["shapes"][-1]), flush=True)
        save()
    if args.parent_tree:
        runs = {"parent": [], "child": []}
        for _ in range(args.rounds):
            for key, tree in (("parent", os.path.abspath(args.parent_tree)), ("child", HERE)):
                runs[key].append(example_updates(tree))
        report["example"] = dict(runs, parent_updates_median=float(np.median([r["updates_s"] for r in runs["parent"]])),
                                 child_updates_median=float(np.median([r["updates_s"] for r in runs["child"]])),
                                 what="examples/train_ppo_device.py, 30 iterations x 64 steps x 2048 envs: seconds in critic + targets + PPO epochs")
    else:
        report["example"] = "not measured: no --parent-tree"
    print(json.dumps(report["example"]), flush=True)
    save()


if __name__ == "__main__":
    main()
