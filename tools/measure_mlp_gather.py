#!/usr/bin/env python3
"""Measurements of the rows-by-index call form -> profiles/r21_mlp_gather.json.

  1. Microseconds per call for the networks of a SAC update on a replay storage of M = 262 144 transitions -- critics 66-256-256-1 and
     202-256-256-1 (the parabolic plant's row), actors of the same rows with two outputs -- at N = 2048 and 32 768, the index path
     against the parent's (``storage[index]`` copies, then the calls on the copies), alternating in one process, medians of five
     regions of >= 0.3 s each; every parent piece includes the gathers it needs:
       ``critic_step``    both critics, forward + backward with parameter gradients: ``with_grad(obs, act, index=mb, tail_indexed=True)``
                          against ``obs[mb]``, ``act[mb]`` + ``with_grad(o, a)``; the loss is ``q.sum()``, its backward included;
       ``actor_critics``  both critics of the actor step on a fresh action that requires grad: ``with_grad(obs, a, index=mb,
                          params=False)`` against ``obs[mb]`` + ``with_grad(o, a, params=False)``, ``autograd.grad`` to ``a``;
       ``actor_net``      the actor's forward + backward: ``with_grad(obs, index=mb)`` against ``obs[mb]`` + ``with_grad(o)``;
       ``update``         the three in the order of the example, the parent gathering ``obs[mb]`` and ``act[mb]`` ONCE for all of them.
  2. ``updates`` wall time of ``examples/train_sac_device.py 30 1024 256`` with all switches, ``replay`` off and on, and of
     ``examples/train_ppo_device.py 30 2048 64`` with ``graph_update``, ``gather`` off and on: fresh processes, alternating, ``--runs``
     each (default 3), every run listed.

    python tools/measure_mlp_gather.py [out.json] [--no-example] [--runs N]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_control_gym import FusedMLP  # noqa: E402

ROWS = {"66-256-256-1": 65, "202-256-256-1": 201}      # critic -> observation width D (one action column)
BATCHES = (2048, 32768)
POOL = 262144


def region(fn, min_s=0.3):
    """Seconds per call over one region of at least ``min_s``."""
    n = 8
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / n
        n *= 2


def mlp(sizes):
    mods = []
    for i in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.ReLU()]
    return torch.nn.Sequential(*mods[:-1]).cuda()


def alternate(paths):
    for fn in paths.values():      # warm-up
        for _ in range(5):
            fn()
    samples = {k: [] for k in paths}
    for _ in range(5):
        for k, fn in paths.items():
            samples[k].append(region(fn))
    out = {k: {"median_us": statistics.median(v) * 1e6, "regions_us": [s * 1e6 for s in v]} for k, v in samples.items()}
    out["parent_over_new"] = out["parent"]["median_us"] / out["new"]["median_us"]
    return out


def micro(D, n):
    torch.manual_seed(0)
    nets = [mlp((D + 1, 256, 256, 1)), mlp((D + 1, 256, 256, 1)), mlp((D, 256, 256, 2))]
    q1, q2, pi = (FusedMLP(net) for net in nets)
    obs, act = torch.randn(POOL, D, device="cuda"), torch.rand(POOL, 1, device="cuda") * 2 - 1
    mb = torch.randint(0, POOL, (n,), device="cuda")
    fresh = torch.rand(n, 1, device="cuda") * 2 - 1
    params = [p for net in nets for p in net.parameters()]

    def zero():
        for p in params:
            p.grad = None

    def critic_new():
        zero()
        (q1.with_grad(obs, act, index=mb, tail_indexed=True) + q2.with_grad(obs, act, index=mb, tail_indexed=True)).sum().backward()

    def critic_parent(o=None, a=None):
        zero()
        o, a = (obs[mb], act[mb]) if o is None else (o, a)
        (q1.with_grad(o, a) + q2.with_grad(o, a)).sum().backward()

    def critics_new():
        a = fresh.detach().requires_grad_(True)
        loss = (q1.with_grad(obs, a, index=mb, params=False) + q2.with_grad(obs, a, index=mb, params=False)).sum()
        return torch.autograd.grad(loss, a)[0]

    def critics_parent(o=None):
        o = obs[mb] if o is None else o
        a = fresh.detach().requires_grad_(True)
        loss = (q1.with_grad(o, a, params=False) + q2.with_grad(o, a, params=False)).sum()
        return torch.autograd.grad(loss, a)[0]

    def actor_new():
        zero()
        pi.with_grad(obs, index=mb).sum().backward()

    def actor_parent(o=None):
        zero()
        pi.with_grad(obs[mb] if o is None else o).sum().backward()

    def update_new():
        critic_new()
        actor_new()
        critics_new()

    def update_parent():
        o, a = obs[mb], act[mb]
        critic_parent(o, a)
        actor_parent(o)
        critics_parent(o)

    critic_new()
    g_new = [p.grad.clone() for p in params if p.grad is not None]
    critic_parent()
    assert all(torch.equal(a, b) for a, b in zip(g_new, [p.grad for p in params if p.grad is not None])), "the critic steps disagree in bits"
    assert torch.equal(critics_new(), critics_parent()), "the actor step's critic passes disagree in bits"
    return {"critic_step": alternate({"new": critic_new, "parent": critic_parent}),
            "actor_critics": alternate({"new": critics_new, "parent": critics_parent}),
            "actor_net": alternate({"new": actor_new, "parent": actor_parent}),
            "update": alternate({"new": update_new, "parent": update_parent})}


def example_updates(script, argv, runs):
    res = {"off": [], "on": []}
    for _ in range(runs):
        for key, flag in (("off", "0"), ("on", "1")):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)] + argv + [flag], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=600)
            m = re.search(r"updates ([0-9.]+) s", r.stdout.decode())
            if r.returncode != 0 or not m:
                raise RuntimeError(r.stdout.decode()[-2000:])
            res[key].append(float(m.group(1)))
    return {"argv": argv + ["<switch>"], "updates_s": res, "median_off_s": statistics.median(res["off"]),
            "median_on_s": statistics.median(res["on"]), "spread_off_s": [min(res["off"]), max(res["off"])],
            "spread_on_s": [min(res["on"]), max(res["on"])]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r21_mlp_gather.json"))
    ap.add_argument("--no-example", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    opt = ap.parse_args()
    runs, out_path = opt.runs, opt.out
    doc = {"device": torch.cuda.get_device_name(0), "storage_rows": POOL, "micro": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
    for name, D in ROWS.items():
        for n in BATCHES:
            doc["micro"][f"{name}@N={n}"] = micro(D, n)
            save()
    if not opt.no_example:
        doc["sac_example_30x32x1024_hidden256_replay"] = example_updates("train_sac_device.py", ["30", "1024", "256", "1", "1", "1", "1", "0"], runs)
        save()
        doc["ppo_example_30x64x2048_hidden64_graph_update_gather"] = example_updates("train_ppo_device.py", ["30", "2048", "64", "1", "1", "1", "1", "0"], runs)
        save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
