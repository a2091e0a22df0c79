#!/usr/bin/env python3
"""Measurements of the fused MLP backward pass -> profiles/r12_mlp_backward.json.

  1. ``FusedMLP.with_grad`` forward + ``backward()`` of a sum-of-squares loss against torch autograd on the same module (eager), the
     two paths alternating in one process, medians of five regions of >= 0.3 s each; the backward launches alone as well.
  2. ``updates`` wall time of examples/train_ppo_device.py (30 x 64 x 2048) with ``fused_grad`` off and on: fresh processes,
     alternating, four runs each.
  3. The errors e_kernel / e_torch of tests/test_gpu_mlp_backward.py's real tanh networks against float64 autograd.

    python tools/measure_mlp_backward.py [out.json] [--no-example]
"""
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
from pdecontrolgym_amd.policy import FusedMLP  # noqa: E402


def mlp(sizes):
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


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


def micro(sizes, B):
    torch.manual_seed(0)
    net = mlp(sizes).cuda()
    pol = FusedMLP(net)
    x = torch.randn(B, sizes[0], device="cuda")

    def fused():
        net.zero_grad(set_to_none=True)
        (pol.with_grad(x) ** 2).sum().backward()

    def eager():
        net.zero_grad(set_to_none=True)
        (net(x) ** 2).sum().backward()

    weights = [w.detach() for w, _, _ in pol.layers]
    dw = [torch.empty_like(w) for w in weights]
    db = [torch.empty_like(b.detach()) for _, b, _ in pol.layers]
    dy = torch.randn(B, sizes[-1], device="cuda")
    desc = pol._net(None, False, plain=True)

    def backward_only():
        pol.backend.mlp_backward(desc, x, dy, weights, dw, db)

    paths = {"with_grad": fused, "torch_eager": eager, "backward_launches": backward_only}
    for fn in paths.values():      # warm-up
        for _ in range(5):
            fn()
    samples = {k: [] for k in paths}
    for _ in range(5):             # alternating
        for k, fn in paths.items():
            samples[k].append(region(fn))
    out = {k: {"median_us": statistics.median(v) * 1e6, "regions_us": [s * 1e6 for s in v]} for k, v in samples.items()}
    out["speedup_with_grad_over_eager"] = out["torch_eager"]["median_us"] / out["with_grad"]["median_us"]
    return out


def example_updates(runs=4):
    res = {"off": [], "on": []}
    for _ in range(runs):
        for key, flag in (("off", "0"), ("on", "1")):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ppo_device.py"), "30", "2048", "64", flag],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            m = re.search(r"updates ([0-9.]+) s", r.stdout.decode())
            if r.returncode != 0 or not m:
                raise RuntimeError(r.stdout.decode()[-2000:])
            res[key].append(float(m.group(1)))
    return {"updates_s": res, "median_off_s": statistics.median(res["off"]), "median_on_s": statistics.median(res["on"])}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r12_mlp_backward.json")
    doc = {"device": torch.cuda.get_device_name(0), "micro": {}, "tolerance": []}
    for sizes in ((65, 64, 64, 1), (257, 64, 64, 1)):
        for B in (32768, 2048):
            doc["micro"][f"{'-'.join(map(str, sizes))}-B{B}"] = micro(sizes, B)
    from tests import mlp_backward_exact as R
    from tests import test_gpu_mlp_backward as T
    for sizes, B in R.REAL_CASES:
        for name, e_k, e_t in T.real_case_errors(sizes, B):
            doc["tolerance"].append({"net": "-".join(map(str, sizes)), "B": B, "tensor": name, "e_kernel": e_k, "e_torch": e_t})
    if "--no-example" not in sys.argv:
        doc["ppo_example_30x64x2048"] = example_updates()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "tolerance"}, indent=1))


if __name__ == "__main__":
    main()
