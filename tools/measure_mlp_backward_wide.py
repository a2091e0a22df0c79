#!/usr/bin/env python3
"""Measurements of the wide fused MLP backward pass -> profiles/r15_mlp_backward_wide.json.

  1. ``FusedMLP.with_grad`` forward + ``backward()`` of a sum-of-squares loss against torch float32 autograd on the same module
     (eager) for SB3's SAC shapes -- the 66-256-256-1 ReLU critic at B = 2048 (the SAC example's batch) and 32 768, the 65-256-256-2
     ReLU actor body at B = 2048 -- the two paths alternating in one process, medians of five regions of >= 0.3 s each; the backward
     launches alone as well.
  2. ``updates`` wall time of examples/train_sac_device.py (30 x 32 x 1024, 256 units) with ``fused_grad`` off and on: fresh
     processes, alternating, four runs each.
  3. The errors e_kernel / e_torch of tests/test_gpu_mlp_backward_wide.py's real networks against float64 autograd, and the
     tolerance factor they give (worst ratio over tensors with e_torch >= 2**-24, doubled, rounded up to a power of two).

    python tools/measure_mlp_backward_wide.py [out.json] [--no-example]
    python tools/measure_mlp_backward_wide.py --launches B [count]     # only the backward launches of the critic: for a kernel trace
"""
import json
import math
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from measure_mlp_backward import region  # noqa: E402
from pdecontrolgym_amd.policy import FusedMLP  # noqa: E402

CRITIC, ACTOR = (66, 256, 256, 1), (65, 256, 256, 2)


def mlp(sizes):
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def paths_of(sizes, B):
    torch.manual_seed(0)
    net = mlp(sizes).cuda()
    pol = FusedMLP(net)
    assert not pol.fits_backward() and pol.fits_backward_wide()
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
        pol.backend.mlp_backward_wide(desc, x, dy, weights, dw, db)

    return {"with_grad": fused, "torch_eager": eager, "backward_launches": backward_only}


def micro(sizes, B):
    paths = paths_of(sizes, B)
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
            r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_sac_device.py"), "30", "1024", "256", flag],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            m = re.search(r"updates ([0-9.]+) s", r.stdout.decode())
            if r.returncode != 0 or not m:
                raise RuntimeError(r.stdout.decode()[-2000:])
            res[key].append(float(m.group(1)))
    return {"updates_s": res, "median_off_s": statistics.median(res["off"]), "median_on_s": statistics.median(res["on"])}


def tolerance():
    from tests import mlp_backward_wide_exact as W
    from tests import test_gpu_mlp_backward_wide as T
    rows = []
    for sizes, act, B in W.REAL_CASES:
        for name, e_k, e_t in T.real_case_errors(sizes, act, B):
            rows.append({"net": "-".join(map(str, sizes)) + "-" + act, "B": B, "tensor": name, "e_kernel": e_k, "e_torch": e_t})
    counted = [r for r in rows if r["e_torch"] >= 2.0 ** -24]
    worst = max(counted, key=lambda r: r["e_kernel"] / r["e_torch"])
    ratio = worst["e_kernel"] / worst["e_torch"]
    return rows, {"worst_ratio": ratio, "worst": worst, "pairs": len(rows), "pairs_with_e_torch_at_least_2^-24": len(counted),
                  "m": 2.0 ** math.ceil(math.log2(2.0 * ratio))}


def main():
    if "--launches" in sys.argv:
        at = sys.argv.index("--launches")
        B, count = int(sys.argv[at + 1]), int(sys.argv[at + 2]) if len(sys.argv) > at + 2 else 200
        fn = paths_of(CRITIC, B)["backward_launches"]
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r15_mlp_backward_wide.json")
    doc = {"device": torch.cuda.get_device_name(0), "micro": {}}
    for sizes, B in ((CRITIC, 2048), (CRITIC, 32768), (ACTOR, 2048)):
        doc["micro"][f"{'-'.join(map(str, sizes))}-relu-B{B}"] = micro(sizes, B)
    doc["tolerance"], doc["tolerance_factor"] = tolerance()
    if "--no-example" not in sys.argv:
        doc["sac_example_30x32x1024_hidden256"] = example_updates()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "tolerance"}, indent=1))


if __name__ == "__main__":
    main()
