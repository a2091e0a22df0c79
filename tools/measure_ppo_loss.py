#!/usr/bin/env python3
"""Measurements of the PPO loss head -> profiles/r13_ppo_loss.json.

  1. ``head(...)`` + ``result.backward()`` against the eager torch lines it replaces in examples/train_ppo_device.py (the gathers, the
     log-probability, ratio, clamp, min, the means and ``loss.backward()``), the networks excluded: ``mean`` and ``values`` are leaf
     tensors, so both paths end in the accumulation of their ``.grad``.  The same eager lines captured in a hipGraph are the third
     path (launch count against fusion).  Paths alternating in one process, medians of five regions of >= 0.3 s each, at the example's
     minibatch (N = 32 768 of M = 131 072 rows, A = 1) and at N = 2048.
  2. ``updates`` wall time of examples/train_ppo_device.py (30 x 64 x 2048) with ``fused_grad`` on and ``fused_loss`` off / on: fresh
     processes, alternating, four runs each.
  3. The errors e_kernel / e_torch of tests/test_gpu_ppo_loss.py's real-valued cases against the float64 restatement, and the
     tolerance factor m they give (the worst ratio among pairs with e_torch >= 2^-24, doubled, rounded up to a power of two).

    python tools/measure_ppo_loss.py [out.json] [--no-example]
"""
import json
import math
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_control_gym import PPOLoss  # noqa: E402

CLIP = 0.2


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


def micro(N, M):
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)      # noqa: E731
    mean, values = rnd(N, 1).requires_grad_(), rnd(N, 1).requires_grad_()
    log_std = torch.full((1,), -0.7, device="cuda", requires_grad=True)
    a_f, adv_f, ret_f = rnd(M), rnd(M), rnd(M)
    mb = torch.randperm(M, device="cuda", generator=g)[:N]
    with torch.no_grad():
        lp_f = torch.zeros(M, device="cuda")
        lp_f[mb] = -0.5 * ((a_f[mb] - mean[:, 0]) / log_std.exp()) ** 2 - log_std - 0.3 * rnd(N)
    adv_n = (adv_f - adv_f.mean()) / (adv_f.std() + 1e-8)
    head = PPOLoss(clip_range=CLIP, ent_coef=1e-3, vf_coef=0.25, normalize_advantage=True)
    leaves = (mean, values, log_std)

    def fused():
        for p in leaves:
            p.grad = None
        head(mean, log_std, values, a_f, lp_f, adv_f, ret_f, index=mb).backward()

    def eager_lines():
        m = mean.squeeze(-1)
        logp = -0.5 * ((a_f[mb] - m) / log_std.exp()) ** 2 - log_std
        ratio = (logp - lp_f[mb]).exp()
        pg = -torch.min(ratio * adv_n[mb], ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n[mb]).mean()
        vloss = 0.5 * (values.squeeze(-1) - ret_f[mb]).pow(2).mean()
        loss = pg + 0.5 * vloss - 1e-3 * log_std.sum()
        loss.backward()

    def eager():
        for p in leaves:
            p.grad = None
        eager_lines()

    paths = {"head": fused, "torch_eager": eager}
    graph_error = None
    try:      # the eager lines as one hipGraph: the gradients are accumulated into static tensors, zeroed inside the graph
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                for p in leaves:
                    p.grad = None
                eager_lines()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        for p in leaves:
            p.grad = None
        with torch.cuda.graph(graph):
            eager_lines()
        static = [p.grad for p in leaves]

        def graphed():
            for s in static:
                s.zero_()
            graph.replay()
        graphed()
        torch.cuda.synchronize()
        paths["torch_lines_in_a_graph"] = graphed
    except Exception as e:      # noqa: BLE001  (reported, not hidden: the JSON says why the third path is missing)
        graph_error = f"{type(e).__name__}: {e}"[:400]
        torch.cuda.synchronize()
    for fn in paths.values():      # warm-up
        for _ in range(5):
            fn()
    samples = {k: [] for k in paths}
    for _ in range(5):             # alternating
        for k, fn in paths.items():
            samples[k].append(region(fn))
    out = {k: {"median_us": statistics.median(v) * 1e6, "regions_us": [s * 1e6 for s in v]} for k, v in samples.items()}
    out["eager_over_head"] = out["torch_eager"]["median_us"] / out["head"]["median_us"]
    if graph_error:
        out["graph_error"] = graph_error
    return out


def example_updates(runs=4):
    res = {"off": [], "on": []}
    for _ in range(runs):
        for key, flag in (("off", "0"), ("on", "1")):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ppo_device.py"), "30", "2048", "64", "1", flag],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            m = re.search(r"updates ([0-9.]+) s", r.stdout.decode())
            if r.returncode != 0 or not m:
                raise RuntimeError(r.stdout.decode()[-2000:])
            res[key].append(float(m.group(1)))
    return {"fused_grad": 1, "updates_s": res, "median_off_s": statistics.median(res["off"]), "median_on_s": statistics.median(res["on"])}


def tolerance():
    from tests import test_gpu_ppo_loss as T
    rows = []
    for n, A in T.REAL_CASES:
        for normalize in (False, True):
            for name, e_k, e_t in T.real_case_errors(n, A, normalize):
                rows.append({"case": f"n{n}_A{A}_{'norm' if normalize else 'raw'}", "name": name, "e_kernel": e_k, "e_torch": e_t})
    for name, e_k, e_t in T.end_to_end_errors():
        rows.append({"case": "end_to_end_65-64-64-1_n1000", "name": name, "e_kernel": e_k, "e_torch": e_t})
    counted = [r for r in rows if r["e_torch"] >= 2.0 ** -24]
    worst = max(counted, key=lambda r: r["e_kernel"] / r["e_torch"])
    ratio = worst["e_kernel"] / worst["e_torch"]
    m = 2 ** max(0, math.ceil(math.log2(2.0 * ratio)))
    below = [r for r in rows if r["e_torch"] < 2.0 ** -24]
    return {"pairs": rows, "worst_ratio": ratio, "worst_pair": [worst["case"], worst["name"]], "m": m,
            "pairs_below_2^-24": len(below), "largest_e_kernel_below_2^-24": max((r["e_kernel"] for r in below), default=0.0)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r13_ppo_loss.json")
    doc = {"device": torch.cuda.get_device_name(0), "micro": {}}
    for N, M in ((32768, 131072), (2048, 8192)):
        doc["micro"][f"N{N}_M{M}_A1"] = micro(N, M)
    doc["tolerance"] = tolerance()
    if "--no-example" not in sys.argv:
        doc["ppo_example_30x64x2048"] = example_updates()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "pairs"} if k == "tolerance" else v) for k, v in doc.items()}, indent=1))


if __name__ == "__main__":
    main()
