#!/usr/bin/env python3
"""Measurements of the SAC loss heads -> profiles/r14_sac_loss.json.

  1. ``head.sample`` x 2 + ``head.critic`` + ``head.actor`` with their ``backward()`` against the eager torch lines they replace in
     examples/train_sac_device.py (the gathers of rewards and terminations, ``sample()`` twice, two ``cat``, two ``min``, the target,
     the three losses and their three ``backward()``), the networks excluded: the actor's rows ``raw`` and the critics' outputs are
     leaf tensors, so both paths end in the accumulation of their ``.grad``.  The same eager lines captured in a hipGraph are the
     third path (launch count against fusion).  Paths alternating in one process, medians of five regions of >= 0.3 s each, at the
     example's batch (N = 2048, A = 1) and at N = 32 768.
  2. ``updates`` wall time of examples/train_sac_device.py (30 x 32 x 1024, ``fused_grad`` on) with ``fused_loss`` off / on: fresh
     processes, alternating, four runs each.
  3. The errors e_kernel / e_torch of tests/test_gpu_sac_loss.py's real-valued cases against the float64 restatement, and the
     tolerance factor m they give (the worst ratio among pairs with e_torch >= 2^-24, doubled, rounded up to a power of two).

    python tools/measure_sac_loss.py [out.json] [--no-example]
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
from pde_control_gym import SACLoss  # noqa: E402

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
GAMMA, TARGET_ENTROPY = 0.99, -1.0


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


def sample_lines(raw):
    """``sample()`` of examples/train_sac_device.py on the rows [mu, log_std]."""
    mean, ls = raw[:, :raw.shape[1] // 2], raw[:, raw.shape[1] // 2:]
    ls = ls.clamp(LOG_STD_MIN, LOG_STD_MAX)
    z = mean + ls.exp() * torch.randn_like(mean)
    a = torch.tanh(z)
    logp = (-0.5 * ((z - mean) / ls.exp()) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(-1) - torch.log(1 - a * a + 1e-6).sum(-1)
    return a, logp


def micro(N, M, D=65):
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)      # noqa: E731
    raw, raw2 = (0.5 * rnd(N, 2)).requires_grad_(), 0.5 * rnd(N, 2)
    q1, q2, q1_pi, q2_pi = (rnd(N, 1).requires_grad_() for _ in range(4))
    q1n, q2n = rnd(N, 1), rnd(N, 1)
    o, o2 = rnd(N, D), rnd(N, D)
    rew, term = rnd(M, 1), (torch.rand(M, 1, device="cuda", generator=g) < 0.1).float()
    mb = torch.randint(0, M, (N,), device="cuda", generator=g)
    log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
    head = SACLoss(GAMMA, TARGET_ENTROPY, (LOG_STD_MIN, LOG_STD_MAX))
    leaves = (raw, q1, q2, q1_pi, q2_pi, log_alpha)

    def fused():
        for p in leaves:
            p.grad = None
        eps2, eps = torch.randn(2, N, 1, device="cuda")
        with torch.no_grad():
            _, logp2 = head.sample(raw2, eps2, obs=o2)
        head.critic(q1, q2, q1n, q2n, logp2, rew, term, log_alpha, index=mb).backward()
        _, logp = head.sample(raw, eps, obs=o)
        head.actor(q1_pi, q2_pi, logp, log_alpha).backward()

    def eager_lines():
        r, d = rew[mb], term[mb]
        alpha = log_alpha.exp().detach()
        with torch.no_grad():
            a2, logp2 = sample_lines(raw2)
            torch.cat([o2, a2], 1)
            q_next = torch.min(q1n, q2n) - alpha * logp2.unsqueeze(1)
            target = r + GAMMA * (1.0 - d) * q_next
        q_loss = (q1 - target).pow(2).mean() + (q2 - target).pow(2).mean()
        q_loss.backward()
        a_pi, logp = sample_lines(raw)
        torch.cat([o, a_pi], 1)
        actor_loss = (alpha * logp.unsqueeze(1) - torch.min(q1_pi, q2_pi)).mean()
        actor_loss.backward()
        alpha_loss = -(log_alpha * (logp.detach() + TARGET_ENTROPY).mean())
        alpha_loss.backward()

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
            r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_sac_device.py"), "30", "1024", "64", "1", flag],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            m = re.search(r"updates ([0-9.]+) s", r.stdout.decode())
            if r.returncode != 0 or not m:
                raise RuntimeError(r.stdout.decode()[-2000:])
            res[key].append(float(m.group(1)))
    return {"fused_grad": 1, "updates_s": res, "median_off_s": statistics.median(res["off"]), "median_on_s": statistics.median(res["on"])}


def tolerance():
    from tests import test_gpu_sac_loss as T
    rows = []
    for n, A in T.REAL_CASES:
        for name, e_k, e_t in T.real_case_errors(n, A):
            rows.append({"case": f"n{n}_A{A}", "name": name, "e_kernel": e_k, "e_torch": e_t})
    for name, e_k, e_t in T.end_to_end_errors():
        rows.append({"case": "end_to_end_65-64-64_n1000", "name": name, "e_kernel": e_k, "e_torch": e_t})
    counted = [r for r in rows if r["e_torch"] >= 2.0 ** -24]
    worst = max(counted, key=lambda r: r["e_kernel"] / r["e_torch"])
    ratio = worst["e_kernel"] / worst["e_torch"]
    m = 2 ** max(0, math.ceil(math.log2(2.0 * ratio)))
    below = [r for r in rows if r["e_torch"] < 2.0 ** -24]
    return {"pairs": rows, "worst_ratio": ratio, "worst_pair": [worst["case"], worst["name"]], "m": m,
            "pairs_below_2^-24": len(below), "largest_e_kernel_below_2^-24": max((r["e_kernel"] for r in below), default=0.0)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r14_sac_loss.json")
    doc = {"device": torch.cuda.get_device_name(0), "micro": {}}
    for N, M in ((2048, 524288), (32768, 524288)):
        doc["micro"][f"N{N}_M{M}_A1"] = micro(N, M)
    doc["tolerance"] = tolerance()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:                  # (kept if the example runs fail)
        json.dump(doc, f, indent=1)
    if "--no-example" not in sys.argv:
        doc["sac_example_30x32x1024"] = example_updates()
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "pairs"} if k == "tolerance" else v) for k, v in doc.items()}, indent=1))


if __name__ == "__main__":
    main()
