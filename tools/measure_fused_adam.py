#!/usr/bin/env python3
"""Measurements of the fused optimiser step -> profiles/r16_fused_adam.json.

  1. Microseconds per optimiser step for two parameter sets -- the PPO example's 13 tensors (65-64-64-1 twice + ``log_std``, clip 0.5)
     and SAC's twin 66-256-256-1 critics with their targets -- on four paths, alternating in one process, medians of five regions of
     >= 0.3 s each:
       ``fused_adam``              ``FusedAdam.step`` (attached wrappers and targets: nothing else to do);
       ``torch_eager``             the parent's path: ``clip_grad_norm_`` (PPO), default ``Adam``, ``refresh()`` of the wrappers, the
                                   ``lerp_`` loop (SAC);
       ``torch_fused``             the same with ``Adam(fused=True)`` and ``_foreach_lerp_``;
       ``torch_capturable_graph``  ``clip_grad_norm_`` + ``Adam(capturable=True)`` (+ ``_foreach_lerp_``) in a hipGraph; ``refresh()``
                                   cannot be captured (it reads version counters on the host), so it runs OUTSIDE the graph after
                                   every replay -- with the version counters bumped by hand, since a replay does not bump them.
     Gradients are static tensors; every path owns its copy of the parameters.
  2. ``updates`` wall time of both examples (``fused_grad`` and ``fused_loss`` on) with ``fused_opt`` off / on, and of the PPO example
     with ``fused_opt`` on and ``graph_update`` off / on: fresh processes, alternating, ``--runs`` each (default 4).
  3. The pairs e_kernel / e_torch of tests/test_gpu_fused_adam.py's real-valued case and the tolerance factor they give.
  4. With ``--parent DIR`` (a built checkout of the parent commit): ``bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs`` of both
     trees, alternating; the dumped arrays must be bit-identical.

    python tools/measure_fused_adam.py [out.json] [--no-example] [--runs N] [--parent DIR]
"""
import copy
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
from pde_control_gym import FusedAdam, FusedMLP  # noqa: E402


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


def mlp(sizes, act):
    mods = []
    for i in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), act()]
    return torch.nn.Sequential(*mods[:-1]).cuda()


def build(kind):
    """(networks, extra parameters, target networks or None, clip, tau)"""
    torch.manual_seed(0)
    if kind == "ppo_13_tensors":
        return [mlp([65, 64, 64, 1], torch.nn.Tanh) for _ in range(2)], [torch.nn.Parameter(torch.full((1,), -0.7, device="cuda"))], None, 0.5, None
    nets = [mlp([66, 256, 256, 1], torch.nn.ReLU) for _ in range(2)]
    return nets, [], [copy.deepcopy(n).requires_grad_(False) for n in nets], None, 0.005


def micro(kind):
    paths = {}
    info = {}
    for path in ("fused_adam", "torch_eager", "torch_fused", "torch_capturable_graph"):
        nets, extra, targets, clip, tau = build(kind)
        params = [p for n in nets for p in n.parameters()] + extra
        wrappers = [FusedMLP(n) for n in nets]
        for p in params:
            p.grad = torch.randn_like(p) * 0.01
        tparams = [p for n in targets for p in n.parameters()] if targets else []
        lerp_from = params[:len(tparams)]
        info["tensors"], info["elements"] = len(params), sum(p.numel() for p in params)
        if path == "fused_adam":
            opt = FusedAdam(params, lr=3e-4, max_grad_norm=clip)
            for w in wrappers:
                opt.attach(w)
            if targets:
                opt.attach_target(lerp_from, tparams, tau)
            paths[path] = (lambda opt=opt, polyak=bool(targets): opt.step(polyak=polyak))
            continue
        kw = {"fused": True} if path == "torch_fused" else ({"capturable": True} if path == "torch_capturable_graph" else {})
        opt = torch.optim.Adam(params, lr=3e-4, **kw)

        def device_part(opt=opt, params=params, clip=clip, tparams=tparams, lerp_from=lerp_from, each=path == "torch_eager", tau=tau):
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(params, clip)
            opt.step()
            if tparams:
                with torch.no_grad():
                    if each:
                        for p, pt in zip(lerp_from, tparams):
                            pt.lerp_(p, tau)
                    else:
                        torch._foreach_lerp_(tparams, [p.detach() for p in lerp_from], tau)

        def refresh(wrappers=wrappers):
            for w in wrappers:
                w.refresh()

        if path != "torch_capturable_graph":
            paths[path] = (lambda device_part=device_part, refresh=refresh: (device_part(), refresh()))
            continue
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    device_part()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                device_part()

            def graphed(graph=graph, params=params, refresh=refresh):
                graph.replay()
                for p in params:
                    torch.autograd.graph.increment_version(p)
                refresh()
            paths[path] = graphed
        except Exception as e:      # noqa: BLE001  (reported, not hidden)
            info["graph_error"] = f"{type(e).__name__}: {e}"[:400]
            torch.cuda.synchronize()
    for fn in paths.values():      # warm-up
        for _ in range(5):
            fn()
    samples = {k: [] for k in paths}
    for _ in range(5):             # alternating
        for k, fn in paths.items():
            samples[k].append(region(fn))
    out = {k: {"median_us": statistics.median(v) * 1e6, "regions_us": [s * 1e6 for s in v]} for k, v in samples.items()}
    out.update(info)
    for k in paths:
        if k != "fused_adam":
            out[k + "_over_fused_adam"] = out[k]["median_us"] / out["fused_adam"]["median_us"]
    return out


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
    return {"argv": argv + ["<fused_opt>"], "updates_s": res, "median_off_s": statistics.median(res["off"]), "median_on_s": statistics.median(res["on"])}


def tolerance():
    from tests import test_gpu_fused_adam as T
    got = T.tolerance_pairs()
    rows = [{"tensor": k, "e_kernel": e_k, "e_torch": e_t} for k, e_k, e_t in got["pairs"]]
    counted = [r for r in rows if r["e_torch"] >= 2.0 ** -24]
    out = {"pairs": rows, "norms_kernel_float64": got["norms"], "pairs_below_2^-24": len(rows) - len(counted)}
    if counted:
        ratio = max(r["e_kernel"] / r["e_torch"] for r in counted)
        out["worst_ratio"], out["m"] = ratio, 2 ** max(0, math.ceil(math.log2(2.0 * ratio)))
    return out


def headline(parent, rounds=2):
    import numpy as np
    import tempfile
    times, dumps = {"this": [], "parent": []}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(rounds):
            for key, tree in (("this", ROOT), ("parent", parent)):
                dump = os.path.join(tmp, f"{key}{i}")
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", dump], cwd=tree,
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout.decode()[-2000:])
                times[key].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
                dumps[key] = dump
        names = sorted(os.listdir(dumps["this"]))
        same = names == sorted(os.listdir(dumps["parent"])) and bool(names) and all(
            np.load(os.path.join(dumps["this"], n)).tobytes() == np.load(os.path.join(dumps["parent"], n)).tobytes() for n in names)
    return {"results": times, "outputs_bit_identical": bool(same)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 4
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    args = [a for a in args if a not in (str(runs), parent)]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r16_fused_adam.json")
    doc = {"device": torch.cuda.get_device_name(0), "micro": {k: micro(k) for k in ("ppo_13_tensors", "sac_twin_critics_with_targets")}}
    doc["tolerance"] = tolerance()

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
    save()
    if "--no-example" not in sys.argv:
        doc["ppo_example_30x64x2048"] = example_updates("train_ppo_device.py", ["30", "2048", "64", "1", "1"], runs)
        save()
        doc["sac_example_30x32x1024"] = example_updates("train_sac_device.py", ["30", "1024", "64", "1", "1"], runs)
        save()
        doc["ppo_example_graph_update_30x64x2048"] = example_updates("train_ppo_device.py", ["30", "2048", "64", "1", "1", "1"], runs)
        save()
    if parent:
        doc["headline"] = headline(parent)
        save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
