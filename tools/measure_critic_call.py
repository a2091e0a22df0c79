#!/usr/bin/env python3
"""Measurements of the critic(obs, action) call form -> profiles/r18_critic_call.json.

  1. Microseconds per call for three ReLU critics -- 66-64-64-1, 66-256-256-1 and 202-256-256-1 (the parabolic plant's row) -- at
     N = 2048 and 32 768, the new path against the parent's, alternating in one process, medians of five regions of >= 0.3 s each:
       ``critic_step``     forward + backward with parameter gradients: ``with_grad(obs, act)`` against ``torch.cat`` +
                           ``with_grad(block)``; the loss is ``q.sum()``, its backward included on both sides;
       ``actor_pass``      both critics of the actor step, the action requiring grad: ``with_grad(obs, a, params=False)`` twice and
                           ``autograd.grad`` to ``a`` (two [N, 1] gradients added) against ``with_grad(block)`` twice on a block that
                           requires grad (the full backward, two [N, D + 1] gradients added, the action column sliced);
       ``actor_launches``  the backend calls of one critic's backward alone, no autograd and no allocation: ``mlp_backward_cat``
                           with ``params=False`` and ``dx2`` only against ``mlp_backward`` / ``mlp_backward_wide`` with the full dx.
  2. ``updates`` wall time of ``examples/train_sac_device.py 30 1024 <hidden>`` with hidden = 64 and 256: the three switches against
     four, fresh processes, alternating, ``--runs`` each (default 4), every run listed.
  3. With ``--parent DIR`` (a built checkout of the parent commit): ``bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs`` of both
     trees, alternating; the dumped arrays must be bit-identical (the headline runs none of this code).

    python tools/measure_critic_call.py [out.json] [--no-example] [--runs N] [--parent DIR]
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
from pde_control_gym import FusedMLP  # noqa: E402

NETS = {"66-64-64-1": (66, 64, 64, 1), "66-256-256-1": (66, 256, 256, 1), "202-256-256-1": (202, 256, 256, 1)}
BATCHES = (2048, 32768)


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


def micro(sizes, n):
    torch.manual_seed(0)
    D = sizes[0] - 1
    nets = [mlp(sizes), mlp(sizes)]
    q = [FusedMLP(net) for net in nets]
    obs, act = torch.randn(n, D, device="cuda"), torch.rand(n, 1, device="cuda") * 2 - 1
    params = [p for net in nets for p in net.parameters()]
    out = {}

    def zero():
        for p in params:
            p.grad = None

    def critic_new():
        zero()
        q[0].with_grad(obs, act).sum().backward()

    def critic_parent():
        zero()
        q[0].with_grad(torch.cat([obs, act], 1)).sum().backward()
    out["critic_step"] = alternate({"new": critic_new, "parent": critic_parent})

    def actor_new():
        a = act.detach().requires_grad_(True)
        loss = (q[0].with_grad(obs, a, params=False) + q[1].with_grad(obs, a, params=False)).sum()
        return torch.autograd.grad(loss, a)[0]

    def actor_parent():
        zero()
        block = torch.cat([obs, act], 1).requires_grad_(True)
        (q[0].with_grad(block) + q[1].with_grad(block)).sum().backward()
        return block.grad[:, D:]
    assert torch.equal(actor_new(), actor_parent()), "the two actor passes disagree in bits"
    out["actor_pass"] = alternate({"new": actor_new, "parent": actor_parent})

    pol, bk = q[0], q[0].backend
    desc = pol._net(None, False, plain=True)
    weights = [w.detach() for w, _, _ in pol.layers]
    dw, db = [torch.empty_like(w) for w in weights], [torch.empty_like(b.detach()) for _, b, _ in pol.layers]
    block, dy = torch.cat([obs, act], 1), torch.ones(n, 1, device="cuda")
    dx, dx2 = torch.empty_like(block), torch.empty_like(act)
    wide = not pol.fits_backward()
    old = bk.mlp_backward_wide if wide else bk.mlp_backward
    out["actor_launches"] = alternate({"new": lambda: bk.mlp_backward_cat(desc, obs, act, dy, weights, None, None, None, dx2, params=False, wide=wide),
                                       "parent": lambda: old(desc, block, dy, weights, dw, db, dx)})
    return out


def example_updates(hidden, runs):
    res = {"three_switches": [], "four_switches": []}
    for _ in range(runs):
        for key, flag in (("three_switches", "0"), ("four_switches", "1")):
            argv = ["30", "1024", str(hidden), "1", "1", "1", flag]
            r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_sac_device.py")] + argv, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=600)
            m = re.search(r"updates ([0-9.]+) s", r.stdout.decode())
            if r.returncode != 0 or not m:
                raise RuntimeError(r.stdout.decode()[-2000:])
            res[key].append(float(m.group(1)))
    return {"argv": ["30", "1024", str(hidden), "1", "1", "1", "<fused_critic>"], "updates_s": res,
            "median_three_s": statistics.median(res["three_switches"]), "median_four_s": statistics.median(res["four_switches"]),
            "spread_three_s": [min(res["three_switches"]), max(res["three_switches"])],
            "spread_four_s": [min(res["four_switches"]), max(res["four_switches"])]}


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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r18_critic_call.json")
    doc = {"device": torch.cuda.get_device_name(0), "micro": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
    for name, sizes in NETS.items():
        for n in BATCHES:
            doc["micro"][f"{name}@N={n}"] = micro(sizes, n)
            save()
    if "--no-example" not in sys.argv:
        for hidden in (64, 256):
            doc[f"sac_example_30x32x1024_hidden{hidden}"] = example_updates(hidden, runs)
            save()
    if parent:
        doc["headline"] = headline(parent)
        save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
