#!/usr/bin/env python3
"""Generate tests/golden/traffic_backstep.npz: the backstepping baseline of the reference's traffic notebook
(examples/TrafficPDE1D/Backstepping control.ipynb) in closed loop with the reference's own TrafficPDE1D.

The controller is NOT restated here: at generation time the notebook's JSON is read from the reference checkout and the one code
cell that defines ``bcksController`` is exec'd, so every command in the fixture comes out of the reference's text and no line of it
is committed.  The episode loop around it is the notebook's (reset, then command / step until terminated or truncated).

Cases: simulation type in (outlet, both, inlet) x control_freq in (1, 2) at the notebook's parameters (T=240, dt=0.25, dx=10, X=500,
v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60), and one small grid (X=110: M = 12 nodes, outlet, control_freq 1).
Stored per case: the commands, rewards and flags of every step, the observations of steps 0-40 and 950-970 (the PDE freezes at step
960 = T/dt while the episode runs to T/dt seconds = 3 840 steps: kept), the episode's reward sum and length.

Run:  python tests/golden/make_golden_traffic_backstep.py [--check]      (needs the reference checkout; not run on the GPU box)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import REF, import_reference  # noqa: E402

FILE = "traffic_backstep.npz"
NOTEBOOK = os.path.join("examples", "TrafficPDE1D", "Backstepping control.ipynb")
BASE = dict(T=240, dt=0.25, X=500, dx=10, v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60)
OBS_STEPS = np.array(list(range(0, 41)) + list(range(950, 971)), dtype=np.int64)
CASES = {f"{sim}_cf{cf}": dict(BASE, simulation_type=sim, control_freq=cf) for sim in ("outlet", "both", "inlet") for cf in (1, 2)}
CASES["outlet_m12"] = dict(BASE, X=110, simulation_type="outlet", control_freq=1)
SHAREABLE = ("obs", "rewards", "done", "truncated", "command_outlet")
PARAM_KEYS = ("T", "dt", "X", "dx", "v_steady", "ro_steady", "v_max", "ro_max", "tau", "control_freq")


def notebook_controller():
    """``bcksController`` of the notebook: the source of the code cell that defines it, exec'd in a namespace of its own."""
    with open(os.path.join(REF, NOTEBOOK)) as f:
        cells = json.load(f)["cells"]
    src = [c["source"] for c in cells if c["cell_type"] == "code" and "def bcksController" in "".join(c["source"])]
    assert len(src) == 1, "the notebook no longer defines bcksController in exactly one cell"
    ns = {"np": np}
    exec("".join(src[0]) if isinstance(src[0], list) else src[0], ns)
    return ns["bcksController"]


def run_case(src, controller, kw):
    with contextlib.redirect_stdout(io.StringIO()):
        env = src.TrafficPDE1D(reward_class=src.TrafficARZReward(), **kw)
        obs, _ = env.reset()
    observations, commands, rewards, done, truncated = [np.array(obs, dtype=np.float64).reshape(-1)], [], [], [], []
    terminate = truncate = False
    while not truncate and not terminate:
        action = controller(env, obs, None)
        obs, reward, terminate, truncate, _ = env.step(action)
        commands.append(np.array(action, dtype=np.float64).reshape(-1))
        observations.append(np.array(obs, dtype=np.float64).reshape(-1))
        rewards.append(float(reward))
        done.append(bool(terminate))
        truncated.append(bool(truncate))
    total = 0
    for r in rewards:          # the notebook's  rew += rewards
        total += r
    observations, commands = np.stack(observations), np.stack(commands)
    sim = kw["simulation_type"]
    ends = {"inlet": ("command_inlet",), "outlet": ("command_outlet",), "both": ("command_inlet", "command_outlet")}[sim]
    out = {k: np.ascontiguousarray(commands[:, i]) for i, k in enumerate(ends)}      # one column per driven end
    # meta: the notebook's reward sum, the episode's length, the grid's nodes (tests: META_KEYS), then the parameters
    out.update(rewards=np.array(rewards, dtype=np.float64), done=np.array(done, dtype=np.uint8), truncated=np.array(truncated, dtype=np.uint8),
               obs=observations[OBS_STEPS], meta=np.array([total, len(rewards), env.M] + [kw[k] for k in PARAM_KEYS], dtype=np.float64))
    return out


def save(path, store):
    """An .npz (a zip of .npy members, what np.load reads) whose members are each compressed by the better of deflate and LZMA: the
    dense float64 rows come out about a sixth smaller than np.savez_compressed leaves them.  Fixed member dates: the same bytes every run."""
    import zipfile
    import zlib
    import lzma
    with zipfile.ZipFile(path, "w") as z:
        for k, v in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            data = buf.getvalue()
            best = zipfile.ZIP_LZMA if len(lzma.compress(data, preset=9)) + 64 < len(zlib.compress(data, 9)) else zipfile.ZIP_DEFLATED
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = best
            z.writestr(info, data, compresslevel=9 if best == zipfile.ZIP_DEFLATED else None)


def generate(out=HERE):
    src = import_reference()
    controller = notebook_controller()
    store = {}
    runs = {name: run_case(src, controller, kw) for name, kw in CASES.items()}
    for name, run in runs.items():
        # 'both' holds its inlet at qs, which is what 'outlet' does by itself: where an array of a 'both' case equals the outlet case's
        # bit for bit it is stored once, and <case>/shares names the case that holds it (tests: traffic_backstep_restatement.golden_case)
        twin = runs.get(name.replace("both", "outlet")) if name.startswith("both") else None
        shared = []
        for k, v in run.items():
            assert np.all(np.isfinite(v)), (name, k)
            if twin is not None and k in SHAREABLE and v.shape == twin[k].shape and v.tobytes() == twin[k].tobytes():
                shared.append(k)
            else:
                store[f"{name}/{k}"] = v
        if shared:
            store[f"{name}/shares"] = np.array([name.replace("both", "outlet")] + shared)
    store["obs_steps"] = OBS_STEPS
    path = os.path.join(out, FILE)
    save(path, store)
    return path


def check():
    """Regenerate into a scratch directory and compare with the committed file: same keys, dtypes, shapes and bits."""
    import tempfile
    diffs = []
    with tempfile.TemporaryDirectory() as tmp:
        b = np.load(generate(tmp), allow_pickle=False)
        a = np.load(os.path.join(HERE, FILE), allow_pickle=False)
        for k in sorted(set(a.files) | set(b.files)):
            if k not in a.files or k not in b.files:
                diffs.append(f"{FILE}: key {k} only in the {'generator output' if k in b.files else 'committed file'}")
            elif a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
                diffs.append(f"{FILE}: {k} differs")
    return diffs


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        d = check()
        print("\n".join(d) if d else "fixtures == generator output")
        sys.exit(1 if d else 0)
    p = generate()
    print("wrote", p, os.path.getsize(p), "bytes")
