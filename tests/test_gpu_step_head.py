"""The head of the fast-path 1D step launch (step1d_kernel<HeadArgs, ...>, pdegym_1d.hip): the input row's base, beta and its stride, the
per-instance words and the batch size are the kernel's leading arguments, filled by the launcher from the same structures as before.
What can go wrong there: a leading pointer that does not follow the double-buffered observation from launch to launch (or from node
to node of a captured graph), a beta stride of 0, the `inst >= B` exit of the last workgroup's spare waves, and the rare paths that
re-read through the leading pointers (exact redo) or write through the structure's (auto-reset).

Everything is compared with the NumPy oracle (oracle/pde_oracle.py) as in tests/test_gpu_step_ends.py, whose helpers this file
uses: rows and observations as bit patterns, flags and time indices exactly, rewards to rtol 1e-6.  Every buffer a step writes --
the observation pair, the state rows, reward, norms, flags, time index, |u[-1]| sum, norm ring -- lives in a guarded allocation
(tests/poison.py) whose guard starts right behind row B - 1: a wave with inst >= B that stored anything shows there.

The smallest shapes that take each form of the head: parabolic nx = 256 (rows fill the wave, four slots per lane), nx = 64 (one
slot), nx = 100 (ragged row); transport nx = 128 (two slots) and nx = 512 (eight).
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("parabolic", 256), ("parabolic", 64), ("parabolic", 100), ("transport", 128), ("transport", 512)]
SHAPE_IDS = [f"{k}-nx{n}" for k, n in SHAPES]
STATE_WORDS = ("reward", "norm_now", "norm_back", "terminated", "truncated", "time_index", "bsum", "ring")


def _helpers():
    import torch
    from tests import poison as PZ
    from tests import test_gpu_step_ends as SE
    return torch, PZ, SE


def _start(kind, nx, S, nt, B, state_in, init, beta, **kw):
    """tests/test_gpu_step_ends._start, with the per-instance outputs and state words moved into guarded allocations as well.
    beta of one dimension is shared by the batch (beta_stride = 0)."""
    torch, PZ, SE = _helpers()
    env, orc = SE._pair(kind, SE._kw(kind, nx, S, nt, kw.pop("max_state", 1e10)), B, state_in)
    orc.reset(init, np.broadcast_to(beta, init.shape).copy())
    env.reset(torch.tensor(init), torch.tensor(beta))
    assert env.t["beta"].dim() == beta.ndim
    pool = kw.pop("pool", None)
    if pool is not None:
        env.enable_auto_reset(torch.tensor(pool), keep_final_obs=kw.pop("keep_final_obs", True))
    arena = PZ.Arena("cuda")
    SE._guard(env, arena)
    for k in STATE_WORDS:
        env.t[k] = arena.like(k, env.t[k])
    if env.t["reset_count"] is not None:
        env.t["reset_count"] = arena.like("reset_count", env.t["reset_count"])
    return env, orc, arena


@pytest.mark.gpu
@pytest.mark.parametrize("state_in", [True, False], ids=["state_in", "own_u"])
@pytest.mark.parametrize("kind,nx", SHAPES, ids=SHAPE_IDS)
def test_ragged_batches_three_steps_both_beta_layouts(kind, nx, state_in):
    """B in {1, 3, 4, 5, 9} (the last workgroup has waves with inst >= B) x S in {1, 3} x beta per instance / shared: three
    consecutive steps, so the input row alternates between the two observation buffers."""
    torch, PZ, SE = _helpers()
    n = nx + (kind == "parabolic")
    for B in (1, 3, 4, 5, 9):
        for S in (1, 3):
            for shared in (False, True):
                rng, init, beta = SE._random_case(kind, n, B, 1000 * nx + 10 * B + S)
                env, orc, arena = _start(kind, nx, S, 4 * S + 1, B, state_in, init, beta[0] if shared else beta)
                for i in range(3):
                    a = rng.uniform(-1, 1, B).astype(np.float32)
                    SE._step_and_compare(env, orc, arena, a, f"{kind} nx={nx} B={B} S={S} shared={shared} step {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("state_in", [True, False], ids=["state_in", "own_u"])
@pytest.mark.parametrize("kind,nx", [("parabolic", 256), ("parabolic", 100), ("transport", 512)])
def test_captured_graph_nodes_carry_their_own_leading_pointers(kind, nx, state_in):
    """Three steps captured into one graph and replayed twice from the same start: node i must read the buffer node i - 1 wrote.
    Both replays give the oracle's third row."""
    torch, PZ, SE = _helpers()
    B, S = 5, 3
    n = nx + (kind == "parabolic")
    rng, init, beta = SE._random_case(kind, n, B, 31 * nx)
    acts = rng.uniform(-1, 1, (3, B)).astype(np.float32)
    warm, _, _ = _start(kind, nx, S, 4 * S + 1, B, state_in, init, beta)
    warm.step(torch.tensor(acts[0]))          # the code object is loaded before anything is captured
    env, orc, arena = _start(kind, nx, S, 4 * S + 1, B, state_in, init, beta)
    dev_acts = [torch.tensor(a, device="cuda") for a in acts]
    keep = {k: env.t[k].clone() for k in ("time_index", "bsum", "ring")}
    row0 = env.t["obs"].clone()
    start = env.t["obs"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for a in dev_acts:
                out = env.step(a)
    with np.errstate(all="ignore"):
        for a in acts:
            o_ref, r_ref, te_ref, tr_ref = orc.step(a)
    for replay in range(2):
        for k, v in keep.items():
            env.t[k].copy_(v)
        for o in env._obs:
            PZ.poison_(o)
        if not state_in:
            env.t["u"].copy_(row0)
        start.copy_(row0)
        g.replay()
        arena.check()
        o, r, te, tr = (x.cpu().numpy() for x in out)
        SE._assert_bits(o, o_ref, f"{kind} nx={nx} replay {replay}: obs")
        SE._assert_bits(env.u.cpu().numpy(), o_ref, f"{kind} nx={nx} replay {replay}: u")
        SE._assert_reward(r, r_ref, orc.norm_now, f"replay {replay}")
        np.testing.assert_array_equal(te.astype(bool), te_ref)
        np.testing.assert_array_equal(tr.astype(bool), tr_ref)
        np.testing.assert_array_equal(env.time_index.cpu().numpy(), orc.time_index)


@pytest.mark.gpu
@pytest.mark.parametrize("state_in", [True, False], ids=["state_in", "own_u"])
@pytest.mark.parametrize("kind,nx", [("parabolic", 256), ("parabolic", 100), ("transport", 128), ("transport", 512)])
def test_rare_paths_between_ordinary_instances(kind, nx, state_in):
    """In one batch of 9: an instance at time index nt - 2 whose step ends the episode (fused auto-reset from the pool), an instance
    with a non-finite node (exact redo: the row is read again through the leading pointer) between finite neighbours, and a command
    of exactly -0.0."""
    torch, PZ, SE = _helpers()
    B, S, nt = 9, 3, 150
    n = nx + (kind == "parabolic")
    rng, init, beta = SE._random_case(kind, n, B, 7 * nx + 1)
    init[5, n // 2] = np.inf
    pool = rng.uniform(1, 3, (2 * B, n)).astype(np.float32)
    env, orc, arena = _start(kind, nx, S, nt, B, state_in, init, beta, pool=pool)
    orc.time_index[4] = nt - 2
    env.t["time_index"][4] = nt - 2
    a = rng.uniform(-1, 1, B).astype(np.float32)
    a[7] = -0.0
    ended = SE._step_and_compare(env, orc, arena, a, f"{kind} nx={nx}", reset_rows="oracle", pool=pool)
    # the row holding inf: its norm is inf or NaN -- inf >= max_state truncates (and restarts), NaN compares false and goes on
    assert ended[4] and not ended[[0, 1, 2, 3, 6, 7, 8]].any()


def test_library_is_built_with_the_options_the_notes_say_were_kept():
    """profiles/r08_ab_notes.txt names the per-file compiler options kept for pdegym_1d.hip after the A/B runs; build.py must compile
    that file with exactly those, no other file with any, and the in-tree library must be the one built from them."""
    from pdecontrolgym_amd import build
    text = open(os.path.join(ROOT, "profiles", "r08_ab_notes.txt")).read()
    m = re.search(r"^KEPT per-file options of pdegym_1d\.hip: (.*)$", text, re.M)
    assert m, "profiles/r08_ab_notes.txt has no 'KEPT per-file options of pdegym_1d.hip:' line"
    kept = [] if m.group(1).strip() == "(none)" else m.group(1).split()
    assert build.FILE_OPTS.get("pdegym_1d.hip", []) == kept
    assert all(not v for k, v in build.FILE_OPTS.items() if k != "pdegym_1d.hip")
    build.build()
    assert build.library_stamp() == build._fingerprint()
