"""GPU tests of pdegym_squashed_gaussian_sample, its backward, pdegym_sac_critic_loss and pdegym_sac_actor_loss
(csrc/pdegym_sac_loss.hip) and pde_control_gym.SACLoss: the parts of the heads that neither exp, tanh nor log decides against the
NumPy restatement (tests/sac_loss_restatement.py) BIT FOR BIT, the real-valued parts held to the error of the eager torch float32
composition against float64, saturation, non-finite data, a captured graph, and the head behind three FusedMLP.with_grad networks.

Every launch of this file goes through ``_sample`` / ``_backward`` / ``_critic`` / ``_actor``, which ALWAYS check the poisoned-buffer
contract of tests/poison.py: inputs live in guarded buffers whose padding columns hold poison, outputs and the workspace are poisoned
and guarded, and after the launch every output element of rows i < N is written, the padding columns and all guards are untouched,
every input is bit-unchanged -- and a launch with a workspace is made TWICE, on two differently poisoned workspaces, and must give
the same bits.  ``policy`` displaces every buffer off its 256-byte boundary (tests/poison.py; the policies of
tests/test_gpu_pointer_alignment.py): the workspace, a buffer of 32-bit words, then starts 4, 8 or 12 bytes past one -- under "one" 4,
which is no 8-byte boundary for the doubles in it.

Tolerance factor of the real-valued parts: e_kernel <= M_FACTOR * e_torch + 2^-20 (the rule and the floor of DESIGN.md section 4.13).
M_FACTOR = 8 was measured on the first run of these cases (every pair is in profiles/r14_sac_loss.json, "tolerance"; DESIGN.md
section 4.16): the worst ratio among pairs with e_torch >= 2^-24 is 3.8 (the first latent bias of the end-to-end case's actor step, a
sum over rows that cancels), doubled and rounded up to a power of two.  Pairs whose e_torch is below 2^-24 -- two sub-ulp errors,
whatever their ratio -- pass through the 2^-20 floor: the largest e_kernel among them is 2.6e-7."""
import math

import numpy as np
import pytest

from tests import nonfinite, poison
from tests import sac_loss_restatement as R
from tests.test_gpu_pointer_alignment import POLICIES as DISPLACED
from tests.test_sac_loss import sb3_actor_losses, sb3_critic_loss, sb3_sample

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = 256            # csrc/pdegym_sac_loss.hip: kRows, rows per workgroup and chunk (one row per lane)
GROUPS = 256          # kMaxGroups: past ROWS * GROUPS rows a workgroup takes a second chunk
# one row; around a wave; one short of / exactly / one past a workgroup's rows; four workgroups, the last a single row
N_LIST = (1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 1)
N_SECOND_CHUNK = ROWS * GROUPS + 1
A_LIST = (1, 2, 8)
POLICIES = (None,) + tuple(DISPLACED)
LO, HI = -20.0, 2.0
GAMMA, TARGET_ENTROPY = 0.99, -1.5
M_FACTOR = 8
FLOOR = 2.0 ** -20
WS_FILLS = (0x7FF8DEAD, -0x0123457)      # (as doubles: a NaN pattern, then a huge negative number)


def _backend():
    from pdecontrolgym_amd.backend import default_backend
    return default_backend()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _wide(arena, name, a, extra):
    """``a`` [n, w] in the first w columns of a guarded [n, w + extra] buffer whose other columns hold poison."""
    full = arena.new(name, (a.shape[0], a.shape[1] + extra), torch.float32)
    poison.poison_(full)
    full[:, :a.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return full


def _check_columns(t, lo, hi, name):
    inside = torch.zeros(t.shape[1], dtype=torch.bool, device=t.device)
    inside[lo:hi] = True
    poison.assert_written(t, (slice(None), inside), name)
    if not bool(inside.all()):
        poison.assert_untouched(t, (slice(None), ~inside), name + " outside its columns")


def _sample(case, pad=(0, 0, 0, 0), policy=None, lo=LO, hi=HI):
    """One pdegym_squashed_gaussian_sample call on guarded copies; ``pad``: extra columns of raw, eps, obs and the output block.
    Returns (block [N, D + A], log_prob [N])."""
    n, A = case["eps"].shape
    obs = case.get("obs")
    D = 0 if obs is None else obs.shape[1]
    arena = poison.Arena("cuda", policy=policy)
    ins = {"raw": _wide(arena, "raw", case["raw"], pad[0]), "eps": _wide(arena, "eps", case["eps"], pad[1])}
    if obs is not None:
        ins["obs"] = _wide(arena, "obs", obs, pad[2])
    before = {k: v.clone() for k, v in ins.items()}
    block = poison.poison_(arena.new("actions", (n, D + A + pad[3]), torch.float32))
    logp = poison.poison_(arena.new("log_prob", (n,), torch.float32))
    _backend().squashed_gaussian_sample(ins["raw"][:, :2 * A], ins["eps"][:, :A], block[:, :D + A], logp, lo, hi,
                                        obs=None if obs is None else ins["obs"][:, :D])
    arena.check()
    _check_columns(block, 0, D + A, "actions")
    poison.assert_written(logp, None, "log_prob")
    for k, x in before.items():
        poison.assert_bits_equal(ins[k], x, None, k)
    return block[:, :D + A].cpu().numpy().copy(), logp.cpu().numpy().copy()


def _backward(case, d_actions, d_log_prob, pad=(0, 0, 0), policy=None, lo=LO, hi=HI, block_D=0):
    """One pdegym_squashed_gaussian_sample_backward call.  ``d_actions`` [N, A] or None -- with ``block_D`` it sits in columns
    [block_D, block_D + A) of a [N, block_D + A] block, like a critic's dx, and is passed in place; ``d_log_prob`` [N], a Python
    float (ONE device scalar) or None.  ``pad``: extra columns of raw, eps, d_raw.  Returns d_raw [N, 2A]."""
    n, A = case["eps"].shape
    arena = poison.Arena("cuda", policy=policy)
    ins = {"raw": _wide(arena, "raw", case["raw"], pad[0]), "eps": _wide(arena, "eps", case["eps"], pad[1])}
    da = dl = None
    if d_actions is not None:
        full = poison.poison_(arena.new("d_actions", (n, block_D + A), torch.float32))
        full[:, block_D:].copy_(torch.from_numpy(d_actions))
        ins["d_actions"] = full
        da = full[:, block_D:]
    if d_log_prob is not None:
        if isinstance(d_log_prob, float):
            ins["d_log_prob"] = arena.like("d_log_prob", torch.tensor([d_log_prob], dtype=torch.float32))
            dl = ins["d_log_prob"].expand(n)
        else:
            dl = ins["d_log_prob"] = arena.like("d_log_prob", torch.from_numpy(d_log_prob))
    before = {k: v.clone() for k, v in ins.items()}
    d_raw = poison.poison_(arena.new("d_raw", (n, 2 * A + pad[2]), torch.float32))
    _backend().squashed_gaussian_sample_backward(ins["raw"][:, :2 * A], ins["eps"][:, :A], da, dl, d_raw[:, :2 * A], lo, hi)
    arena.check()
    _check_columns(d_raw, 0, 2 * A, "d_raw")
    for k, x in before.items():
        poison.assert_bits_equal(ins[k], x, None, k)
    return d_raw[:, :2 * A].cpu().numpy().copy()


def _with_workspace(arena, n, launch, outs, ins, before):
    bk = _backend()
    need = int(bk.lib.pdegym_sac_loss_workspace(n))
    assert need > 0 and need % 4 == 0
    ws = arena.new("workspace", (need // 4,), torch.int32)
    runs = []
    for fill in WS_FILLS:
        for x in outs.values():
            poison.poison_(x)
        ws.fill_(fill)
        launch(bk, ws.view(torch.uint8))
        arena.check()                                        # (synchronises) no guard byte changed
        for k, x in outs.items():
            poison.assert_written(x, None, k)
        for k, x in before.items():
            poison.assert_bits_equal(ins[k], x, None, k)
        runs.append({k: x.cpu().numpy().copy() for k, x in outs.items()})
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{k} depends on what the workspace held before the call"
    return runs[0]


def _critic(case, index=None, two=True, log_alpha=0.0, gamma=GAMMA, policy=None):
    """One pdegym_sac_critic_loss call (made twice, see the module docstring).  Returns d_q1, d_q2, target, stats."""
    n = case["q1"].shape[0]
    arena = poison.Arena("cuda", policy=policy)
    names = ("q1", "q1_target", "next_log_prob", "rewards", "dones") + (("q2", "q2_target") if two else ())
    ins = {k: arena.like(k, torch.from_numpy(case[k])) for k in names}
    ins["log_alpha"] = arena.like("log_alpha", torch.tensor([log_alpha], dtype=torch.float32))
    if index is not None:
        assert index.min() >= 0 and index.max() < case["rewards"].shape[0] and index.shape == (n,)
        ins["index"] = arena.like("index", torch.from_numpy(index))
    before = {k: v.clone() for k, v in ins.items()}
    outs = {k: arena.new(k, (n,), torch.float32) for k in ("d_q1", "target") + (("d_q2",) if two else ())}
    outs["stats"] = arena.new("stats", (4,), torch.float32)

    def launch(bk, ws):
        bk.sac_critic_loss(ins["q1"], ins.get("q2"), ins["q1_target"], ins.get("q2_target"), ins["next_log_prob"], ins["rewards"],
                           ins["dones"], ins["log_alpha"], gamma, outs["d_q1"], outs.get("d_q2"), target=outs["target"], stats=outs["stats"],
                           index=ins.get("index"), workspace=ws)
    return _with_workspace(arena, n, launch, outs, ins, before)


def _actor(case, two=True, log_alpha=0.0, target_entropy=TARGET_ENTROPY, policy=None):
    """One pdegym_sac_actor_loss call (made twice).  Returns d_q1_pi, d_q2_pi, d_log_prob [1], d_log_alpha [1], stats."""
    n = case["q1"].shape[0]
    arena = poison.Arena("cuda", policy=policy)
    ins = {k: arena.like(k, torch.from_numpy(case[k])) for k in ("q1", "log_prob") + (("q2",) if two else ())}
    ins["log_alpha"] = arena.like("log_alpha", torch.tensor([log_alpha], dtype=torch.float32))
    before = {k: v.clone() for k, v in ins.items()}
    outs = {k: arena.new(k, (n,), torch.float32) for k in ("d_q1_pi",) + (("d_q2_pi",) if two else ())}
    outs.update(d_log_prob=arena.new("d_log_prob", (1,), torch.float32), d_log_alpha=arena.new("d_log_alpha", (1,), torch.float32),
                stats=arena.new("stats", (4,), torch.float32))

    def launch(bk, ws):
        bk.sac_actor_loss(ins["q1"], ins.get("q2"), ins["log_prob"], ins["log_alpha"], target_entropy, outs["d_q1_pi"], outs.get("d_q2_pi"),
                          outs["d_log_prob"], outs["d_log_alpha"], stats=outs["stats"], workspace=ws)
    return _with_workspace(arena, n, launch, outs, ins, before)


def _critic_args(case, two=True):
    return (case["q1"], case["q2"] if two else None, case["q1_target"], case["q2_target"] if two else None, case["next_log_prob"],
            case["rewards"], case["dones"])


def _index(n, rows, seed, repeated=False):
    rng = np.random.default_rng([seed, n, rows])
    if repeated:
        return rng.integers(0, max(rows // 4, 1), n).astype(np.int64)
    return rng.permutation(rows)[:n].astype(np.int64)


# ---- exact parts ------------------------------------------------------------------------------------------------------------------------
def _integer_critic_case(n, seed):
    """Integer-valued q, r and next log-probabilities, d in {0, 1}; with gamma = 0.5 and alpha == 1 every value of a row is a
    multiple of 0.5 far below 2^24: target, errors and squares are exact in float32, the sums exact in float64 in any order."""
    rng = np.random.default_rng([seed, n, 5])
    rows = 3 * n
    f = lambda lo, hi, k: rng.integers(lo, hi, k).astype(np.float32)      # noqa: E731
    return {"q1": f(-40, 40, n), "q2": f(-40, 40, n), "q1_target": f(-40, 40, n), "q2_target": f(-40, 40, n),
            "next_log_prob": f(-8, 8, n), "rewards": f(-20, 20, rows), "dones": f(0, 2, rows)}, _index(n, rows, seed)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("two", [True, False], ids=["twin", "single"])
def test_critic_gradient_target_and_loss_are_exact_on_integer_data(two, policy):
    sizes = N_LIST + ((N_SECOND_CHUNK,) if two and policy is None else ())
    assert any(n & (n - 1) == 0 and n > 1 for n in sizes)
    for n in sizes:
        case, index = _integer_critic_case(n, seed=n)
        got = _critic(case, index, two=two, log_alpha=0.0, gamma=0.5, policy=policy)
        want = R.critic_float32(*_critic_args(case, two), 0.0, 0.5, index=index)
        for k in ("d_q1", "target") + (("d_q2",) if two else ()):
            np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{k} n={n}")
        np.testing.assert_array_equal(_bits(got["stats"]), _bits(want["stats"]), err_msg=f"stats n={n}")
        # and the same from the definition, in float64
        q1, q2, r, d = (case[k].astype(np.float64) for k in ("q1", "q2", "rewards", "dones"))
        m = np.minimum(case["q1_target"], case["q2_target"]) if two else case["q1_target"]
        y = r[index] + (1 - d[index]) * 0.5 * (m.astype(np.float64) - case["next_log_prob"])
        np.testing.assert_array_equal(got["target"], y)
        sq = ((q1 - y) ** 2).sum() + (((q2 - y) ** 2).sum() if two else 0.0)
        np.testing.assert_array_equal(got["stats"][0], np.float32(0.5 * sq / n))
        np.testing.assert_array_equal(got["d_q1"], ((q1 - y).astype(np.float32) * np.float32(1.0 / n)))
    # alpha = exp(0) reads back as exactly 1
    lp = {"q1": case["q1"], "q2": case["q2"], "log_prob": case["next_log_prob"]}
    assert _actor(lp, two=two, log_alpha=0.0, policy=policy)["stats"][2] == 1.0


def _margin_actor_case(n, seed):
    """q2 = q1 +- (1e-3 + |draw|): the margin between the critics is there by construction (asserted, never trimmed); ties planted in
    every seventh row, starting at row 0."""
    rng = np.random.default_rng([seed, n, 9])
    q1 = rng.normal(0.0, 3.0, n).astype(np.float32)
    gap = (1e-3 + np.abs(rng.normal(0.0, 1.0, n))) * rng.choice([-1.0, 1.0], n)
    q2 = (q1.astype(np.float64) + gap).astype(np.float32)
    ties = np.arange(0, n, 7)
    q2[ties] = q1[ties]
    free = np.setdiff1d(np.arange(n), ties)
    assert (np.abs(q2[free].astype(np.float64) - q1[free]) >= 9e-4).all()
    return {"q1": q1, "q2": q2, "log_prob": rng.normal(-1.0, 1.0, n).astype(np.float32)}, ties, free


@pytest.mark.parametrize("policy", POLICIES)
def test_actor_zero_pattern_ties_and_scalars(policy):
    sizes = N_LIST + ((N_SECOND_CHUNK,) if policy is None else ())
    for n in sizes:
        case, ties, free = _margin_actor_case(n, seed=n)
        got = _actor(case, log_alpha=-0.25, policy=policy)
        want = R.actor_float32(case["q1"], case["q2"], case["log_prob"], -0.25, TARGET_ENTROPY)
        g = np.float32(-np.float32(1.0 / n))
        np.testing.assert_array_equal(_bits(got["d_q1_pi"]), _bits(want["d_q1_pi"]))
        np.testing.assert_array_equal(_bits(got["d_q2_pi"]), _bits(want["d_q2_pi"]))
        assert (got["d_q1_pi"][ties] == g).all() and (_bits(got["d_q2_pi"][ties]) == 0).all(), "a tie goes to the first critic"
        second = case["q2"][free] < case["q1"][free]
        assert ((got["d_q2_pi"][free] == g) == second).all() and ((got["d_q1_pi"][free] == 0) == second).all()
        assert n < 64 or (second.any() and (~second).any())
        # log_prob alone decides d_log_alpha and the mean: float64 sums of float32 terms rounded once -- NumPy adds them in another
        # order, which moves the float64 sum by a few 2^-53 and the rounded result by one float32 ulp at most
        np.testing.assert_allclose(got["d_log_alpha"], want["d_log_alpha"], rtol=2.0 ** -23)
        np.testing.assert_allclose(got["stats"][3], want["stats"][3], rtol=2.0 ** -23)
        # alpha = expf(-0.25): d_log_prob is its single product with (float)(1 / N)
        np.testing.assert_array_equal(got["d_log_prob"][0], got["stats"][2] * np.float32(1.0 / n))
        assert abs(float(got["stats"][2]) - math.exp(-0.25)) <= 2.0 ** -23
        one = _actor(case, two=False, log_alpha=-0.25, policy=policy)
        assert (one["d_q1_pi"] == g).all()


def _mask_case(n, A, seed, eps_zero=False):
    """Rows 0 .. 3 (of every 16): log_std exactly on the minimum, exactly on the maximum, 1e-3 below and 1e-3 above (float32)."""
    case = R.seeded_sample_case(n, A, seed=seed)
    rows = {k: np.arange(k, n, 16) for k in range(4)}
    for k, v in enumerate((np.float32(LO), np.float32(HI), np.float32(LO) - np.float32(1e-3), np.float32(HI) + np.float32(1e-3))):
        assert (v < LO) if k == 2 else (v > HI) if k == 3 else True
        case["raw"][rows[k], A:] = v
        case["raw"][rows[k], :A] *= np.float32(0.25)
    case["eps"][np.concatenate([rows[1], rows[3]])] *= np.float32(0.05)      # sigma = e^2 there: keep z moderate
    if eps_zero:
        case["eps"][:] = 0.0
    return case, rows


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("A", A_LIST)
def test_clip_mask_of_the_log_std_gradient(A, policy):
    """On either bound the clamp passes the gradient (non-zero: it contains -d_log_prob), 1e-3 outside the gate selects exactly
    +0; with eps == 0 the forward log-probability of those rows is the restatement's."""
    for n in (65, ROWS + 1, 3 * ROWS + 1):
        case, rows = _mask_case(n, A, seed=n + A)
        rng = np.random.default_rng(n)
        d_a = rng.normal(0.0, 1.0, (n, A)).astype(np.float32)
        d_lp = (rng.choice([-1.0, 1.0], n) * (0.5 + np.abs(rng.normal(0.0, 1.0, n)))).astype(np.float32)
        got = _backward(case, d_a, d_lp, pad=(1, 2, 3), policy=policy)
        want = R.sample_backward_float32(case["raw"], case["eps"], LO, HI, d_a, d_lp)
        on = np.concatenate([rows[0], rows[1]])
        out = np.concatenate([rows[2], rows[3]])
        assert (got[on, A:] != 0).all(), "on the closed interval the gradient passes"
        assert (_bits(got[out, A:]) == 0).all(), "outside it the gradient is exactly +0"
        assert (got[out, :A] != 0).all() and ((got[:, A:] == 0) == (want[:, A:] == 0)).all()
        zero = _mask_case(n, A, seed=n + A, eps_zero=True)[0]
        _, lp = _sample(zero, pad=(2, 0, 0, 1), policy=policy)
        _, lp32 = R.sample_float32(zero["raw"], zero["eps"], LO, HI)
        _, lp64 = R.sample_float64(zero["raw"], zero["eps"], LO, HI)
        planted = np.concatenate([on, out])
        scale = np.abs(lp64[planted]).max()
        e_kernel, e_rest = np.abs(lp[planted] - lp64[planted]).max() / scale, np.abs(lp32[planted] - lp64[planted]).max() / scale
        assert e_kernel <= M_FACTOR * e_rest + FLOOR, (e_kernel, e_rest)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("A", A_LIST)
def test_one_row_probes_pin_the_gathers_the_strides_and_the_fused_block(A, policy):
    n, D = ROWS + 7, 5
    rows = 3 * n
    for i0 in (0, ROWS - 1, ROWS, n - 1):
        # the fused block: observation columns bit-equal, nothing written past column D + A (the poisoned padding is checked by
        # _sample), the action columns those of the call without obs
        case = R.seeded_sample_case(n, A, seed=i0 + A, D=D)
        block, lp = _sample(case, pad=(3, 1, 2, 4), policy=policy)
        alone, lp_alone = _sample({k: case[k] for k in ("raw", "eps")}, pad=(0, 2, 0, 1), policy=policy)
        np.testing.assert_array_equal(_bits(block[:, :D]), _bits(case["obs"]))
        np.testing.assert_array_equal(_bits(block[:, D:]), _bits(alone))
        np.testing.assert_array_equal(_bits(lp), _bits(lp_alone))
        # d_actions read in place from a [N, D + A] block, non-zero in ONE row: d_raw is non-zero in that row only
        d_a = np.zeros((n, A), np.float32)
        d_a[i0] = 1.0 + np.arange(A, dtype=np.float32)
        got = _backward(case, d_a, None, pad=(2, 3, 1), policy=policy, block_D=D)
        ref = R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, None)
        hit = np.zeros(n, bool)
        hit[i0] = True
        assert (got[~hit] == 0).all() and (got[hit] != 0).all()
        np.testing.assert_allclose(got[i0], ref[i0], rtol=1e-3)      # (w = 1 - a^2 >= 1.3e-3 carries a relative error of up to 1e-4)
        dense = _backward(case, d_a, None, policy=policy)
        np.testing.assert_array_equal(_bits(got), _bits(dense))
        # the one device scalar equals the dense array of equal entries
        a = _backward(case, d_a, 0.375, pad=(0, 1, 2), policy=policy)
        b = _backward(case, d_a, np.full(n, 0.375, np.float32), pad=(1, 0, 0), policy=policy)
        np.testing.assert_array_equal(_bits(a), _bits(b))
        # the critic's gather: rewards zero except at ONE buffer row, reached from one minibatch row
        loss = R.seeded_loss_case(n, seed=i0, rows=rows)
        index = _index(n, rows, seed=i0 + 1)
        loss["rewards"][:] = 0.0
        loss["dones"][:] = 0.0
        with_r = {**loss, "rewards": loss["rewards"].copy()}
        with_r["rewards"][int(index[i0])] = 64.0
        base = _critic(loss, index, policy=policy)
        got = _critic(with_r, index, policy=policy)
        moved = got["target"] != base["target"]
        assert moved[i0] and moved.sum() == 1 and abs(float(got["target"][i0] - base["target"][i0]) - 64.0) < 1e-3


@pytest.mark.parametrize("two", [True, False], ids=["twin", "single"])
def test_dense_call_on_gathered_arrays_equals_the_indexed_call(two):
    for n in (65, 3 * ROWS + 1):
        for repeated in (False, True):
            case = R.seeded_loss_case(n, seed=n, rows=3 * n)
            index = _index(n, 3 * n, seed=n, repeated=repeated)
            a = _critic(case, index, two=two, log_alpha=-0.5)
            dense = {**case, "rewards": case["rewards"][index], "dones": case["dones"][index]}
            b = _critic(dense, None, two=two, log_alpha=-0.5)
            for k in a:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, n, repeated)
            c = _critic(case, index, two=two, log_alpha=-0.5)                       # and a second call gives the same bits
            for k in a:
                assert np.array_equal(_bits(a[k]), _bits(c[k])), (k, n)


@pytest.mark.parametrize("A", A_LIST)
def test_saturated_rows(A):
    """|z| >= 20: a = +-1 exactly, log_prob finite, and k = 2 a w / u exactly 0 -- d_mu = d_a * w + d_lp * k is +-0, d_log_std is
    (d_lp * -1) to the last bit."""
    n = ROWS + 3
    case = R.seeded_sample_case(n, A, seed=A)
    sat = np.arange(0, n, 9)
    sign = np.where(np.arange(sat.size) % 2 == 0, 1.0, -1.0)[:, None]
    case["raw"][sat, :A] = (sign * np.linspace(20.0, 60.0, sat.size)[:, None]).astype(np.float32)
    case["raw"][sat, A:] = -1.0
    case["eps"][sat] = np.float32(0.5) * sign.astype(np.float32)
    block, lp = _sample(case, pad=(1, 1, 0, 2))
    assert (block[sat] == sign).all() and np.isfinite(lp).all() and (np.abs(block) <= 1).all()
    rng = np.random.default_rng(A)
    d_a, d_lp = rng.normal(0, 1, (n, A)).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    got = _backward(case, d_a, d_lp, pad=(1, 0, 1))
    assert (got[sat, :A] == 0).all(), "w == 0 and k == 0: nothing reaches mu"
    np.testing.assert_array_equal(got[sat, A:], np.repeat(-d_lp[sat, None], A, axis=1))
    assert (R.saturation_k_float32(case["raw"], case["eps"], LO, HI)[sat] == 0).all()
    want32, lp32 = R.sample_float32(case["raw"], case["eps"], LO, HI)
    np.testing.assert_allclose(lp[sat], lp32[sat], rtol=1e-6)


# ---- real-valued parts -------------------------------------------------------------------------------------------------------------------
def _rel(x, x64):
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    scale = np.abs(x64).max()
    return np.abs(x - x64).max() / scale if scale > 0 else (0.0 if np.abs(x - x64).max() == 0 else np.inf)


def _assert_held_to_torch(what, errors):
    """e_kernel <= M_FACTOR * e_torch + 2^-20 for every pair; each is printed first (pytest -s shows them)."""
    for label, ek, et in errors:
        print(f"SAC-LOSS-RATIO {what} {label} e_kernel {ek:.3e} e_torch {et:.3e} ratio {ek / et if et > 0 else float('nan'):.3f}")
    failures = [(label, ek, et) for label, ek, et in errors if not ek <= M_FACTOR * et + FLOOR]
    assert not failures, (what, failures)


REAL_CASES = [(63, 1), (65, 2), (ROWS + 1, 8), (3 * ROWS + 1, 2), (2048, 1), (N_SECOND_CHUNK, 1)]


def real_case_errors(n, A):
    """[(label, e_kernel, e_torch)] of one real-valued case, e = max|x - x64| / max|x64| against the float64 restatement on the
    CPU; e_torch is the error of the eager torch float32 composition (SB3's expressions under autograd) on the device.  |z| <= 4 and
    log_std in [-3, 1] (R.seeded_sample_case).  tools/measure_sac_loss.py records the pairs."""
    case = R.seeded_sample_case(n, A, seed=n + A, D=3)
    rng = np.random.default_rng([n, A, 3])
    d_a = rng.normal(0.0, 1.0, (n, A)).astype(np.float32)
    d_lp = rng.normal(0.0, 1.0, n).astype(np.float32)
    out = []
    # sample and its backward
    block, lp = _sample(case, pad=(1, 0, 2, 1))
    d_raw = _backward(case, d_a, d_lp, pad=(0, 1, 2))
    b64, lp64 = R.sample_float64(case["raw"], case["eps"], LO, HI, case["obs"])
    g64 = R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, d_lp)
    raw_t = torch.from_numpy(case["raw"]).cuda().requires_grad_()
    a_t, lp_t = sb3_sample(raw_t, torch.from_numpy(case["eps"]).cuda())
    torch.autograd.backward([a_t, lp_t], [torch.from_numpy(d_a).cuda(), torch.from_numpy(d_lp).cuda()])
    out += [("actions", _rel(block[:, 3:], b64[:, 3:]), _rel(a_t.detach().cpu().numpy(), b64[:, 3:])),
            ("log_prob", _rel(lp, lp64), _rel(lp_t.detach().cpu().numpy(), lp64)),
            ("d_raw", _rel(d_raw, g64), _rel(raw_t.grad.cpu().numpy(), g64))]
    # critic
    loss = R.seeded_loss_case(n, seed=n, rows=3 * n)
    index = _index(n, 3 * n, seed=n)
    log_alpha = -0.3
    got = _critic(loss, index, log_alpha=log_alpha)
    ref = R.critic_float64(*_critic_args(loss), log_alpha, GAMMA, index=index)
    d = {k: torch.from_numpy(v).cuda() for k, v in loss.items()}
    idx = torch.from_numpy(index).cuda()
    la = torch.tensor([log_alpha], device="cuda", requires_grad=True)
    q1, q2 = d["q1"].requires_grad_(), d["q2"].requires_grad_()
    c_loss, target = sb3_critic_loss(q1, q2, d["q1_target"], d["q2_target"], d["next_log_prob"], d["rewards"][idx], d["dones"][idx], la[0], GAMMA)
    c_loss.backward()
    eager = {"d_q1": q1.grad, "d_q2": q2.grad, "target": target,
             "stats": torch.stack([c_loss.detach(), d["q1"].detach().mean(), d["q2"].detach().mean(), target.mean()])}
    eager = {k: v.detach().cpu().numpy() for k, v in eager.items()}
    out += [(k, _rel(got[k], ref[k]), _rel(eager[k], ref[k])) for k in ("d_q1", "d_q2", "target")]
    out += [(s, _rel(got["stats"][i], ref["stats"][i]), _rel(eager["stats"][i], ref["stats"][i])) for i, s in enumerate(R.CRITIC_STATS)]
    # actor and entropy coefficient
    got = _actor(loss, log_alpha=log_alpha)
    ref = R.actor_float64(loss["q1"], loss["q2"], loss["log_prob"], log_alpha, TARGET_ENTROPY)
    lp_d = d["log_prob"].requires_grad_()
    a_loss, e_loss = sb3_actor_losses(d["q1"].detach(), d["q2"].detach(), lp_d, la[0], TARGET_ENTROPY)
    a_loss.backward()
    e_loss.backward()
    eager = {"d_log_prob": lp_d.grad[:1], "d_log_alpha": la.grad, "stats": torch.stack([a_loss.detach(), e_loss.detach(), la.detach().exp()[0], lp_d.detach().mean()])}
    eager = {k: v.detach().cpu().numpy() for k, v in eager.items()}
    out += [(k, _rel(got[k], ref[k]), _rel(eager[k], ref[k])) for k in ("d_log_prob", "d_log_alpha")]
    out += [(s, _rel(got["stats"][i], ref["stats"][i]), _rel(eager["stats"][i], ref["stats"][i])) for i, s in enumerate(R.ACTOR_STATS)]
    return out


@pytest.mark.parametrize("n,A", REAL_CASES)
def test_real_valued_parts_are_as_close_to_float64_as_eager_torch(n, A):
    _assert_held_to_torch(f"n{n}_A{A}", real_case_errors(n, A))


# ---- non-finite data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 8])
def test_non_finite_inputs_reach_what_the_restatement_says(A):
    n = ROWS + 9
    i_bad = ROWS + 3
    rows = np.zeros(n, bool)
    rows[i_bad] = True
    # a NaN mu: its row of the actions, its log_prob, its row of d_raw's mu columns
    case = R.seeded_sample_case(n, A, seed=11, D=2)
    rng = np.random.default_rng(A)
    d_a, d_lp = rng.normal(0, 1, (n, A)).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    clean_b, clean_lp = _sample(case)
    clean_g = _backward(case, d_a, d_lp)
    assert np.isfinite(clean_b).all() and np.isfinite(clean_lp).all() and np.isfinite(clean_g).all()
    for col in (0, A):                                       # a NaN mean, then a NaN log_std
        bad = {**case, "raw": nonfinite.plant(case["raw"], (i_bad, col))}
        block, lp = _sample(bad)
        want_b, want_lp = R.sample_float64(bad["raw"], bad["eps"], LO, HI, bad["obs"])
        nonfinite.nan_mask_equal(block, want_b, "actions")
        nonfinite.nan_mask_equal(lp, want_lp, "log_prob")
        assert np.isnan(lp[i_bad]) and np.isnan(block[i_bad, 2]) and np.isfinite(block[:, :2]).all()
        nonfinite.same_bits_and_nans(block[~rows], clean_b[~rows], "the other rows of the block")
        nonfinite.same_bits_and_nans(lp[~rows], clean_lp[~rows], "the other rows of log_prob")
        got = _backward(bad, d_a, d_lp)
        nonfinite.nan_mask_equal(got, R.sample_backward_float64(bad["raw"], bad["eps"], LO, HI, d_a, d_lp), "d_raw")
        assert np.isnan(got[i_bad, 0]) and np.isfinite(got[~rows]).all()
        nonfinite.same_bits_and_nans(got[~rows], clean_g[~rows], "the other rows of d_raw")
        if col == A:
            assert got[i_bad, A] == 0, "a NaN log_std is outside the gate: 0 is selected"
    # critic: a NaN q1 row, then a NaN reward
    loss = R.seeded_loss_case(n, seed=12, rows=3 * n)
    index = _index(n, 3 * n, seed=12)
    clean = _critic(loss, index, log_alpha=-0.3)
    assert all(np.isfinite(v).all() for v in clean.values())
    bad = {**loss, "q1": nonfinite.plant(loss["q1"], i_bad)}
    got = _critic(bad, index, log_alpha=-0.3)
    want = R.critic_float64(*_critic_args(bad), -0.3, GAMMA, index=index)
    for k in got:
        nonfinite.nan_mask_equal(got[k], want[k], k)
    assert np.isnan(got["d_q1"][rows]).all() and np.isfinite(got["d_q1"][~rows]).all() and np.isfinite(got["d_q2"]).all()
    assert np.isfinite(got["target"]).all() and np.isnan(got["stats"][[0, 1]]).all() and np.isfinite(got["stats"][[2, 3]]).all()
    nonfinite.same_bits_and_nans(got["d_q1"][~rows], clean["d_q1"][~rows], "the other rows of d_q1")
    bad = {**loss, "rewards": nonfinite.plant(loss["rewards"], int(index[i_bad]))}
    got = _critic(bad, index, log_alpha=-0.3)
    want = R.critic_float64(*_critic_args(bad), -0.3, GAMMA, index=index)
    for k in got:
        nonfinite.nan_mask_equal(got[k], want[k], k)
    for k in ("d_q1", "d_q2", "target"):
        assert np.isnan(got[k][rows]).all() and np.isfinite(got[k][~rows]).all(), k
        nonfinite.same_bits_and_nans(got[k][~rows], clean[k][~rows], k)
    assert np.isnan(got["stats"][[0, 3]]).all() and np.isfinite(got["stats"][[1, 2]]).all()
    # actor: a NaN q2 is minimal and takes the gradient of its row; the sums that contain it are NaN
    clean = _actor(loss, log_alpha=-0.3)
    bad = {**loss, "q2": nonfinite.plant(loss["q2"], i_bad)}
    got = _actor(bad, log_alpha=-0.3)
    want = R.actor_float64(bad["q1"], bad["q2"], bad["log_prob"], -0.3, TARGET_ENTROPY)
    for k in got:
        nonfinite.nan_mask_equal(got[k], want[k], k)
    assert got["d_q2_pi"][i_bad] != 0 and got["d_q1_pi"][i_bad] == 0 and np.isnan(got["stats"][0]) and np.isfinite(got["stats"][1:]).all()
    nonfinite.same_bits_and_nans(got["d_q1_pi"][~rows], clean["d_q1_pi"][~rows], "d_q1_pi")
    np.testing.assert_array_equal(_bits(got["d_log_alpha"]), _bits(clean["d_log_alpha"]))


# ---- SACLoss: graph capture, and behind three with_grad networks -----------------------------------------------------------------------
def test_a_captured_sample_critic_actor_sequence_replays_to_the_eager_bits():
    import pde_control_gym
    n, A, D = 3 * ROWS + 1, 2, 4
    head = pde_control_gym.SACLoss(GAMMA, TARGET_ENTROPY)
    data = []
    for seed in (1, 2):
        c = {**R.seeded_sample_case(n, A, seed=seed, D=D), **R.seeded_loss_case(n, seed=seed, rows=3 * n)}
        c["index"] = _index(n, 3 * n, seed=seed)
        data.append(c)
    dev = {k: torch.from_numpy(v).cuda() for k, v in data[0].items()}
    log_alpha = torch.full((1,), -0.2, device="cuda")

    def call():
        with torch.no_grad():
            block, lp = head.sample(dev["raw"], dev["eps"], obs=dev["obs"])
            crit = head.critic(dev["q1"], dev["q2"], dev["q1_target"], dev["q2_target"], lp, dev["rewards"], dev["dones"], log_alpha, index=dev["index"])
            act = head.actor(dev["q1"], dev["q2"], lp, log_alpha)
            d_raw = head._sample_backward(dev["raw"], dev["eps"], None, act.grad_log_prob.expand(n), D)
        return {"block": block, "log_prob": lp, "critic_stats": crit.stats, "d_q1": crit.grad_q1, "d_q2": crit.grad_q2, "target": crit.target,
                "actor_stats": act.stats, "d_q1_pi": act.grad_q1_pi, "d_q2_pi": act.grad_q2_pi, "d_log_prob": act.grad_log_prob,
                "d_log_alpha": act.grad_log_alpha, "d_raw": d_raw}
    first = call()                                           # warm-up: allocates the outputs and the workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, no parallel branches
        res = call()
    for k in first:
        assert k == "d_raw" or res[k].data_ptr() == first[k].data_ptr(), f"{k}: a warmed-up call allocates nothing"
    for case in reversed(data):                              # new data in the same tensors, eager first, then the replay
        for k, v in dev.items():
            v.copy_(torch.from_numpy(case[k]))
        eager = call()
        torch.cuda.synchronize()
        want = {k: v.clone() for k, v in eager.items()}
        for k, v in eager.items():
            v.zero_()
        res["d_raw"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, w in want.items():
            poison.assert_bits_equal(res[k], w, None, k)
        assert bool(torch.isfinite(res["critic_stats"]).all()) and bool(torch.isfinite(res["actor_stats"]).all())


def end_to_end_errors():
    """A 65-64-64-2 squashed-Gaussian actor and two 66-64-64-1 critics through FusedMLP.with_grad, the three steps of one SAC update
    through the head: the errors of the .grad of every Parameter and of log_alpha against float64 autograd of SB3's expressions on
    the CPU, beside those of torch float32 autograd on the device.  The critic step's gradients and the actor step's are kept apart
    (the actor step also reaches the critics' parameters, as it does in SB3)."""
    import copy
    import pde_control_gym
    from pde_control_gym import FusedMLP
    n, D, A, rows = 1000, 65, 1, 3000
    torch.manual_seed(5)

    def mlp(i, o):
        return torch.nn.Sequential(torch.nn.Linear(i, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, o))
    latent = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh())
    mu, log_std = torch.nn.Linear(64, A), torch.nn.Linear(64, A)
    with torch.no_grad():
        log_std.weight.mul_(0.1)
        log_std.bias.fill_(-1.0)
        mu.weight.mul_(0.3)
    nets = {"latent": latent, "mu": mu, "log_std": log_std, "q1": mlp(D + A, 1), "q2": mlp(D + A, 1), "q1_t": mlp(D + A, 1), "q2_t": mlp(D + A, 1)}
    o, o2 = torch.randn(n, D), torch.randn(n, D)
    act = torch.rand(n, A) * 2 - 1
    eps, eps2 = torch.randn(n, A).clamp(-2.5, 2.5), torch.randn(n, A).clamp(-2.5, 2.5)
    rewards, dones = torch.randn(rows), (torch.rand(rows) < 0.2).float()
    index = torch.from_numpy(_index(n, rows, seed=9))
    trained = ("latent", "mu", "log_std", "q1", "q2")
    names = [f"{w}.{i}" for w in trained for i in range(len(list(nets[w].parameters())))] + ["log_alpha"]

    def update(dtype, device, fused):
        m = {k: copy.deepcopy(v).to(device=device, dtype=dtype) for k, v in nets.items()}
        la = torch.full((1,), -0.3, dtype=dtype, device=device, requires_grad=True)
        t = lambda x: x.to(device=device, dtype=dtype)      # noqa: E731
        params = [p for w in trained for p in m[w].parameters()] + [la]

        def grads():
            out = [None if p.grad is None else p.grad.detach().cpu().numpy().copy() for p in params]
            for p in params:
                p.grad = None
            return out
        if fused:
            head = pde_control_gym.SACLoss(GAMMA, TARGET_ENTROPY)
            raw_fn = FusedMLP.squashed_gaussian(m["latent"], m["mu"], m["log_std"], (LO, HI)).with_grad
            q1_fn, q2_fn = FusedMLP(m["q1"]).with_grad, FusedMLP(m["q2"]).with_grad
            with torch.no_grad():
                block2, lp2 = head.sample(raw_fn(t(o2)), t(eps2), obs=t(o2))
                q1n, q2n = m["q1_t"](block2), m["q2_t"](block2)
            oa = torch.cat([t(o), t(act)], 1)
            head.critic(q1_fn(oa), q2_fn(oa), q1n, q2n, lp2, t(rewards), t(dones), la, index=index.to(device)).backward()
            g_critic = grads()
            block, lp = head.sample(raw_fn(t(o)), t(eps), obs=t(o))
            head.actor(q1_fn(block), q2_fn(block), lp, la).backward()
            return g_critic, grads()
        raw_of = lambda x: torch.cat([m["mu"](m["latent"](x)), m["log_std"](m["latent"](x))], 1)      # noqa: E731
        with torch.no_grad():
            a2, lp2 = sb3_sample(raw_of(t(o2)), t(eps2))
            oa2 = torch.cat([t(o2), a2], 1)
            q1n, q2n = m["q1_t"](oa2).squeeze(1), m["q2_t"](oa2).squeeze(1)
        oa = torch.cat([t(o), t(act)], 1)
        idx = index.to(device)
        loss, _ = sb3_critic_loss(m["q1"](oa).squeeze(1), m["q2"](oa).squeeze(1), q1n, q2n, lp2, t(rewards)[idx], t(dones)[idx], la[0], GAMMA)
        loss.backward()
        g_critic = grads()
        a_pi, lp = sb3_sample(raw_of(t(o)), t(eps))
        oa_pi = torch.cat([t(o), a_pi], 1)
        a_loss, e_loss = sb3_actor_losses(m["q1"](oa_pi).squeeze(1), m["q2"](oa_pi).squeeze(1), lp, la[0], TARGET_ENTROPY)
        a_loss.backward()
        e_loss.backward()
        return g_critic, grads()
    ref, eager, got = update(torch.float64, "cpu", False), update(torch.float32, "cuda", False), update(torch.float32, "cuda", True)
    out = []
    for step, r_, e_, g_ in zip(("critic_step", "actor_step"), ref, eager, got):
        for name, r, e, g in zip(names, r_, e_, g_):
            assert (r is None) == (g is None) == (e is None), (step, name)
            if r is not None:
                out.append((f"{step}.{name}", _rel(g, r), _rel(e, r)))
    assert len(out) == 12 + (8 + 12 + 1), "the critic step fills the critics, the actor step everything and log_alpha"
    return out


def test_the_head_behind_three_with_grad_networks_fills_the_parameter_grads():
    _assert_held_to_torch("end_to_end_65-64-64_n1000", end_to_end_errors())
