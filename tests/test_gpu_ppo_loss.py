"""GPU tests of pdegym_ppo_loss / pdegym_diag_gaussian_log_prob (csrc/pdegym_ppo_loss.hip) and pde_control_gym.PPOLoss: the parts of
the head that no exp decides against the NumPy restatement (tests/ppo_loss_restatement.py) BIT FOR BIT, the real-valued parts held
to the error of the eager torch float32 composition against float64, non-finite data, a captured graph, and the head behind two
FusedMLP.with_grad networks.

Every launch of this file goes through ``_launch`` (``_launch_log_prob`` for the second entry point), which ALWAYS checks the
poisoned-buffer contract of tests/poison.py: inputs live in guarded buffers whose padding columns hold poison, outputs and the
workspace are poisoned and guarded, and after the launch every output element of rows i < N is written, the padding columns of
d_mean and all guards are untouched, every input is bit-unchanged -- and the launch is made TWICE, on two differently poisoned
workspaces, and must give the same bits.  ``policy`` displaces every buffer off its 256-byte boundary (tests/poison.py; the
policies of tests/test_gpu_pointer_alignment.py): the workspace, a buffer of 32-bit words, then starts 4, 8 or 12 bytes past one --
under "one" 4, which is no 8-byte boundary for the doubles in it."""
import math

import numpy as np
import pytest

from tests import poison
from tests import ppo_loss_restatement as R
from tests.test_gpu_pointer_alignment import POLICIES as DISPLACED
from tests.test_ppo_loss import sb3_loss

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = 256            # csrc/pdegym_ppo_loss.hip: kRows, rows per workgroup and chunk (one row per lane)
GROUPS = 256          # kMaxGroups: past ROWS * GROUPS rows a workgroup takes a second chunk
# one row; two; around a wave; one short of / exactly / one past a workgroup's rows; three workgroups, the last partial
N_LIST = (1, 2, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 5)
N_SECOND_CHUNK = ROWS * GROUPS + 1
A_LIST = (1, 2, 8)
POLICIES = (None,) + tuple(DISPLACED)
CLIP, ENT, VF = 0.2, 1e-3, 0.5
# Tolerance factor of the real-valued parts: e_kernel <= M_FACTOR * e_torch + 2^-20.  Measured on the first run of these cases
# (every pair is in profiles/r13_ppo_loss.json, "tolerance"): the worst ratio among pairs with
# e_torch >= 2^-24 is 23.2 (the last actor bias of the end-to-end case, a sum of d_mean that cancels), doubled and rounded up to a
# power of two.
M_FACTOR = 64
FLOOR = 2.0 ** -20


def _backend():
    from pdecontrolgym_amd.backend import default_backend
    return default_backend()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _index(n, rows, seed, repeated=False):
    rng = np.random.default_rng([seed, n, rows])
    if repeated:
        return rng.integers(0, max(rows // 4, 1), n).astype(np.int64)
    return rng.permutation(rows)[:n].astype(np.int64)


def _launch(case, index=None, normalize=True, values=True, pad=(0, 0, 0), policy=None, clip=CLIP, ent=ENT, vf=VF):
    """One pdegym_ppo_loss call (made twice, see the module docstring) on guarded device copies of the NumPy arrays of ``case``;
    ``pad``: extra columns of mean, actions and d_mean (row strides A + pad).  Returns the outputs as NumPy arrays."""
    n, A = case["mean"].shape
    rows = case["actions"].shape[0]
    arena = poison.Arena("cuda", policy=policy)

    def wide(name, a, extra):
        full = arena.new(name, (a.shape[0], a.shape[1] + extra), torch.float32)
        poison.poison_(full)
        full[:, :a.shape[1]].copy_(torch.from_numpy(a))
        return full

    ins = {"mean": wide("mean", case["mean"], pad[0]), "actions": wide("actions", case["actions"], pad[1])}
    for k in ("log_std", "old_log_prob", "advantages") + (("values", "returns") if values else ()):
        ins[k] = arena.like(k, torch.from_numpy(case[k]))
    if index is not None:
        assert index.min() >= 0 and index.max() < rows and index.shape == (n,)
        ins["index"] = arena.like("index", torch.from_numpy(index))
    before = {k: v.clone() for k, v in ins.items()}
    outs = {"d_mean": arena.new("d_mean", (n, A + pad[2]), torch.float32), "d_log_std": arena.new("d_log_std", (A,), torch.float32),
            "stats": arena.new("stats", (8,), torch.float32)}
    if values:
        outs["d_values"] = arena.new("d_values", (n,), torch.float32)
    bk = _backend()
    need = int(bk.lib.pdegym_ppo_loss_workspace(n, A))
    assert need > 0 and need % 4 == 0
    ws = arena.new("workspace", (need // 4,), torch.int32)
    assert ws.data_ptr() % 4 == 0
    runs = []
    for fill in (0x7FF8DEAD, -0x0123457):                   # (as doubles: a NaN pattern, then a huge negative number)
        for x in outs.values():
            poison.poison_(x)
        ws.fill_(fill)
        bk.ppo_loss(ins["mean"][:, :A], ins["log_std"], ins.get("values"), ins["actions"][:, :A], ins["old_log_prob"], ins["advantages"],
                    ins.get("returns"), outs["d_mean"][:, :A], outs.get("d_values"), outs["d_log_std"], outs["stats"], clip, ent, vf,
                    normalize, index=ins.get("index"), workspace=ws.view(torch.uint8))
        arena.check()                                        # (synchronises) no guard byte changed
        inside = torch.zeros(A + pad[2], dtype=torch.bool, device="cuda")
        inside[:A] = True
        poison.assert_written(outs["d_mean"], (slice(None), inside), "d_mean")
        poison.assert_untouched(outs["d_mean"], (slice(None), ~inside), "d_mean padding")
        for k in ("d_values", "d_log_std", "stats"):
            if k in outs:
                poison.assert_written(outs[k], None, k)
        for k, x in before.items():
            poison.assert_bits_equal(ins[k], x, None, k)
        runs.append({k: (x[:, :A] if k == "d_mean" else x).cpu().numpy().copy() for k, x in outs.items()})
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{k} depends on what the workspace held before the call"
    return runs[0]


def _launch_log_prob(case, index=None, pad=(0, 0), policy=None):
    n, A = case["mean"].shape
    arena = poison.Arena("cuda", policy=policy)
    ins = {}
    for k, extra in (("mean", pad[0]), ("actions", pad[1])):
        full = arena.new(k, (case[k].shape[0], A + extra), torch.float32)
        poison.poison_(full)
        full[:, :A].copy_(torch.from_numpy(case[k]))
        ins[k] = full
    ins["log_std"] = arena.like("log_std", torch.from_numpy(case["log_std"]))
    if index is not None:
        assert index.min() >= 0 and index.max() < case["actions"].shape[0]
        ins["index"] = arena.like("index", torch.from_numpy(index))
    before = {k: v.clone() for k, v in ins.items()}
    out = poison.poison_(arena.new("out", (n,), torch.float32))
    _backend().diag_gaussian_log_prob(ins["mean"][:, :A], ins["log_std"], ins["actions"][:, :A], out, index=ins.get("index"))
    arena.check()
    poison.assert_written(out, None, "out")
    for k, x in before.items():
        poison.assert_bits_equal(ins[k], x, None, k)
    return out.cpu().numpy()


def _args(case, values=True):
    return (case["mean"], case["log_std"], case["values"] if values else None, case["actions"], case["old_log_prob"], case["advantages"],
            case["returns"] if values else None)


def _case(n, A, seed=0, indexed=True, repeated=False):
    rows = 3 * n if indexed else n
    index = _index(n, rows, seed, repeated) if indexed else None
    return R.with_old_log_prob_near(R.seeded_case(n, A, seed=seed, rows=rows), index), index


# ---- exact parts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("A", A_LIST)
def test_value_gradient_is_exact_at_every_size(A, policy):
    """d_values = (values[i] - returns[k]) * (float)(2 vf_coef / N): one subtraction and one product per row, the restatement's bits
    at every N of the list (dense, indexed and with repeated index entries), with padded rows."""
    for n in N_LIST:
        for indexed, repeated in ((False, False), (True, False), (True, True)):
            case, index = _case(n, A, seed=n, indexed=indexed, repeated=repeated)
            got = _launch(case, index, normalize=n % 2 == 0, pad=(3, 1, 2), policy=policy)
            want = R.head_float32(*_args(case), CLIP, ENT, VF, n % 2 == 0, index=index)
            np.testing.assert_array_equal(_bits(got["d_values"]), _bits(want["d_values"]))


@pytest.mark.parametrize("n", [1, 2, 64, 256, 1024])
def test_value_loss_of_integer_values_is_exact(n):
    """Integer-valued values and returns, N a power of two, vf_coef = 0.5: every term, the sum and the mean are exact in any order."""
    case, index = _case(n, 2, seed=7)
    rng = np.random.default_rng(n)
    case["values"] = rng.integers(-40, 40, n).astype(np.float32)
    case["returns"] = rng.integers(-40, 40, case["returns"].shape[0]).astype(np.float32)
    got = _launch(case, index, vf=0.5)
    want = R.head_float32(*_args(case), CLIP, ENT, 0.5, True, index=index)
    np.testing.assert_array_equal(got["d_values"], want["d_values"])
    np.testing.assert_array_equal(got["stats"][2], want["stats"][2])
    dv = case["values"].astype(np.float64) - case["returns"][index].astype(np.float64)
    assert got["stats"][2] == (dv * dv).sum() / n and (got["d_values"] == dv / n).all()


def _margin_case(n, A, seed, normalize):
    """Ratios and advantages away from every decision of the gradient mask: about half the rows outside the clip range (a quarter on
    each side), |advantage| >= 0.5 with both signs.  The margins are asserted on the float64 restatement, never trimmed."""
    rows = 3 * n
    index = _index(n, rows, seed)
    case = R.seeded_case(n, A, seed=seed, rows=rows)
    rng = np.random.default_rng([seed, 99])
    side = rng.integers(0, 4, n)                                   # 0, 1: inside; 2: above 1 + c; 3: below 1 - c
    lr = np.where(side < 2, rng.uniform(-0.1, 0.1, n), np.where(side == 2, rng.uniform(0.25, 0.6, n), rng.uniform(-0.6, -0.3, n)))
    case["old_log_prob"][index] = (R.log_prob_float64(case["mean"], case["log_std"], case["actions"], index) - lr).astype(np.float32)
    case["advantages"] = (rng.choice([-1.0, 1.0], rows) * (0.5 + np.abs(rng.normal(0.0, 1.0, rows)))).astype(np.float32)
    ref = R.head_float64(*_args(case), CLIP, ENT, VF, normalize, index=index)
    assert np.abs(ref["ratio"] - (1 + CLIP)).min() >= 1e-3 and np.abs(ref["ratio"] - (1 - CLIP)).min() >= 1e-3
    assert np.abs(ref["adv"]).min() >= 1e-3
    if n >= ROWS - 1:
        assert (ref["ratio"] > 1 + CLIP).mean() > 0.15 and (ref["ratio"] < 1 - CLIP).mean() > 0.15
    return case, index, ref


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("A", A_LIST)
def test_zero_pattern_of_the_gradient_and_clip_fraction(A, normalize, policy):
    """Rows the clip takes out have d_mean of exactly +0 or -0, every other row is non-zero in every column; clip_fraction is the
    restatement's count.  All N of the list, and one past GROUPS x ROWS rows (a workgroup takes a second chunk) for A = 1."""
    sizes = N_LIST + ((N_SECOND_CHUNK,) if A == 1 and policy is None else ())
    for n in sizes:
        case, index, ref = _margin_case(n, A, seed=n + A, normalize=normalize)
        got = _launch(case, index, normalize=normalize, pad=(1, 2, 3), policy=policy)
        zero = ref["g"] == 0
        assert ((got["d_mean"] == 0) == zero[:, None]).all(), (n, int(((got["d_mean"] == 0) != zero[:, None]).sum()))
        np.testing.assert_array_equal(got["stats"][5], np.float32(ref["stats"][5]))
        assert n < 64 or 0.0 < got["stats"][5] < 1.0


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("A", A_LIST)
def test_one_row_probes_pin_the_gather_and_the_strides(A, policy):
    """advantages zero except at ONE buffer row, reached through index from one minibatch row, no normalisation: d_mean is non-zero
    in that row only, and there it is the float64 restatement's to float32 accuracy -- 2e-5 relative: the log-probability is rounded
    at its own magnitude (up to ~50 here, an ulp of 4e-6) before the ratio's exp -- so a wrong gather or stride moves or changes it."""
    n = ROWS + 7
    rows = 3 * n
    for i0 in (0, ROWS - 1, ROWS, n - 1):
        index = _index(n, rows, seed=i0 + 1)
        case = R.with_old_log_prob_near(R.seeded_case(n, A, seed=i0, rows=rows), index)
        k0 = int(index[i0])
        case["advantages"] = np.zeros(rows, np.float32)
        case["advantages"][k0] = 1.5
        got = _launch(case, index, normalize=False, pad=(2, 3, 1), policy=policy)
        ref = R.head_float64(*_args(case), CLIP, ENT, VF, False, index=index)
        assert ref["g"][i0] != 0, "the probe row is clipped out: the probe shows nothing"
        hit = np.zeros(n, bool)
        hit[i0] = True
        assert (got["d_mean"][~hit] == 0).all() and (got["d_mean"][hit] != 0).all()
        np.testing.assert_allclose(got["d_mean"][i0], ref["d_mean"][i0], rtol=2e-5)
        # d_log_std[j] = g (z_j^2 - 1) - ent_coef cancels where z_j^2 is near 1: the same 2e-5, of g (z_j^2 + 1) and not of the result
        z = (case["actions"][k0].astype(np.float64) - case["mean"][i0]) * np.exp(-case["log_std"].astype(np.float64))
        bound = 2e-5 * (abs(ref["g"][i0]) * (z * z + 1.0) + ENT)
        assert (np.abs(got["d_log_std"] - ref["d_log_std"]) <= bound).all(), (got["d_log_std"], ref["d_log_std"], bound)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("A", A_LIST)
def test_old_log_prob_from_the_second_entry_point_gives_a_ratio_of_exactly_one(A, policy):
    """old_log_prob filled by pdegym_diag_gaussian_log_prob from the same inputs: approx_kl == 0, clip_fraction == 0 and
    policy_loss == -mean(a) to the last bit; the log-probabilities are the float64 restatement's to float32 accuracy."""
    for n in (1, 65, ROWS + 1, 2 * ROWS + 5):
        case, index = _case(n, A, seed=n + 3)
        logp = _launch_log_prob(case, index, pad=(2, 1), policy=policy)
        np.testing.assert_allclose(logp, R.log_prob_float64(case["mean"], case["log_std"], case["actions"], index), rtol=1e-5, atol=1e-5)
        case["old_log_prob"][index] = logp
        got = _launch(case, index, normalize=False, values=False, pad=(2, 1, 0), policy=policy, ent=0.0)
        a = case["advantages"][index].astype(np.float64)
        assert got["stats"][4] == 0 and got["stats"][5] == 0
        np.testing.assert_array_equal(got["stats"][1], np.float32(-(math.fsum(a) / n)))
        np.testing.assert_array_equal(got["stats"][0], got["stats"][1])
        assert got["stats"][2] == 0 and got["stats"][6] == 0 and got["stats"][7] == 1


@pytest.mark.parametrize("A", A_LIST)
def test_dense_call_on_gathered_arrays_equals_the_indexed_call(A):
    for n in (65, 2 * ROWS + 5):
        for repeated in (False, True):
            case, index = _case(n, A, seed=n, repeated=repeated)
            a = _launch(case, index, pad=(1, 1, 1))
            dense = {k: (v[index] if k in ("actions", "old_log_prob", "advantages", "returns") else v) for k, v in case.items()}
            b = _launch(dense, None, pad=(0, 2, 0))
            for k in a:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, n, repeated)
            c = _launch(case, index, pad=(1, 1, 1))                                   # and a second call gives the same bits
            for k in a:
                assert np.array_equal(_bits(a[k]), _bits(c[k])), (k, n)


# ---- real-valued parts -------------------------------------------------------------------------------------------------------------------
def _rel(x, x64):
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    scale = np.abs(x64).max()
    return np.abs(x - x64).max() / scale if scale > 0 else (0.0 if np.abs(x - x64).max() == 0 else np.inf)


def _torch_eager(case, index, normalize, values=True):
    """The eager torch float32 composition on the device (SB3's expression under autograd, the gathers included)."""
    d = {k: torch.from_numpy(v).cuda() for k, v in case.items() if isinstance(v, np.ndarray)}
    idx = None if index is None else torch.from_numpy(index).cuda()
    g = (lambda x: x) if idx is None else (lambda x: x[idx])
    mean, log_std = d["mean"].requires_grad_(), d["log_std"].requires_grad_()
    vals = d["values"].requires_grad_() if values else None
    loss, stats = sb3_loss(mean, log_std, vals, g(d["actions"]), g(d["old_log_prob"]), g(d["advantages"]), g(d["returns"]), CLIP, ENT, VF,
                           normalize)
    loss.backward()
    out = {"d_mean": mean.grad, "d_log_std": log_std.grad, "stats": torch.stack([stats[k].detach().float().cpu() for k in R.STATS])}
    if values:
        out["d_values"] = vals.grad
    return {k: v.cpu().numpy() for k, v in out.items()}


def _errors(got, eager, ref, names):
    """[(label, e_kernel, e_torch)] per tensor and per statistic, e = max|x - x64| / max|x64|."""
    out = []
    for name in names:
        if name == "stats":
            out += [(s, _rel(got["stats"][i], ref["stats"][i]), _rel(eager["stats"][i], ref["stats"][i])) for i, s in enumerate(R.STATS)]
        else:
            out.append((name, _rel(got[name], ref[name]), _rel(eager[name], ref[name])))
    return out


def _assert_held_to_torch(what, errors):
    """e_kernel <= M_FACTOR * e_torch + 2^-20 for every pair; each is printed first (pytest -s shows them)."""
    for label, ek, et in errors:
        print(f"PPO-LOSS-RATIO {what} {label} e_kernel {ek:.3e} e_torch {et:.3e} ratio {ek / et if et > 0 else float('nan'):.3f}")
    failures = [(label, ek, et) for label, ek, et in errors if not ek <= M_FACTOR * et + FLOOR]
    assert not failures, (what, failures)


REAL_CASES = [(63, 1), (65, 2), (ROWS + 1, 8), (2 * ROWS + 5, 2), (32768, 1), (N_SECOND_CHUNK, 1)]


def real_case_errors(n, A, normalize):
    """The errors of one real-valued case against the float64 restatement on the CPU (tools/measure_ppo_loss.py records them).
    clip_fraction and the gradient mask are step functions of the ratio and of the advantage's sign: rows whose log-ratio lies
    within 1e-3 of log(1 +- c) are moved 4e-3 away when the case is made, so that a float32 rounding decides no row (the margins
    are asserted)."""
    case, index = _case(n, A, seed=n + A)
    lr = R.log_prob_float64(case["mean"], case["log_std"], case["actions"], index) - case["old_log_prob"][index].astype(np.float64)
    near = (np.abs(lr - math.log(1 + CLIP)) < 1e-3) | (np.abs(lr - math.log(1 - CLIP)) < 1e-3)
    case["old_log_prob"][index[near]] -= np.float32(4e-3)
    ref = R.head_float64(*_args(case), CLIP, ENT, VF, normalize, index=index)
    assert min(np.abs(ref["ratio"] - (1 + CLIP)).min(), np.abs(ref["ratio"] - (1 - CLIP)).min()) > 5e-4 and np.abs(ref["adv"]).min() > 1e-6
    got = _launch(case, index, normalize=normalize, pad=(1, 0, 2))
    return _errors(got, _torch_eager(case, index, normalize), ref, ("d_mean", "d_values", "d_log_std", "stats"))


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("n,A", REAL_CASES)
def test_real_valued_parts_are_as_close_to_float64_as_eager_torch(n, A, normalize):
    _assert_held_to_torch(f"n{n}_A{A}_{'norm' if normalize else 'raw'}", real_case_errors(n, A, normalize))


# ---- non-finite data ------------------------------------------------------------------------------------------------------------------------
def _nan_places(out, values=True):
    return {k: np.isnan(np.asarray(out[k], np.float64)) for k in ("d_mean", "d_log_std", "stats") + (("d_values",) if values else ())}


@pytest.mark.parametrize("A", [1, 8])
def test_non_finite_inputs_reach_what_the_restatement_says(A):
    n = ROWS + 9
    case, index = _case(n, A, seed=11)
    i_bad = ROWS + 3
    k_bad = int(index[i_bad])
    clean = _launch(case, index, normalize=False)
    assert all(np.isfinite(v).all() for v in clean.values())
    # a NaN advantage without normalisation: its row of d_mean, d_log_std and the sums that contain it
    bad = dict(case, advantages=case["advantages"].copy())
    bad["advantages"][k_bad] = np.nan
    got = _launch(bad, index, normalize=False)
    want = _nan_places(R.head_float64(*_args(bad), CLIP, ENT, VF, False, index=index))
    for k, w in want.items():
        assert np.array_equal(np.isnan(got[k]), w), k
    rows = np.zeros(n, bool)
    rows[i_bad] = True
    assert np.isnan(got["d_mean"][rows]).all() and np.isfinite(got["d_mean"][~rows]).all() and np.isfinite(got["d_values"]).all()
    assert np.array_equal(_bits(got["d_mean"][~rows]), _bits(clean["d_mean"][~rows]))
    assert np.isnan(got["stats"][[0, 1]]).all() and np.isfinite(got["stats"][[2, 3, 4, 5, 6, 7]]).all()
    # with normalisation it reaches every row
    got = _launch(bad, index, normalize=True)
    want = _nan_places(R.head_float64(*_args(bad), CLIP, ENT, VF, True, index=index))
    for k, w in want.items():
        assert np.array_equal(np.isnan(got[k]), w), k
    assert np.isnan(got["d_mean"]).all() and np.isfinite(got["d_values"]).all() and np.isnan(got["stats"][[0, 1, 6, 7]]).all()
    # a NaN return: d_values[i], value_loss and loss only
    bad = dict(case, returns=case["returns"].copy())
    bad["returns"][k_bad] = np.nan
    got = _launch(bad, index, normalize=True)
    want = _nan_places(R.head_float64(*_args(bad), CLIP, ENT, VF, True, index=index))
    for k, w in want.items():
        assert np.array_equal(np.isnan(got[k]), w), k
    assert np.isnan(got["d_values"][rows]).all() and np.isfinite(got["d_values"][~rows]).all() and np.isfinite(got["d_mean"]).all()
    assert np.isnan(got["stats"][[0, 2]]).all() and np.isfinite(got["stats"][[1, 3, 4, 5, 6, 7]]).all() and np.isfinite(got["d_log_std"]).all()


# ---- PPOLoss: graph capture, and behind two with_grad networks ---------------------------------------------------------------------------
def test_a_captured_head_replays_to_the_eager_bits():
    import pde_control_gym
    n, A = 2 * ROWS + 5, 2
    cases = [_case(n, A, seed=s) for s in (1, 2)]
    dev = {k: torch.from_numpy(v).cuda() for k, v in cases[0][0].items() if isinstance(v, np.ndarray)}
    idx = torch.from_numpy(cases[0][1]).cuda()
    head = pde_control_gym.PPOLoss(CLIP, ENT, VF, True)

    def call():
        return head(dev["mean"], dev["log_std"], dev["values"], dev["actions"], dev["old_log_prob"], dev["advantages"], dev["returns"], index=idx)
    res = call()                                             # warm-up: allocates the outputs and the workspace
    torch.cuda.synchronize()
    ptrs = (res.stats.data_ptr(), res.grad_mean.data_ptr())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = call()
    assert (res.stats.data_ptr(), res.grad_mean.data_ptr()) == ptrs
    for case, index in reversed(cases):                      # new data in the same tensors, eager first, then the replay
        for k, v in dev.items():
            v.copy_(torch.from_numpy(case[k]))
        idx.copy_(torch.from_numpy(index))
        eager = call()
        torch.cuda.synchronize()
        want = {k: getattr(eager, k).clone() for k in ("stats", "grad_mean", "grad_values", "grad_log_std")}
        for k in want:
            getattr(eager, k).zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, w in want.items():
            poison.assert_bits_equal(getattr(res, k), w, None, k)
        assert bool(torch.isfinite(res.stats).all()) and float(res.loss) == float(want["stats"][0])


def end_to_end_errors():
    """65-64-64-1 actor and critic through FusedMLP.with_grad, head(...), result.backward(): the errors of the .grad of every
    Parameter and of log_std against float64 autograd of the whole expression on the CPU, beside those of torch float32 autograd on
    the device."""
    import pde_control_gym
    from pde_control_gym import FusedMLP
    n, D, rows = 1000, 65, 3000
    torch.manual_seed(5)

    def mlp():
        return torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1))
    actor, critic = mlp(), mlp()
    log_std = torch.nn.Parameter(torch.full((1,), -0.7))
    obs = torch.randn(n, D)
    case = R.seeded_case(n, 1, seed=9, rows=rows)
    index = _index(n, rows, seed=9)
    with torch.no_grad():
        logp = torch.distributions.Normal(actor(obs), log_std.exp()).log_prob(torch.from_numpy(case["actions"][index])).sum(1)
        case["old_log_prob"][index] = (logp - 0.3 * torch.randn(n)).numpy()
    buf = {k: torch.from_numpy(case[k]) for k in ("actions", "old_log_prob", "advantages", "returns")}
    idx = torch.from_numpy(index)

    def autograd(dtype, device):
        nets = [torch.nn.Sequential(*[type(m)(m.in_features, m.out_features) if isinstance(m, torch.nn.Linear) else torch.nn.Tanh() for m in net])
                for net in (actor, critic)]
        for new, old in zip(nets, (actor, critic)):
            new.load_state_dict(old.state_dict())
            new.to(device=device, dtype=dtype)
        ls = torch.nn.Parameter(log_std.detach().to(device=device, dtype=dtype))
        b = {k: v.to(device=device, dtype=dtype) for k, v in buf.items()}
        i, o = idx.to(device), obs.to(device=device, dtype=dtype)
        loss, _ = sb3_loss(nets[0](o), ls, nets[1](o).squeeze(-1), b["actions"][i], b["old_log_prob"][i], b["advantages"][i], b["returns"][i],
                           CLIP, ENT, VF, True)
        loss.backward()
        return [p.grad.cpu().numpy() for net in nets for p in net.parameters()] + [ls.grad.cpu().numpy()]
    ref, eager = autograd(torch.float64, "cpu"), autograd(torch.float32, "cuda")
    actor.cuda()
    critic.cuda()
    log_std_d = torch.nn.Parameter(log_std.detach().cuda())
    head = pde_control_gym.PPOLoss(CLIP, ENT, VF, True)
    o = obs.cuda()
    b = {k: v.cuda() for k, v in buf.items()}
    result = head(FusedMLP(actor).with_grad(o), log_std_d, FusedMLP(critic).with_grad(o), b["actions"], b["old_log_prob"], b["advantages"],
                  b["returns"], index=idx.cuda())
    result.backward()
    params = [p for net in (actor, critic) for p in net.parameters()] + [log_std_d]
    names = [f"{w}.{i}" for w in ("actor", "critic") for i in range(6)] + ["log_std"]
    got = {k: p.grad.cpu().numpy() for k, p in zip(names, params)}
    return _errors(got, dict(zip(names, eager)), dict(zip(names, ref)), names)


def test_the_head_behind_two_with_grad_networks_fills_the_parameter_grads():
    _assert_held_to_torch("end_to_end_65-64-64-1_n1000", end_to_end_errors())
