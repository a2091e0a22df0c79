"""Inputs shared by tests/test_terminal_obs.py (CPU, fake backend) and tests/test_gpu_terminal_obs.py: 1D environments whose
episodes end INSIDE a short rollout window for both reasons.  The horizon is 3 env-steps, so with T = 7 every instance that is not cut
off terminates twice; ``max_state_value`` sits between the initial row norms of two groups of pool rows (the way
tests/test_gpu_1d.py: test_norm_reward_epilogues_match_oracle does it), so the rows of the large group are cut off
(``truncated and not terminated``) at the first step of each of their episodes."""
import numpy as np

HORIZON, T_STEPS = 3, 7
KINDS = {"parabolic": "PDEControlGym-ReactionDiffusionPDE1D", "transport": "PDEControlGym-TransportPDE1D"}


def nodes(kind, nx):
    return nx + 1 if kind == "parabolic" else nx


def env_params(kind, nx, S=3, control_type="Dirchilet", sensing_loc="full", sensing_type=None, small=1.0):
    """The parameter dictionary of ``make_vec``.  Pool row i is the constant row c_i: c_i in [8, 9] when i % 3 == 0 (norm above
    ``max_state_value`` = 4 sqrt(n): cut off), c_i in ``small`` * [1, 2] otherwise (norm well below it for the 3 steps of an episode;
    the Neumann-actuated rows grow about 2.5-fold per env-step on these grids and start from ``small`` = 0.1)."""
    from pde_control_gym.src import TunedReward1D
    n = nodes(kind, nx)
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
    beta = np.full(n, 3.0 if kind == "parabolic" else 0.5, np.float32)

    def rows(idx, nx_):
        idx = np.asarray(idx)
        c = np.where(idx % 3 == 0, 8.0, small) + np.where(idx % 3 == 0, 1.0, small) * np.random.default_rng(11).uniform(0, 1, 4096)[idx % 4096]
        return (c[:, None] * np.ones((1, n))).astype(np.float32), np.tile(beta, (len(idx), 1))

    return {"T": HORIZON * S * dt, "dt": dt, "X": 1, "dx": dx, "reward_class": TunedReward1D(HORIZON * S, -1e3, 3e2), "normalize": True,
            "sensing_loc": sensing_loc, "control_type": control_type, "sensing_type": sensing_type, "sensing_noise_func": None,
            "limit_pde_state_size": True, "max_state_value": 4.0 * float(np.sqrt(n)), "max_control_value": 5,
            "control_sample_rate": S * dt, "batched_reset_func": rows}


def make_1d(kind, nx, B, auto_reset=True, beta_pool=None, **kw):
    """A reset 1D vector environment of B instances (``kw``: ``device`` / ``backend`` and overrides of ``env_params``);
    ``beta_pool=False`` keeps beta fixed over the restarts (a controller with one shared gain row)."""
    import pde_control_gym
    over = {k: kw.pop(k) for k in ("S", "control_type", "sensing_loc", "sensing_type", "small") if k in kw}
    extra = {k: kw.pop(k) for k in ("sensing_noise_tensor_func",) if k in kw}
    venv = pde_control_gym.make_vec(KINDS[kind], num_envs=B, **{**env_params(kind, nx, **over), **extra}, **kw)
    venv.reset_tensor()
    if auto_reset:
        venv.enable_fused_auto_reset(beta_pool=beta_pool)
    return venv


TRAFFIC_BASE = dict(T=1.0, dt=0.5, X=220, dx=20, v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60)
TRAFFIC_RS = (0.12, 0.155, 0.12, 0.125, 0.155)                    # 0.155 * 1.1 (the profile's crest) > ro_max: cut off at once
TRAFFIC_POOL = TRAFFIC_RS + TRAFFIC_RS      # (row (b + k B) mod 10 is instance b's own density: a backstepping law's weights stay valid)


def make_traffic(sim, B=5, **kw):
    """TrafficPDE1D on M = 12 nodes whose clock reaches T / dt = 2 at the fourth step (terminated) and whose instances 1 and 4 start
    -- and restart -- above ``ro_max`` (truncated and not terminated at every step)."""
    import random
    import pde_control_gym
    from pde_control_gym.src import TrafficARZReward
    random.seed(0)
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, reward_class=TrafficARZReward(), simulation_type=sim,
                                    limit_pde_state_size=True, control_freq=1, **TRAFFIC_BASE, **kw)
    venv.reset_tensor()
    rs = np.asarray(TRAFFIC_RS[:B], dtype=np.float64)
    venv.core.set_action_bounds(rs * venv.core.Veq(rs))
    venv.core.reset(rs)
    venv.enable_fused_auto_reset(init_pool=np.asarray(TRAFFIC_POOL))
    assert venv.core.M == 12
    return venv


def traffic_commands(T, B, A, seed=1):
    return np.random.default_rng(seed).uniform(1.0, 1.4, (T, B, A))


def make_tumor(B=5, fused=True, **kw):
    """BrainTumor1D on nx = 21 nodes, TherapyWrapper steps, with the detection and death radii (8 and 12) inside so short a domain and
    280 days: with the doses of ``tumor_commands`` patients 2, 3 and 4 use up their dosage within the window and their post-therapy
    run ends the episode -- patient 2's at the time limit (terminated), the others' at the death radius (truncated and not
    terminated).  Patients are identical but for their commands: a policy, which gives them all the same doses, ends them all the
    same way."""
    import pde_control_gym
    from pde_control_gym.src import BrainTumorReward
    from tests.test_tumor import KW, tumor_ic
    venv = pde_control_gym.make_vec("PDEControlGym-BrainTumor1D", num_envs=B, weekends=False, fused_step=fused, T=280,
                                    reward_class=BrainTumorReward(), reset_init_condition_func=tumor_ic,
                                    **{**KW, "X": 20, "t1_detection_radius": 8, "t1_death_radius": 12}, **kw)
    assert venv.core.nx == 21
    venv.benchmark()
    venv.reset_tensor()
    return venv


def tumor_commands(T, B, seed=5):
    return np.random.default_rng(seed).uniform(0.2, 1, (T, B)) * np.linspace(0.03, 0.9, B)[None]


# The environments of the one-launch 1D cases of tests/test_gpu_terminal_obs.py: id -> (kind, nx, overrides of env_params).  The CPU
# suite steps each of them on the oracle (tests/test_terminal_obs.py) and checks that the inputs hold a termination and a cut-off.
GPU_ENVS_1D = {
    "parabolic_n65_full": ("parabolic", 64, {}),
    "parabolic_n40": ("parabolic", 39, {}),
    "parabolic_n257": ("parabolic", 256, {}),
    "transport_n64": ("transport", 64, {}),
    "neumann": ("parabolic", 39, dict(control_type="Neumann", small=0.1)),
    "scalar_sensing": ("transport", 40, dict(sensing_loc="opposite", sensing_type="Dirchilet")),
    "parabolic_n33": ("parabolic", 32, {}),
}
B_GPU = 5      # a partial workgroup


def commands(T, B, seed=2):
    return np.random.default_rng(seed).uniform(-1, 1, (T, B)).astype(np.float32)
