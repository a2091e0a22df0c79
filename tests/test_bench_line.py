"""bench.py's LAST stdout line is the driver's measurement channel: it must stay small enough to be parsed (the 23 KB
line of round 4 gave BENCH_r04.json `parsed: null`).  Built here from a real full result (profiles/r04p_bench_steps20.json, the
line round 4 printed) and from a synthetic worst case -- no GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def _round4_result():
    with open(os.path.join(ROOT, "profiles", "r04p_bench_steps20.json")) as fh:
        return json.loads(fh.read().strip().splitlines()[-1])


def test_final_line_from_the_round4_result_is_small_and_complete():
    full = _round4_result()
    assert len(json.dumps(full)) > 20000                      # the line that was not parsed
    line = bench.final_line(full)
    assert "\n" not in line and len(line) < bench.MAX_LINE == 4096
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    assert d["value"] == bench._r(full["value"]) and d["config"]["workload"] == full["config"]["workload"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_step", "kernel_avg_ns", "step_event_ns",
              "counters_stale", "counters_live", "valu_wave_insts_per_step", "hbm_frac", "valu_issue_frac", "hbm_copy_measured_GBps"):
        assert k in rf, k
    assert abs(rf["frac"] - full["roofline"]["frac"]) < 1e-3 and rf["bound"] == full["roofline"]["bound"]
    assert abs(rf["step_event_ns"] - full["roofline"]["step_ms"] * 1e6) < 1.0          # the bench's own HIP-event time per step
    # `frac` can be recomputed from the line alone: wave-instructions x 2 cycles / (1024 SIMDs x 2.4 GHz x step time)
    if rf["bound"] == "valu_issue":
        again = rf["valu_wave_insts_per_step"] * 2 / (1024 * 2.4e9 * rf["step_event_ns"] * 1e-9)
        assert abs(again - rf["frac"]) < 2e-3
    cb = d["cpu_baseline"]
    assert cb["cores"] == 1 and cb["kind"] == "port" and cb["all_cores"]["logical_cpus"] == full["cpu_baseline"]["all_cores"]["logical_cpus"]
    names = [s["name"] for s in d["secondary"]]
    for must in ("ns2d_c4_b4096", "ns2d_c4_f64_b4096", "transport_c3", "ns2d_c4_f64", "ns2d_c5_f64"):
        assert must in names
    for s in d["secondary"]:
        assert set(s) == {"name", "value", "ms_per_step", "dtype", "bound", "frac"}
        assert abs(s["value"] / full["also"][s["name"]]["value"] - 1) < 1e-5
    assert "also" not in d and "timed_regions_s" not in d


def test_final_line_stays_under_the_cap_when_names_and_notes_grow():
    full = _round4_result()
    full["config"]["workload"] = "W" * 3000
    full["cpu_baseline"]["sample"] = "s" * 5000
    for k in list(full["also"]):
        full["also"][k + "_" + "x" * 200] = full["also"][k]
    line = bench.final_line(full)
    assert len(line) < bench.MAX_LINE
    d = json.loads(line)
    assert d["value"] == bench._r(full["value"]) and d["roofline"]["bound"] and d["cpu_baseline"]["value"]


def test_final_line_multi_gpu_fields_fit():
    full = _round4_result()
    full.pop("also")
    full["n_gpus"] = 8
    full["per_rank_env_steps_per_s"] = [2.0912345678e8 + i for i in range(8)]
    full["n1_equivalent"] = {"value": 2.09e8, "note": "x" * 300}
    full["process_group"] = "nccl"
    line = bench.final_line(full)
    d = json.loads(line)
    assert len(line) < bench.MAX_LINE and len(d["per_rank_env_steps_per_s"]) == 8 and d["process_group"] == "nccl"
    assert d["n1_equivalent"] == 2.09e8 and "secondary" not in d


def test_final_line_survives_an_error_in_a_secondary_workload_and_missing_counters():
    full = _round4_result()
    full["also"]["ns2d_c5_f64"] = {"error": "RuntimeError('boom')" * 20}
    full["roofline"] = {"bound": "hbm", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": None, "traffic": None, "step_ms": 0.02}
    d = json.loads(bench.final_line(full))
    assert any(s["name"] == "ns2d_c5_f64" and "error" in s for s in d["secondary"])
    assert d["roofline"]["frac"] is None and d["roofline"]["traffic"] is None


def test_hbm_probe_library_builds_and_exports_its_entry_point():
    """tools/hbm_probe.hip is built by __graft_entry__.build() into its own small library (not part of the product ABI); no GPU is
    needed to load it and find the symbol."""
    import ctypes
    from pdecontrolgym_amd import build
    lib = ctypes.CDLL(build.build_probe())
    assert hasattr(lib, "pdegym_probe_hbm")
    # ... and it does not touch the product library's fingerprint (it lives outside csrc/)
    assert not os.path.exists(os.path.join(build.CSRC, "hbm_probe.hip"))


def test_final_line_carries_live_counters_and_rocprof_kernel_average():
    """A run whose rocprofv3 children delivered counters (bench.live_counters): counters_live is true, kernel_avg_ns is rocprof's
    average of the dominant kernel (not the bench's event time) and frac follows from the line's own numbers."""
    full = _round4_result()
    live = {"collected": "rocprofv3 children", "kernel": "step1d_kernel<4, true, false, false, false, false, true>", "calls": 77,
            "kernel_avg_ns": 16335.0, "valu_insts_per_step": 11141120.0, "hbm_bytes_per_step": 14.28e6}

    class WL:
        def algorithmic_bytes_per_step(self):
            return 1267482624

        def compulsory_bytes_per_step(self):
            return 12_800_000
    rf = bench.roofline_block(WL(), "parabolic_c2", 0.018010, True, live)
    assert rf["counters_live"] is True and rf["kernel_avg_ns"] == 16335.0 and rf["traffic"] == 14.28e6 and rf["bound"] == "valu_issue"
    assert abs(rf["frac"] - 11141120.0 * 2 / (1024 * 2.4e9 * 18010e-9)) < 1e-6
    full["roofline"] = rf
    d = json.loads(bench.final_line(full))["roofline"]
    assert d["counters_live"] is True and d["kernel_avg_ns"] == 16335.0 and abs(d["step_event_ns"] - 18010.0) < 1.0
    assert abs(d["valu_wave_insts_per_step"] * 2 / (1024 * 2.4e9 * d["step_event_ns"] * 1e-9) - d["frac"]) < 2e-3
    # without live counters the committed ones serve and the line says so
    rf2 = bench.roofline_block(WL(), "parabolic_c2", 0.018010, True, None)
    assert rf2["counters_live"] is False


def test_final_line_single_env_block_and_multi_gpu_secondary():
    full = _round4_result()
    with open(os.path.join(ROOT, "profiles", "r06a_single_env_after.json")) as fh:
        full["also"]["single_env"] = json.load(fh)
    line = bench.final_line(full)
    d = json.loads(line)
    assert len(line) < bench.MAX_LINE
    se = d["single_env_us_per_step"]
    assert set(se) == {"transport_c1", "parabolic_example", "transport_s1", "ns2d_example", "traffic_example", "tumor_example"}
    for gpu, gpu_nohist, cpu in se.values():
        assert gpu > 0 and gpu_nohist > 0 and cpu > 0
    assert se["transport_c1"][0] < se["transport_c1"][2] and se["parabolic_example"][0] < se["parabolic_example"][2]
    assert d["single_env_gpu_wins_above_substeps"] > 0
    # an N > 1 run: the C5 shard workloads carry the node total and every rank's own rate
    multi = _round4_result()
    multi["n_gpus"] = 8
    multi["also"] = {n: {"value": 8e6, "ms_per_step": 0.5, "dtype": dt, "per_rank_env_steps_per_s": [1.01e6 + i for i in range(8)],
                         "instances_per_gpu": 512, "roofline": {"bound": None, "frac": None}}
                     for n, dt in (("ns2d_c5", "f32"), ("ns2d_c5_f64", "f64"))}
    line = bench.final_line(multi)
    sec = {e["name"]: e for e in json.loads(line)["secondary"]}
    assert len(line) < bench.MAX_LINE and set(sec) == {"ns2d_c5", "ns2d_c5_f64"}
    assert all(len(e["per_rank"]) == 8 and e["instances_per_gpu"] == 512 for e in sec.values())


def test_live_counters_parse_rocprof_csvs_and_fail_soft(tmp_path, monkeypatch):
    """bench.live_counters_from_csvs on synthetic rocprofv3 tables (the layout tools/summarize_profiles.py reads): per-launch averages
    of the named kernel only, the gfx950 read-side factor 2, None when a pass saw too few launches; and live_counters() itself returns
    None -- the committed counters then serve -- when the profiler child fails."""
    k = "void (anonymous namespace)::step1d_kernel<4, true, false, false, false, false, true>(pdegym_params1d, pdegym_bufs1d, int)"
    other = "void at::native::elementwise_kernel<...>(int)"
    stats = tmp_path / "p_kernel_stats.csv"
    stats.write_text('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
                     f'"{other}",5,500,100.0,1.0,90,110,1.0\n"{k}",47,752100,16002.1,99.0,15800,17000,20.0\n')

    def pmc(name, counter, values):
        f = tmp_path / f"{name}.csv"
        rows = ['"Correlation_Id","Dispatch_Id","Agent_Id","Queue_Id","Process_Id","Thread_Id","Grid_Size","Kernel_Id","Kernel_Name","Workgroup_Size","LDS_Block_Size","Scratch_Size","VGPR_Count","Accum_VGPR_Count","SGPR_Count","Counter_Name","Counter_Value","Start_Timestamp","End_Timestamp"']
        for i, v in enumerate(values):
            rows.append(f'{i},{i},1,1,1,1,1048576,3,"{k}",256,0,0,40,0,96,"{counter}",{v},0,1')
        rows.append(f'99,99,1,1,1,1,64,4,"{other}",64,0,0,8,0,16,"{counter}",123456789,0,1')
        f.write_text("\n".join(rows) + "\n")
        return str(f)
    paths = {"stats": str(stats), "SQ_INSTS_VALU": pmc("valu", "SQ_INSTS_VALU", [11141120] * 12),
             "FETCH_SIZE": pmc("fetch", "FETCH_SIZE", [4700.0] * 12), "WRITE_SIZE": pmc("write", "WRITE_SIZE", [4540.0] * 12)}
    got = bench.live_counters_from_csvs(paths, "step1d_kernel")
    assert got["kernel"].startswith("step1d_kernel<4, true") and got["calls"] == 47 and got["kernel_avg_ns"] == 16002.1
    assert got["valu_insts_per_step"] == 11141120.0
    assert got["hbm_bytes_per_step"] == 4700.0 * 2048 + 4540.0 * 1024
    assert bench.live_counters_from_csvs(dict(paths, WRITE_SIZE=pmc("few", "WRITE_SIZE", [1.0] * 3)), "step1d_kernel") is None
    assert bench.live_counters_from_csvs(paths, "no_such_kernel") is None
    # the collection itself: a failing profiler child must not take the bench run down
    import subprocess

    import sys
    real_popen = subprocess.Popen
    seen = []

    def failing_child(cmd, **kw):            # stands in for rocprofv3: exits 3 at once
        seen.append((cmd, kw))
        return real_popen([sys.executable, "-c", "import sys; sys.exit(3)"], **kw)
    monkeypatch.setattr(subprocess, "Popen", failing_child)
    monkeypatch.setattr(bench.os.path, "exists", lambda p: True)
    assert bench.live_counters("parabolic_c2") is None
    cmd, kw = seen[0]
    assert kw.get("start_new_session") is True                       # a timeout can take the whole group down
    i = cmd.index("--")
    assert cmd[i + 1] == "python3" and "--pmc" not in cmd[:i]         # the program itself directly after `--`; first pass: stats only
    assert "--no-live-counters" in cmd and "--kernel-trace" in cmd and "--sys-trace" not in cmd

    def hanging_child(cmd, **kw):            # ... and one that never finishes: killed with its group, None returned
        return real_popen([sys.executable, "-c", "import time; time.sleep(60)"], **kw)
    monkeypatch.setattr(subprocess, "Popen", hanging_child)
    t0 = bench.time.perf_counter()
    assert bench.live_counters("parabolic_c2", budget_s=7.0, first_timeout_s=1.0) is None
    assert bench.time.perf_counter() - t0 < 10
    assert bench.live_counters("ns2d_c4") is None             # only the headline has a live path


def test_dump_outputs_keeps_the_dtypes_stays_within_64_mb_and_samples_the_same_way_every_time(tmp_path):
    """--dump-outputs: float64 stays float64, everything else becomes float32; small arrays are written whole, an array that does not
    fit its share of the budget as the same seeded sample of its flattened values every time; the files stay under 64 MB in all."""
    import torch
    g = torch.Generator().manual_seed(0)
    outs = {"obs": torch.rand(4096, 257, generator=g), "reward": torch.rand(4096, generator=g),
            "terminated": torch.randint(0, 2, (4096,), dtype=torch.uint8, generator=g),
            "trajectory": torch.rand(26, 4096, 257, dtype=torch.float64, generator=g)}
    info = bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["obs.npy", "reward.npy", "terminated.npy", "trajectory.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert got["trajectory"].dtype == np.float64 and all(got[k].dtype == np.float32 for k in ("obs", "reward", "terminated"))
    np.testing.assert_array_equal(got["obs"], outs["obs"].numpy())
    np.testing.assert_array_equal(got["terminated"], outs["terminated"].numpy().astype(np.float32))
    assert info["trajectory"][0] == [26, 4096, 257] and 0 < got["trajectory"].size == info["trajectory"][1] < outs["trajectory"].numel()
    assert np.isin(got["trajectory"], outs["trajectory"].numpy().reshape(-1)).all()
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_times_exactly_k_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    """A plain run: the headline line only (no CPU baseline, no secondary workloads, no live counters), ONE timed region of exactly
    --steps steps, and --dump-outputs writes the last step's observations / rewards / flags -- identical in two separate runs."""
    lines = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5",
                            "--dump-outputs", str(tmp_path / tag)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for d in lines:
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 30 and d["warmup"] == 5 and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert "cpu_baseline" not in d and "secondary" not in d and d["roofline"]["counters_live"] is False
        assert d["config"]["launch"].startswith("hipGraph")         # the dump must not push the run off the captured path
    with open(os.path.join(ROOT, "bench_parabolic_c2.json")) as fh:      # written by the second run: compared with its own line
        full = json.load(fh)
    d = lines[1]
    assert len(full["timed_regions_s"]) == 1
    assert abs(d["ms_per_step"] - full["timed_regions_s"][0] / 30 * 1e3) <= 2e-5 * d["ms_per_step"]       # (6 digits in the line)
    assert abs(d["value"] - 4096 * 30 / full["timed_regions_s"][0]) <= 2e-5 * d["value"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["obs.npy", "reward.npy", "terminated.npy", "truncated.npy"]
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert obs.shape == (4096, 257) and obs.dtype == np.float32 and np.isfinite(obs).all()
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
