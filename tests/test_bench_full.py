"""bench.py --full: a plain run measures the headline figure alone and is short; the rooflines, the extras, the comparison with
the oracle and the CPU baseline run with --full only (--no-extras / --no-cpu-baseline take parts out of a --full run)."""
import importlib.util
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# keys of the line that only a --full run fills in
FULL_ONLY = ("roofline", "roofline_headline", "roofline_solve", "roofline_outer_loop", "cpu_baseline", "max_coeff_err_vs_cpu_ref",
             "max_coeff_err_vs_113bit_ref", "in_flight_slots_vs_cpu_ref", "config3_strong_scaling", "one_batch_in_flight",
             "value_200_steps")
# a plain run may spend this long outside its warm-up and timed steps: whole process, start to exit, less (K + W) x ms_per_step
PLAIN_OVERHEAD_LIMIT_S = 30.0


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), capture_output=True, text=True, env=env,
                       timeout=600)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1
    return json.loads(lines[0]), wall


def test_full_is_an_option_and_off_by_default():
    bench = _bench()
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"]).full is False
    args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert args.full is True and (args.gpus, args.steps, args.warmup) == (1, 20, 5)
    # the flags that take parts out of a --full run are still there
    args = bench.parse_args(["--full", "--no-extras", "--no-cpu-baseline"])
    assert args.full and args.no_extras and args.no_cpu_baseline


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_short():
    """`bench.py --gpus 1 --steps 20 --warmup 5`: the headline keys as ever, nothing of what --full measures, and at most 30 s of
    the process's life outside its 25 steps (import, set-up, first-launch costs, clock ramp and stream calibration included)."""
    line, wall = _run("--gpus", "1", "--steps", "20", "--warmup", "5")
    assert line["metric"] == "trajectories/sec (batch of N-seg min-snap paths)" and line["unit"] == "trajectories/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 20 and line["warmup"] == 5 and line["regions"] == 9 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1024 * 1e3 / line["ms_per_step"], rel=1e-9)
    for key in FULL_ONLY:
        assert line[key] is None, key
    assert line["extras"] == {} and line["dump_outputs"] is None
    assert line["config"]["issue_policy"]["stream_pair"]["candidates"] == 8   # (the calibration belongs to the headline)
    overhead = wall - (20 + 5) * line["ms_per_step"] * 1e-3
    print("plain run: %.1f s from start to exit, %.1f s outside its steps" % (wall, overhead))
    assert overhead <= PLAIN_OVERHEAD_LIMIT_S, overhead


@pytest.mark.gpu
def test_full_run_measures_what_a_plain_run_leaves_out():
    """--full on a small batch (a short CPU sample): every key a plain run leaves null is filled in, and the headline keys mean
    what they mean in a plain run."""
    line, _ = _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--config3-paths", "4096", "--cpu-seconds", "0.5")
    assert line["unit"] == "trajectories/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(1024 * 1e3 / line["ms_per_step"], rel=1e-9)
    for key in FULL_ONLY:
        assert line[key] is not None, key
    assert line["roofline"]["frac"] > 0 and line["roofline_headline"]["in_timed_region"] is True
    assert line["roofline_solve"]["achieved"] > 0 and line["roofline_outer_loop"]["avg_launch_us"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["value_all_cores"] > 0
    # (the bounds of tests/test_gpu_headline_kernel.py on the same 20 480 paths: 1e-6 against the double oracle, whose own error
    # on the short-segment paths that is, 1e-7 against its 113-bit route)
    assert line["max_coeff_err_vs_cpu_ref"] < 1e-6 and line["max_coeff_err_vs_113bit_ref"]["max"] < 1e-7
    slots = line["in_flight_slots_vs_cpu_ref"]
    assert slots["slots"] == 20 and slots["every_status_success"] is True
    assert slots["max_coeff_err_vs_cpu_ref"] < 1e-6 and slots["max_coeff_err_vs_113bit_ref"] < 1e-7
    for key in ("roofline_large", "host_buffer_call", "single_request_latency", "materialized_blocks_step", "streams_in_flight",
                "one_batch_in_flight", "nonlinear", "config3", "roofline_solve_saturated", "policy_layer",
                "nonlinear_min_acceleration"):
        assert key in line["extras"], key
    assert "error" not in line["extras"]["policy_layer"] and "error" not in line["extras"]["nonlinear_min_acceleration"]
    assert line["extras"]["config3"]["paths_per_rank"] == 4096 and line["config3_strong_scaling"]["value"] > 0
