"""What a bench.py invocation runs (no GPU): a plain ``--gpus 1 --steps N --warmup W`` run times its N steps once and runs
nothing else; ``--full`` adds the per-kernel timing, the configs[2] leg, the CPU baselines / parity checks and the repeated
timed regions, each of which its ``--no-*`` option drops again."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench


def test_plain_run_times_its_steps_and_nothing_else():
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.gpus, args.steps, args.warmup, args.full) == (1, 7, 2, False)
    assert bench.run_plan(args) == {"kernel_timing": False, "configs2": False, "cpu_baseline": False, "repeat_regions": 1}
    # the legs' own switch-offs change nothing in a plain run
    args = bench.parse(["--no-cpu-baseline", "--no-kernel-timing", "--no-configs2"])
    assert bench.run_plan(args) == {"kernel_timing": False, "configs2": False, "cpu_baseline": False, "repeat_regions": 1}
    assert (args.steps, args.warmup, args.host_input) == (10, 3, False)          # the contract's defaults


def test_full_run_adds_every_leg_and_each_can_be_dropped():
    assert bench.run_plan(bench.parse(["--full"])) == {"kernel_timing": True, "configs2": True, "cpu_baseline": True,
                                                       "repeat_regions": 3}
    plan = bench.run_plan(bench.parse(["--full", "--no-cpu-baseline", "--no-configs2"]))
    assert plan == {"kernel_timing": True, "configs2": False, "cpu_baseline": False, "repeat_regions": 3}
    assert not bench.run_plan(bench.parse(["--full", "--no-kernel-timing"]))["kernel_timing"]


def test_explicit_repeat_regions_hold_in_either_mode():
    assert bench.run_plan(bench.parse(["--repeat-regions", "2"]))["repeat_regions"] == 2
    assert bench.run_plan(bench.parse(["--full", "--repeat-regions", "1"]))["repeat_regions"] == 1
