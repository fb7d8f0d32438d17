"""bench.py's command line, without a GPU: `--full` exists and is off by default, so a plain run is the lean one; the
options that only steer what `--full` adds are still accepted without it (the profiling scripts pass them)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_full_is_an_option_and_off_by_default():
    import bench
    ap = bench.make_parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and (plain.gpus, plain.steps, plain.warmup) == (1, 20, 5)
    assert plain.dump_outputs is None and plain.actors == 4096 and plain.history == 2000 and plain.groups == 1
    full = ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full is True
    assert {k: v for k, v in vars(full).items() if k != "full"} == {k: v for k, v in vars(plain).items() if k != "full"}


def test_cpu_baseline_options_are_accepted_without_full():
    import bench
    a = bench.make_parser().parse_args(["--no-cpu-baseline", "--cpu-seconds", "4", "--cpu-threads", "2"])
    assert a.full is False and a.no_cpu_baseline is True and a.cpu_seconds == 4.0 and a.cpu_threads == 2
