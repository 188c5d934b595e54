"""bench.py's options: a plain run is lean (no measurement attached behind the timed steps), --full attaches them all and
the --no-* options still leave single ones out of a --full run."""
import bench


def _attached(args):
    return {"kernel_timing": not args.no_kernel_timing, "secondary": not args.no_secondary,
            "cpu_baseline": not args.no_cpu_baseline}


def test_plain_run_attaches_nothing():
    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not args.full
    assert (args.steps, args.warmup, args.gpus) == (3, 1, 1)
    assert not any(_attached(args).values())


def test_full_run_attaches_everything():
    assert all(_attached(bench.parse_args(["--full"])).values())


def test_full_run_leaves_out_what_is_asked():
    got = _attached(bench.parse_args(["--full", "--no-secondary", "--no-cpu-baseline"]))
    assert got == {"kernel_timing": True, "secondary": False, "cpu_baseline": False}
