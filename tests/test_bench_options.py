"""bench.py's plain run against --full (which legs each one runs) and the --dump-outputs writer, on the CPU: no GPU library is
loaded by either."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from sparsebench_amd.bench import outputs  # noqa: E402


def _args(argv):
    a = bench.parser().parse_args(argv)
    bench.plain_or_full(a)
    return a


def test_a_plain_run_runs_only_the_headline_loop():
    a = _args(["--gpus", "1", "--steps", "50", "--warmup", "5"])
    assert not a.full and a.loops == "reference" and a.passes == {"clean"}
    assert a.no_preflight and a.no_rccl_leg and a.no_push_inside_leg and a.preflight_skipped
    assert a.dump_outputs is None and a.sustained_steps == 4800  # (the settling warm-up stays; its figure is --full's)


def test_full_keeps_every_leg():
    a = _args(["--full", "--steps", "50"])
    assert a.full and a.loops == "both" and a.passes == {"clean", "events", "phases"}
    assert not a.no_preflight and not a.no_rccl_leg and not a.no_push_inside_leg and a.preflight_skipped is None
    a = _args(["--full", "--no-preflight", "--loops", "structure", "--passes", "clean,events"])
    assert a.no_preflight and a.preflight_skipped == "--no-preflight" and a.loops == "structure" and a.passes == {"clean", "events"}


def test_explicit_options_apply_to_a_plain_run_too():
    a = _args(["--loops", "both", "--passes", "clean,events", "--dump-outputs", "d"])
    assert not a.full and a.loops == "both" and a.passes == {"clean", "events"} and a.dump_outputs == "d"


def test_dump_is_float64_and_whole_when_it_fits(tmp_path):
    x = np.linspace(0.0, 1.0, 2 * 128 ** 3 // 2)
    files = outputs.write(str(tmp_path), {"x": x, "rr_history": np.arange(5.0), "pAp_history": np.arange(4.0)})
    assert sorted(os.path.basename(f) for f in files) == ["pAp_history.npy", "rr_history.npy", "x.npy"]
    got = np.load(str(tmp_path / "x.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, x)


def test_dump_of_a_large_output_is_a_fixed_sample_under_64_mb(tmp_path):
    x = np.arange(12_000_000, dtype=np.float64) * 0.5  # 96 MB
    a, b = tmp_path / "a", tmp_path / "b"
    fa = outputs.write(str(a), {"x": x, "rr_history": np.arange(7.0)}, "_rank1")
    outputs.write(str(b), {"x": x, "rr_history": np.arange(7.0)}, "_rank1")
    assert sum(os.path.getsize(f) for f in fa) <= 64 << 20
    assert sorted(os.path.basename(f) for f in fa) == ["rr_history_rank1.npy", "x_rank1.npy", "x_sample_index_rank1.npy"]
    idx, val = np.load(str(a / "x_sample_index_rank1.npy")), np.load(str(a / "x_rank1.npy"))
    assert idx.dtype == val.dtype == np.float64 and np.array_equal(val, x[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
    for name in ("x_rank1.npy", "x_sample_index_rank1.npy", "rr_history_rank1.npy"):  # the same sample every time
        assert np.array_equal(np.load(str(a / name)), np.load(str(b / name)))
