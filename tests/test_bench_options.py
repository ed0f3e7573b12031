"""CPU tests: what a plain bench.py run does against one with --full (option defaults), and the threaded frame synthesis."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402

EXTRAS = ("cpu_frames", "verify", "repeat", "latency", "profile", "pmc", "other_workloads")


def extras(argv):
    a = bench.parse_args(argv)
    return {k: getattr(a, k) for k in EXTRAS}


def test_plain_run_skips_everything_beyond_the_headline():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and (a.steps, a.warmup, a.settle, a.input_sets) == (20, 5, 8, 3)
    assert extras([]) == {"cpu_frames": 0, "verify": 0, "repeat": 1, "latency": 0, "profile": False, "pmc": False, "other_workloads": False}


def test_full_run_has_every_part():
    assert extras(["--full"]) == {"cpu_frames": 384, "verify": 4, "repeat": 5, "latency": 200, "profile": True, "pmc": True, "other_workloads": True}
    assert not extras(["--full", "--workload", "kitti"])["other_workloads"]
    assert not extras(["--full", "--cpu-frames", "0"])["other_workloads"]
    assert not extras(["--full", "--no-profile"])["other_workloads"]


def test_an_explicit_option_holds_with_or_without_full():
    assert extras(["--verify", "2", "--repeat", "3", "--profile"])["verify"] == 2
    assert extras(["--repeat", "3", "--profile"])["profile"] is True and extras(["--repeat", "3"])["repeat"] == 3
    e = extras(["--full", "--verify", "0", "--repeat", "1", "--latency", "0", "--no-pmc", "--no-other-workloads"])
    assert (e["verify"], e["repeat"], e["latency"], e["pmc"], e["other_workloads"]) == (0, 1, 0, False, False)


def test_other_workload_children_run_with_full(monkeypatch):
    seen = []

    class Done:
        returncode, stdout, stderr = 1, "", "stub"

    monkeypatch.setattr(bench.subprocess, "run", lambda cmd, **k: seen.append(cmd) or Done())
    r = bench.other_workload_child("kitti", bench.parse_args(["--full", "--steps", "7", "--warmup", "2"]))
    assert "error" in r and "--full" in seen[0] and seen[0][seen[0].index("--steps") + 1] == "7"


def test_synth_frames_equal_a_loop():
    from orb_slam3_amd import synth
    canvas = synth.make_canvas(3, size=256, n_shapes=50)
    make = lambda t: synth.frame_from_canvas(canvas, t, 64, 48, 1000 + t)  # noqa: E731
    got = bench.synth_frames(make, 9)
    assert len(got) == 9 and all(np.array_equal(g, make(t)) for t, g in enumerate(got))
