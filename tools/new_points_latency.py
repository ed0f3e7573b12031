#!/usr/bin/env python3
"""Latency of LocalMapping::CreateNewMapPoints' triangulation behind SearchForTriangulation on resident key frames (not imported by bench.py).
Workloads: two 1000-feature monocular key frames and two rig key frames of about 1000 + 1000 features (the BoW scenes of the resident
SearchForTriangulation tests at that size), each with the match count its scene gives.  Forms, alternating repetition by repetition in one process:
  (a) search    orbx_keyframe_search_for_triangulation[_fisheye] alone: the yardstick (its code is the parent's)
  (b) two       (a), then orbx_keyframe_triangulate_pairs[_fisheye] on the row it brought home: two launch chains, two synchronisations
  (c) fused     orbx_keyframe_search_and_triangulate[_fisheye]
Every output of every repetition -- the row, status and pos -- is compared with the search's row and tests/new_points_scene.reference_new_points on it.
Reports median (min - max) in microseconds (host clock around calls that end in a stream synchronisation), `fused_within_spread`: (c)'s median is not
above (a)'s by more than (a)'s own max - min of this run, and per-kernel times from one serialized rocprofv3 --kernel-trace --stats run of a child.
The host loop that (c) replaces is not timed here: tests/cpp/new_points_check.cpp times its C++ restatement on contiguous arrays (argument N).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

f32 = np.float32
KERNELS = ("k_new_points", "k_bow_pair_resident", "k_replay_bow_batch", "k_tri_kb8_resident", "k_replay_bow_finish_batch", "k_bow_rig_rows", "k_xfer")


def kernel_trace(out_dir, reps):
    """One serialized rocprofv3 --kernel-trace --stats run (no counters) of a child that alternates forms (a) and (c); per-kernel statistics."""
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 is not installed")
    d = Path(out_dir) / "kt"
    shutil.rmtree(d, ignore_errors=True)
    r = subprocess.run([exe, "--kernel-trace", "--stats", "-d", str(d), "-o", "kt", "--", sys.executable, str(Path(__file__).resolve()), "--trace-child",
                        "--reps", str(reps)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the traced child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    dbs = sorted(d.rglob("*.db"), key=lambda p: p.stat().st_size)
    if not dbs:
        raise RuntimeError("rocprofv3 wrote no .db")
    cur = sqlite3.connect(str(dbs[-1])).execute("select name, total_calls, total_duration, average from top_kernels")
    stats = {}
    for name, calls, total, avg in cur:
        short = name.split("(")[0].split("::")[-1].replace("void ", "")
        if short.split("<")[0] in KERNELS:
            stats[short] = {"calls": int(calls), "total_us": round(float(total), 1), "avg_us": round(float(avg), 2)}   # (the view's durations are microseconds)
    shutil.rmtree(d, ignore_errors=True)
    return stats


def workloads(ob, osa, m):
    """name -> (search(), pairs(m12), fused(), scene for the reference)."""
    import new_points_scene as S
    import test_gpu_new_points as T
    from test_gpu_frame_bow import SF, Scene
    from test_gpu_keyframe_bow import SG, _stereo_pair
    from test_gpu_keyframe_bow_fisheye import TriScene
    out = {}
    # two 1000-feature monocular key frames a pure x-translation apart
    bow = Scene(978, 1000, 8, 4)
    fx, fy, cx, cy, b = 458.654, 457.296, 367.215, 248.375, 0.11
    Kc = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    F = (np.linalg.inv(Kc).T @ np.array([[0, 0, 0], [0, 0, -b], [0, b, 0]]) @ np.linalg.inv(Kc)).astype(f32)
    eye = np.eye(3, dtype=f32)
    prm = np.array([fx, fy, cx, cy], f32)
    views = [[dict(R=eye, t=np.zeros(3, f32), Ow=np.zeros(3, f32), p=prm)], [dict(R=eye, t=np.array([-b, 0, 0], f32), Ow=np.array([b, 0, 0], f32), p=prm)]]
    a, q = _stereo_pair(ob, m, bow, 2, 1000, False)
    sc = T._adhoc_scene(False, [(a.k, len(a.d), -1, None, SF), (q.k, len(q.d), -1, None, SF)], views, 1.5 * 1.2)
    v1, v2 = m.NewPointsViews(*S.call_views(sc, "base"))      # converted once: the clock sees the calls, not the marshalling of the poses
    par = S.call_params(sc, "base")
    ep = (1e6, 1e6)
    out["monocular"] = (lambda: m.SearchForTriangulationResident(a.dev, q.dev, None, None, SG, F, ep, False, True),
                        lambda m12: m.TriangulatePairsKeyFrames(a.dev, q.dev, v1, v2, SG, SG, par["ratio_factor"], np.arange(len(m12), dtype=np.int32), m12),
                        lambda: m.SearchAndTriangulateResident(a.dev, q.dev, None, None, SG, SG, F, ep, v1, v2, par["ratio_factor"], False, True), sc,
                        (a, q, bow))
    # two rig key frames of about 1000 + 1000 features
    from test_gpu_keyframe_bow_fisheye import SF as RSF, SG as RSG
    tri = TriScene(705, 1500)
    ra, rb = tri.pair(ob, m, 2)
    rsc = T._adhoc_scene(True, [(ra.k, ra.nl, ra.n - ra.nl, None, RSF), (rb.k, rb.nl, rb.n - rb.nl, None, RSF)], T._rig_views(tri), 1.5 * 1.2)
    r1, r2 = m.NewPointsViews(*S.call_views(rsc, "base"), rig=True)
    rpar = S.call_params(rsc, "base")
    out["rig"] = (lambda: m.SearchForTriangulationResidentKB8(ra.dev, rb.dev, None, None, RSG, RSG, tri.cams, tri.cams, tri.R12, tri.t12, False),
                  lambda m12: m.TriangulatePairsKeyFramesKB8(ra.dev, rb.dev, r1, r2, RSG, RSG, rpar["ratio_factor"], np.arange(len(m12), dtype=np.int32), m12),
                  lambda: m.SearchAndTriangulateResidentKB8(ra.dev, rb.dev, None, None, RSG, RSG, tri.cams, tri.cams, tri.R12, tri.t12, r1, r2,
                                                            rpar["ratio_factor"], False), rsc, (ra, rb, tri))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    import new_points_scene as S
    import orb_slam3_amd as osa
    from oracle import oracle_binding as ob
    ob.lib()
    m = osa.ORBmatcher(0.6, True)
    res = {"tool": "new_points_latency", "reps": args.reps}
    for name, (search, pairs, fused, sc, keep) in workloads(ob, osa, m).items():
        n_matches, m12 = search()
        idx1 = np.arange(len(m12), dtype=np.int32)
        wst, wpos = S.reference_new_points(sc, "base", idx1, m12)
        ok = wst == S.OK
        res[f"{name}_features"] = [len(sc["key_frames"][0]["x"]), len(sc["key_frames"][1]["x"])]
        res[f"{name}_matches"], res[f"{name}_accepted"] = int(n_matches), int(ok.sum())

        def same(acc, pos, st):
            return acc == int(ok.sum()) and np.array_equal(st, wst) and np.array_equal(S.bits(pos[ok]), S.bits(wpos[ok]))

        def form_search():
            return search() + (None,)

        def form_two():
            n, row = search()
            return n, row, pairs(row)

        def form_fused():
            n, row, acc, pos, st = fused()
            return n, row, (acc, pos, st)

        forms = {"search": form_search, "fused": form_fused} if args.trace_child else {"search": form_search, "two": form_two, "fused": form_fused}
        times = {f: [] for f in forms}
        for rep in range(args.warmup + args.reps):
            for f, fn in forms.items():   # the forms alternate repetition by repetition
                t0 = time.perf_counter()
                n, row, tri = fn()        # (every form ends in a stream synchronisation)
                dt = time.perf_counter() - t0
                assert n == n_matches and np.array_equal(row, m12) and (tri is None or same(*tri)), (name, f, rep)
                if rep >= args.warmup:
                    times[f].append(dt * 1e6)
        if args.trace_child:
            continue
        for f, a in times.items():
            a = np.array(a)
            res[f"{name}_{f}_med_us"], res[f"{name}_{f}_min_us"], res[f"{name}_{f}_max_us"] = (round(float(np.median(a)), 1), round(float(a.min()), 1),
                                                                                              round(float(a.max()), 1))
        for f, call in (("search", search), ("fused", fused)):
            call()
            t = m.last_transfers()
            res[f"{name}_{f}_upload_bytes"], res[f"{name}_{f}_download_bytes"] = t["upload_bytes"], t["download_bytes"]
        spread = res[f"{name}_search_max_us"] - res[f"{name}_search_min_us"]
        res[f"{name}_fused_minus_search_us"] = round(res[f"{name}_fused_med_us"] - res[f"{name}_search_med_us"], 1)
        res[f"{name}_fused_within_spread"] = bool(res[f"{name}_fused_med_us"] <= res[f"{name}_search_med_us"] + spread)
        res[f"{name}_two_minus_fused_us"] = round(res[f"{name}_two_med_us"] - res[f"{name}_fused_med_us"], 1)
        del keep
    if args.trace_child:
        return
    if not args.no_trace:
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="new_points_trace_"))   # the trace's files; removed after reading
        out_dir.mkdir(parents=True, exist_ok=True)
        for k, v in kernel_trace(out_dir, 20).items():
            for field, x in v.items():
                res[f"trace_{k}_{field}"] = x
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
