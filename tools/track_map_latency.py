#!/usr/bin/env python3
"""Latency of the Tracking searches that run from map ids against the flat handle forms fed by a host projection (not imported by bench.py).
Workloads (tests/track_scene.py at the workload's shapes, monocular / rectified frames), each timed on the same inputs:
  * track_last_frame  TrackWithMotionModel's SearchByProjection(Cur, Last, th, bMono): 1000-feature frames, about 600 tracked points;
  * keyframe          Relocalization's SearchByProjection(Cur, pKF, sAlreadyFound, th, ORBdist): a 1000-feature key frame, about 400 points;
  * rig_track_last_frame / rig_keyframe  the same two on a 1000 + 1000 fisheye-stereo rig (a 2000-feature source rig, about 1200 / 800 points);
                      the host projection there calls the oracle's KannalaBrandt8::project point by point through ctypes and is NOT a stand-in for
                      anything: only `flat`, `map` and the upload bytes of the rig workloads mean something.
Per workload two paths alternate repetition by repetition in one process:
  flat  the host projection (track_scene's float32 numpy gates and query records -- a stand-in for the adapters' C++ loops, timed on its own as
        `host_projection`) followed by orbx_frame_search_by_projection_frame / _window on the resident frame; `flat` is the call, `flat_sum` both;
  map   orbx_frame_track_last_frame_map / orbx_frame_search_by_projection_keyframe_map.
Every output of every repetition is compared with a reference composed from the CPU oracle once.  Reports median (min - max) in microseconds over
--reps repetitions (host clock around calls that end in a stream synchronisation) and the upload the calls count themselves.  Prints one JSON line
(and writes it to --out)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

f32 = np.float32


def table(osa, m, sc, TS):
    M = osa.DeviceMap(TS.CAPACITY)
    have = sc["ids"] >= 0
    M.update(m, sc["ids"][have], **{k: np.ascontiguousarray(v[have]) for k, v in sc["map_points"].items()})
    return M


def mapped(cm, sel):
    return np.where(cm >= 0, sel[np.maximum(cm, 0)], cm).astype(np.int32)


def stats(a):
    a = np.array(a)
    return {"med_us": round(float(np.median(a)), 1), "min_us": round(float(a.min()), 1), "max_us": round(float(a.max()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import orb_slam3_amd as osa
    import track_scene as TS
    from oracle import oracle_binding as ob

    m = osa.ORBmatcher(0.9, True)
    res = {"tool": "track_map_latency", "reps": args.reps}
    for name, p_none in (("track_last_frame", 0.4), ("keyframe", 0.6)):
        sc = TS.make_scene(21, n_src=1000, n_cur=1000, p_none=p_none)
        ids, cur, n = sc["ids"], sc["cur"], len(sc["ids"])
        res[f"{name}_points"] = int((ids >= 0).sum())
        M = table(osa, m, sc, TS)
        view = lambda k, d, ur=None: osa.FrameView(k, d, *TS.BOUNDS, sc["scale_factors"], ur)   # noqa: E731
        F = osa.DeviceFrame(m, len(cur["kps"])).load(view(cur["kps"], cur["desc"], cur["u_right"] if name == "track_last_frame" else None))
        src = view(sc["src_kps"], np.zeros((n, 32), np.uint8))
        if name == "track_last_frame":
            ref = TS.reference_m2(ob, sc, 7.0, 0, True, True, ids, sc["has_obs"], sc["occupied"])
            last = osa.DeviceFrame(m, n).load(src)
            project = lambda: TS.queries_m2(sc, ids, sc["has_obs"])                                                           # noqa: E731
            flat = lambda sel, q: m.SearchByProjectionFrame(F, q, 7.0, 0, sc["occupied"], raw=True)                           # noqa: E731
            new = lambda: m.TrackLastFrame(F, last, sc["cam"], sc["pose"], M, ids, 7.0, 0, sc["has_obs"], sc["occupied"], True, True)   # noqa: E731
        else:
            ref = TS.reference_m3(ob, sc, 10.0, 100.0, True, ids, sc["occupied"])
            last = osa.DeviceKeyFrame.from_host(m, src)
            project = lambda: TS.queries_m3(sc, 10.0, ids)                                                                    # noqa: E731
            flat = lambda sel, q: m.SearchByProjectionWindow(F, q, 100.0, True, sc["occupied"], raw=True)                     # noqa: E731
            new = lambda: m.SearchByProjectionKeyFrame(F, last, sc["cam"], sc["pose"], sc["log_scale_factor"], M, ids, 10.0, 100.0, True,   # noqa: E731
                                                       sc["occupied"], True, True)
        on = ref["projected"] == 1
        times = {"host_projection": [], "flat": [], "flat_sum": [], "map": []}
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            sel, q = project()
            t1 = time.perf_counter()
            nm, cm = flat(sel, q)
            t2 = time.perf_counter()
            assert nm == ref["nm"] and np.array_equal(np.maximum(mapped(cm, sel), -1), ref["match"]), (name, "flat", rep)
            t3 = time.perf_counter()
            gm, gmatch, gpr, (gu, gv) = new()
            t4 = time.perf_counter()
            assert gm == ref["nm"] and np.array_equal(gmatch, mapped(cm, sel)) and np.array_equal(gpr, ref["projected"]), (name, "map", rep)
            assert np.array_equal(gu.view(np.uint32)[on], ref["u"].view(np.uint32)[on]) and np.array_equal(gv.view(np.uint32)[on], ref["v"].view(np.uint32)[on])
            if rep >= args.warmup:
                times["host_projection"].append((t1 - t0) * 1e6); times["flat"].append((t2 - t1) * 1e6)
                times["flat_sum"].append((t2 - t0) * 1e6); times["map"].append((t4 - t3) * 1e6)
        for f, a in times.items():
            for key, v in stats(a).items():
                res[f"{name}_{f}_{key}"] = v
        sel, q = project()
        flat(sel, q)
        res[f"{name}_flat_upload_bytes"] = m.last_transfers()["upload_bytes"]
        res[f"{name}_flat_queries"] = int(len(sel))
        new()
        res[f"{name}_map_upload_bytes"] = m.last_transfers()["upload_bytes"]
        res[f"{name}_matches"] = int(ref["nm"])
        res[f"{name}_map_over_flat"] = round(res[f"{name}_map_med_us"] / res[f"{name}_flat_med_us"], 3)
        res[f"{name}_map_over_flat_sum"] = round(res[f"{name}_map_med_us"] / res[f"{name}_flat_sum_med_us"], 3)
        del F, last, M
    for name, p_none in (("rig_track_last_frame", 0.4), ("rig_keyframe", 0.6)):
        sc = TS.make_rig_scene(ob, 22, n_src=2000, n_left_src=1000, n_side=1000, p_none=p_none)
        ids, cur, n = sc["ids"], sc["cur"], len(sc["ids"])
        res[f"{name}_points"] = int((ids >= 0).sum())
        M = table(osa, m, sc, TS)
        view = lambda k, d: osa.FrameView(k, d, *TS.RIG_BOUNDS, sc["scale_factors"])   # noqa: E731
        none = lambda k: np.full(len(k), -1, np.int32)                                  # noqa: E731
        F = osa.DeviceFrame(m, len(cur["desc"])).load_fisheye(view(cur["kps_left"], cur["desc"]), cur["kps_right"], cur["l2r"], cur["r2l"])
        skl, skr = sc["src_kps"][:sc["n_left_src"]], sc["src_kps"][sc["n_left_src"]:]
        src = view(skl, np.zeros((n, 32), np.uint8))
        if name == "rig_track_last_frame":
            ref = TS.rig_reference_m2(ob, sc, 7.0, 0, True, ids, sc["has_obs"], sc["occupied"])
            last = osa.DeviceFrame(m, n).load_fisheye(src, skr, none(skl), none(skr))
            flat = lambda q: m.SearchByProjectionFrameFisheye(F, None, q, 7.0, 0, sc["occupied"], raw=True)                       # noqa: E731
            new = lambda: m.TrackLastFrameFisheye(F, last, sc["view"], sc["Trl"], M, ids, 7.0, 0, sc["has_obs"], sc["occupied"], True, True)   # noqa: E731
        else:
            ref = TS.rig_reference_m3(ob, sc, 10.0, 100.0, True, ids, sc["occupied"])
            last = osa.DeviceKeyFrame.from_host_fisheye(m, src, skr)
            flat = lambda q: m.SearchByProjectionWindowFisheye(F, q, 100.0, True, sc["occupied"], raw=True)                       # noqa: E731
            new = lambda: m.SearchByProjectionKeyFrameFisheye(F, last, sc["view"], sc["log_scale_factor"], M, ids, 10.0, 100.0, True,   # noqa: E731
                                                              sc["occupied"], True, True)
        sel, q, on = ref["sel"], ref["q"], ref["projected"] == 1
        times = {"flat": [], "map": []}
        for rep in range(args.warmup + args.reps):
            t1 = time.perf_counter()
            nm, cm = flat(q)
            t2 = time.perf_counter()
            assert nm == ref["nm"] and np.array_equal(np.maximum(mapped(cm, sel), -1), ref["match"]), (name, "flat", rep)
            t3 = time.perf_counter()
            gm, gmatch, gpr, (gu, gv) = new()
            t4 = time.perf_counter()
            assert gm == ref["nm"] and np.array_equal(gmatch, mapped(cm, sel)) and np.array_equal(gpr, ref["projected"]), (name, "map", rep)
            assert np.array_equal(gu.view(np.uint32)[on], ref["u"].view(np.uint32)[on]) and np.array_equal(gv.view(np.uint32)[on], ref["v"].view(np.uint32)[on])
            if rep >= args.warmup:
                times["flat"].append((t2 - t1) * 1e6); times["map"].append((t4 - t3) * 1e6)
        for f, a in times.items():
            for key, v in stats(a).items():
                res[f"{name}_{f}_{key}"] = v
        flat(q)
        res[f"{name}_flat_upload_bytes"] = m.last_transfers()["upload_bytes"]
        res[f"{name}_flat_queries"] = int(len(sel))
        new()
        res[f"{name}_map_upload_bytes"] = m.last_transfers()["upload_bytes"]
        res[f"{name}_matches"] = int(ref["nm"])
        res[f"{name}_map_over_flat"] = round(res[f"{name}_map_med_us"] / res[f"{name}_flat_med_us"], 3)
        del F, last, M
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
