#!/usr/bin/env python3
"""Latency of the one-call searches with their map points resident (orbx_map) against the flat forms that upload them (not imported by bench.py).
Workloads, each timed flat / `_map` on the same inputs:
  * local_points  Tracking::SearchLocalPoints: 10 000 resident points, a 1000-feature frame;
  * fuse          LocalMapping::SearchInNeighbors' Fuse: 1000 points into 20 key frames;
  * sim3          LoopClosing's SearchByProjection(pKF, Scw, ...): 1000 points against 8 key frames;
  * pair          the LocalMapping pair: ComputeDistinctiveDescriptors of 1000 map points, then the Fuse above with the new descriptors --
                  flat: orbx_keyframe_distinctive_descriptors, the rows come down and go up again with the search;
                  map:  orbx_keyframe_distinctive_descriptors_to_map, then the `_map` search;
and, alone, update_300: orbx_map_update of 300 points -- the call as it returns (it does not wait) and the call followed by a one-slot read, which
synchronises.
The forms alternate repetition by repetition in one process; every output of every repetition is compared with a reference composed from the CPU
oracle once (tests/test_gpu_frame_handle.py, tests/test_gpu_keyframe.py, tests/sim3_scene.py).  Reports median (min - max) in microseconds over
--reps repetitions (host clock around calls that end in a stream synchronisation) and, per workload, `within_spread`: the `_map` median is not
above the flat median by more than the flat form's own max - min of this run.  Prints one JSON line (and writes it to --out)."""
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
FIELDS = ("pos", "normal", "min_dist", "max_dist", "desc")


def resident(osa, m, rng, mp, capacity):
    """A table that holds `mp` under shuffled ids among twice as many live slots."""
    n = len(mp["pos"])
    slots = rng.permutation(capacity)[:2 * n].astype(np.int32)
    M = osa.DeviceMap(capacity)
    M.update(m, slots, **{k: np.concatenate([mp[k], mp[k][::-1]]) for k in FIELDS})
    return M, np.ascontiguousarray(slots[:n])


def equal(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return (a is None and b is None) or np.array_equal(a, b)


def local_points(osa, ob, m):
    import test_gpu_frame_handle as FH
    rng = np.random.default_rng(31)
    N, n_mp = 1000, 10000
    k, d = FH._frame(rng, N)
    src, pos, normal, min_d, max_d = FH._local_map(rng, k, n_mp, False)
    desc = FH._noisy(rng, d[src], 0.05)
    eligible, has_obs = (rng.random(n_mp) < 0.9).astype(np.uint8), (rng.random(n_mp) < 0.95).astype(np.uint8)
    a = 0.01
    Rcw = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], f32)
    tcw = np.array([0.02, -0.01, 0.03], f32)
    Ow = (-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32)
    lsf = f32(np.log(f32(1.2)))
    bounds = np.array([0.0, FH.W, 0.0, FH.H], f32)
    w = ob.is_in_frustum(Rcw, tcw, Ow, FH.EUROC4 + (0.0,), bounds, lsf, 8, 0.5, pos, normal, min_d, max_d)
    iv = w["in_view"] & eligible
    rec = dict(proj_x=w["proj_x"], proj_y=w["proj_y"], proj_xr=w["proj_xr"], level=w["level"], view_cos=w["view_cos"], desc=desc, in_view=iv,
               has_obs=has_obs)
    on, ofm = ob.search_by_projection_mappoints(ob.OracleGrid(k, 0.0, float(FH.W), 0.0, float(FH.H)), d, FH.SF, rec, 3.0, 0.8, None, None)
    F = osa.DeviceFrame(m, N).load(osa.FrameView(k, d, 0.0, float(FH.W), 0.0, float(FH.H), FH.SF))
    M, ids = resident(osa, m, rng, dict(pos=pos, normal=normal, min_dist=min_d, max_dist=max_d, desc=desc), 1 << 16)
    cam10, pose = FH.EUROC4 + (0, 0, 0, 0, 0, 0.0), (Rcw, tcw, Ow)
    forms = {"flat": lambda: m.SearchLocalPoints(F, cam10, pose, lsf, 0.5, pos, normal, min_d, max_d, desc, eligible, has_obs, 3.0),
             "map": lambda: m.SearchLocalPointsMap(F, cam10, pose, lsf, 0.5, M, ids, eligible, has_obs, 3.0)}
    return forms, (on, ofm, iv), (F, M)


def fuse_scene(osa, ob, m):
    import test_gpu_keyframe as T
    sc = T._scene(2024, 20)
    kfs = [osa.DeviceKeyFrame.from_host(m, T._view(osa, sc, k), sc["inv_level_sigma2"]) for k in range(20)]
    return T, sc, kfs


def fuse(osa, ob, m, scene):
    T, sc, kfs = scene
    want = T._reference(ob, sc, range(20))[:3]
    M, ids = resident(osa, m, np.random.default_rng(5), sc["map_points"], 1 << 14)
    forms = {"flat": lambda: m.FuseMapPoints(kfs, sc["cams"], sc["poses"], sc["map_points"], T.TH, sc["log_scale_factor"]),
             "map": lambda: m.FuseMapPointsMap(kfs, sc["cams"], sc["poses"], M, ids, T.TH, sc["log_scale_factor"])}
    return forms, want, (kfs, M)


def sim3(osa, ob, m):
    import sim3_scene as S
    import test_gpu_keyframe as T
    K = 8
    sc = S.make_scene(5, K, n_mp=800, n_dup=200)
    assert len(sc["map_points"]["pos"]) == 1000
    ref = S.search_reference(ob, sc, range(K), 8.0, 1.5, 0)
    want = (ref["nm"], ref["match"], ref["projected"], None)
    kfs = [osa.DeviceKeyFrame.from_host(m, T._view(osa, sc, k, False), None) for k in range(K)]
    M, ids = resident(osa, m, np.random.default_rng(6), sc["map_points"], 1 << 14)
    forms = {"flat": lambda: m.SearchByProjectionSim3KeyFrames(kfs, sc["cams"], sc["poses"], sc["map_points"], 8.0, 1.5, sc["log_scale_factor"]),
             "map": lambda: m.SearchByProjectionSim3KeyFramesMap(kfs, sc["cams"], sc["poses"], M, ids, 8.0, 1.5, sc["log_scale_factor"])}
    return forms, want, (kfs, M)


def pair(osa, ob, m, scene):
    """Every map point of the Fuse scene with 3..10 observations: noisy copies of its descriptor, dealt to three more key frames."""
    from distinctive_sets import noisy_copy, random_keypoints
    T, sc, kfs = scene
    rng = np.random.default_rng(8)
    mp = sc["map_points"]
    n = len(mp["pos"])
    sizes = rng.integers(3, 11, n)
    sp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = noisy_copy(rng, np.repeat(mp["desc"], sizes, axis=0), 0.08)
    r = np.arange(len(rows))
    ok, oi = (r % 3).astype(np.int32), (r // 3).astype(np.int32)
    sf = (f32(1.2) ** np.arange(8)).astype(f32)
    holders = [osa.DeviceKeyFrame.from_host(m, osa.FrameView(random_keypoints(rng, len(rows[h::3])), np.ascontiguousarray(rows[h::3]), 0.0, 640.0, 0.0,
                                                             480.0, sf), None) for h in range(3)]
    best = ob.distinctive_descriptors(rows, sp)
    new = dict(mp, desc=np.ascontiguousarray(rows[sp[:-1] + best]))
    want = (best,) + tuple(T._reference(ob, dict(sc, map_points=new), range(20))[:3])
    M, ids = resident(osa, m, np.random.default_rng(9), mp, 1 << 14)

    def flat():
        b, desc = m.DistinctiveDescriptorsKeyFrames(holders, sp, ok, oi)
        return (b,) + tuple(m.FuseMapPoints(kfs, sc["cams"], sc["poses"], dict(mp, desc=desc), T.TH, sc["log_scale_factor"]))

    def resident_pair():
        b = m.DistinctiveDescriptorsKeyFramesToMap(holders, sp, ok, oi, M, ids)
        return (b,) + tuple(m.FuseMapPointsMap(kfs, sc["cams"], sc["poses"], M, ids, T.TH, sc["log_scale_factor"]))

    return {"flat": flat, "map": resident_pair}, want, (holders, M)


def update_300(osa, m, reps, warmup):
    rng = np.random.default_rng(10)
    M = osa.DeviceMap(1 << 14)
    ids = rng.permutation(1 << 14)[:300].astype(np.int32)
    pts = dict(pos=rng.normal(0, 5, (300, 3)).astype(f32), normal=rng.normal(0, 1, (300, 3)).astype(f32), min_dist=rng.random(300).astype(f32),
               max_dist=rng.random(300).astype(f32), desc=rng.integers(0, 256, (300, 32), dtype=np.uint8))
    call, synced = [], []
    for rep in range(warmup + reps):
        pts["pos"] += f32(0.5)
        t0 = time.perf_counter()
        M.update(m, ids, **pts)
        t1 = time.perf_counter()
        got = M.read(m, ids[:1])
        t2 = time.perf_counter()
        assert np.array_equal(got["pos"][0], pts["pos"][0]) and np.array_equal(got["desc"][0], pts["desc"][0]), rep
        if rep >= warmup:
            call.append((t1 - t0) * 1e6); synced.append((t2 - t0) * 1e6)
    got = M.read(m, ids)
    assert all(np.array_equal(got[k], pts[k]) for k in FIELDS)
    return {"update_300_call": call, "update_300_then_read1": synced}


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
    from oracle import oracle_binding as ob

    m = osa.ORBmatcher(0.8, True)
    res = {"tool": "map_resident_latency", "reps": args.reps}
    scene = fuse_scene(osa, ob, m)
    for name, build in (("local_points", lambda: local_points(osa, ob, m)), ("fuse", lambda: fuse(osa, ob, m, scene)), ("sim3", lambda: sim3(osa, ob, m)),
                        ("pair", lambda: pair(osa, ob, m, scene))):
        m.mfNNratio = 0.8 if name == "local_points" else 0.6
        forms, want, keep = build()
        times = {f: [] for f in forms}
        for rep in range(args.warmup + args.reps):
            for f, fn in forms.items():   # the forms alternate repetition by repetition
                t0 = time.perf_counter()
                out = fn()                # (every entry point synchronises before it returns)
                dt = time.perf_counter() - t0
                assert equal(tuple(out), tuple(want)), (name, f, rep)
                if rep >= args.warmup:
                    times[f].append(dt * 1e6)
        for f, a in times.items():
            for key, v in stats(a).items():
                res[f"{name}_{f}_{key}"] = v
            forms[f]()
            res[f"{name}_{f}_upload_bytes"] = m.last_transfers()["upload_bytes"]
        spread = res[f"{name}_flat_max_us"] - res[f"{name}_flat_min_us"]
        res[f"{name}_map_over_flat"] = round(res[f"{name}_map_med_us"] / res[f"{name}_flat_med_us"], 3)
        res[f"{name}_within_spread"] = bool(res[f"{name}_map_med_us"] <= res[f"{name}_flat_med_us"] + spread)
        del keep
    for name, a in update_300(osa, m, args.reps, args.warmup).items():
        for key, v in stats(a).items():
            res[f"{name}_{key}"] = v
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
