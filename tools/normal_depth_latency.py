#!/usr/bin/env python3
"""Latency of refreshing map points on the device -- descriptor, normal and both distance bounds in one call -- against the descriptor-only call and
against the route through the host (not imported by bench.py).  The workload is DESIGN 7l's LocalMapping step: 2000 map points with 3..30
observations each, eight of them with 100..300, over 40 resident key frames, half of them rigs with a second pyramid (5 levels, factor 1.1).  Forms,
alternating repetition by repetition in one process on one table each:
  (a) distinct   orbx_keyframe_distinctive_descriptors_to_map alone: the yardstick
  (b) host       (a), then normals and bounds on the host, then orbx_map_update of the three fields (it does not wait; the next call's wait does).
                 The host part is NUMPY, vectorised across the sets position by position -- not the integrator's C++ loop under two mutexes.
  (c) refresh    orbx_keyframe_refresh_map_points_to_map
Every output of every repetition -- best_obs and the records of all 2000 slots, whose normal, bounds and descriptor are overwritten with garbage before
each repetition -- is compared with the composed reference (oracle.distinctive_descriptors, tests/normal_depth_scene.reference_normal_depth).
Reports median (min - max) in microseconds (host clock around calls that end in a stream synchronisation; form (b) is closed by a one-slot read),
`refresh_within_spread`: (c)'s median is not above (a)'s by more than (a)'s own max - min of this run, and per-kernel times from one serialized
rocprofv3 --kernel-trace --stats run of a child.  Prints one JSON line (and writes it to --out)."""
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
N_KF, N_MP, N_LARGE = 40, 2000, 8
FIELDS = ("pos", "normal", "min_dist", "max_dist", "desc")


def make_workload(seed):
    import normal_depth_scene as ND
    rng = np.random.default_rng(seed)
    kfs = []
    for k in range(N_KF):
        rig = k % 2 == 1
        nlevels, factor = ND.PYRAMIDS[1 if rig else 0]
        nl, nr = (800, 700) if rig else (1500, -1)
        kl, kr = ND._keypoints(rng, nl, nlevels), ND._keypoints(rng, max(nr, 0), nlevels)
        c = rng.normal(0, 2, 3).astype(f32)
        kfs.append(dict(n_left=nl, n_right=nr, kps=kl, kps_right=kr, octave=np.concatenate([kl["octave"], kr["octave"]]).astype(np.int32),
                        scale=ND.scale_factors(nlevels, factor), center=c, center_right=(c + rng.normal(0, 0.08, 3).astype(f32)).astype(f32) if rig else None,
                        desc=rng.integers(0, 256, (nl + max(nr, 0), 32), dtype=np.uint8)))
    sizes = rng.integers(3, 31, N_MP)
    sizes[rng.permutation(N_MP)[:N_LARGE]] = rng.integers(100, 301, N_LARGE)
    sets = [ND._random_set(rng, kfs, int(n)) for n in sizes]
    refs = [ND._pick_ref(rng, kfs, s) for s in sets]
    mid = np.mean([kf["center"] for kf in kfs], axis=0)
    d = rng.normal(0, 1, (N_MP, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return dict(key_frames=kfs, sizes=list(sizes), set_ptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                obs_kf=np.array([k for s in sets for k, _ in s], np.int32), obs_idx=np.array([i for s in sets for _, i in s], np.int32),
                ref_obs=np.array(refs, np.int32), pos=(mid + d * rng.uniform(9, 13, (N_MP, 1))).astype(f32), nan_set=-1)


def host_normal_depth(wl, pre):
    """reference_normal_depth in float32 numpy, vectorised ACROSS the sets: position j of every set that has one is added in step j, so every set's
    sum keeps the order of its list and every operation rounds on its own.  `pre`: what does not depend on pos (gathered once)."""
    sp, pos = wl["set_ptr"], wl["pos"]
    P = pos[pre["set_of"]]
    d = (P - pre["centre"]).astype(f32)
    nrm = np.sqrt((((f32(0) + d[:, 0] * d[:, 0]).astype(f32) + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32))
    t = (d / nrm[:, None]).astype(f32)
    acc = np.zeros((len(sp) - 1, 3), f32)
    for j, members in enumerate(pre["at_position"]):
        acc[members] = (acc[members] + t[sp[members] + j]).astype(f32)
    normal = (acc / pre["n"][:, None]).astype(f32)
    pc = (pos - pre["ref_centre"]).astype(f32)
    dist = np.sqrt((((f32(0) + pc[:, 0] * pc[:, 0]).astype(f32) + pc[:, 1] * pc[:, 1]).astype(f32) + pc[:, 2] * pc[:, 2]).astype(f32))
    mx = (dist * pre["ref_scale"]).astype(f32)
    return normal, (mx / pre["last_scale"]).astype(f32), mx


def precompute(wl):
    kfs, sp, ok, oi = wl["key_frames"], wl["set_ptr"], wl["obs_kf"], wl["obs_idx"]
    sizes = np.diff(sp)
    right = np.array([kfs[k]["n_right"] >= 0 and i >= kfs[k]["n_left"] for k, i in zip(ok, oi)])
    centre = np.stack([kfs[k]["center_right"] if r else kfs[k]["center"] for k, r in zip(ok, right)]).astype(f32)
    o = sp[:-1] + wl["ref_obs"]
    return dict(set_of=np.repeat(np.arange(len(sizes)), sizes), centre=centre, n=sizes.astype(f32),
                at_position=[np.flatnonzero(sizes > j) for j in range(int(sizes.max()))],
                ref_centre=np.stack([kfs[k]["center"] for k in ok[o]]).astype(f32),
                ref_scale=np.array([kfs[k]["scale"][kfs[k]["octave"][i]] for k, i in zip(ok[o], oi[o])], f32),
                last_scale=np.array([kfs[k]["scale"][-1] for k in ok[o]], f32))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


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
        short = name.split("(")[0].split("::")[-1]
        if short in ("k_distinctive_kf", "k_distinctive_kf_large", "k_normal_depth_kf", "k_map_scatter_refresh", "k_map_scatter_desc", "k_xfer"):
            stats[short] = {"calls": int(calls), "total_us": round(float(total), 1), "avg_us": round(float(avg), 2)}   # (the view's durations are microseconds)
    shutil.rmtree(d, ignore_errors=True)
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    import distinctive_sets as DS
    import normal_depth_scene as ND
    import orb_slam3_amd as osa
    from oracle import oracle_binding as ob

    wl = make_workload(505)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, wl)
    c, cr = ND.centers(wl)
    sp, ok, oi, ro = wl["set_ptr"], wl["obs_kf"], wl["obs_idx"], wl["ref_obs"]
    rows = DS.gather([kf["desc"] for kf in wl["key_frames"]], ok, oi)
    want_best = ob.distinctive_descriptors(rows, sp)
    want_desc = np.ascontiguousarray(rows[sp[:-1] + want_best])
    want = ND.reference(wl)
    pre = precompute(wl)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(host_normal_depth(wl, pre), want)), "the vectorised host form is not the reference"
    rng = np.random.default_rng(9)
    ids = np.ascontiguousarray(rng.permutation(1 << 14)[:N_MP].astype(np.int32))
    garbage = dict(normal=rng.normal(0, 1, (N_MP, 3)).astype(f32), min_dist=rng.random(N_MP).astype(f32), max_dist=rng.random(N_MP).astype(f32),
                   desc=rng.integers(0, 256, (N_MP, 32), dtype=np.uint8))
    tables = {}

    def distinct(M):
        return m.DistinctiveDescriptorsKeyFramesToMap(kfs, sp, ok, oi, M, ids)

    def host(M):
        best = distinct(M)
        normal, mn, mx = host_normal_depth(wl, pre)
        M.update(m, ids, normal=normal, min_dist=mn, max_dist=mx)
        M.read(m, ids[:1])   # (the update does not wait: the following call's synchronisation closes it)
        return best

    def refresh(M):
        return m.RefreshMapPointsToMap(kfs, c, cr, sp, ok, oi, ro, M, ids)

    forms = {"distinct": distinct, "refresh": refresh} if args.trace_child else {"distinct": distinct, "host": host, "refresh": refresh}
    for name in forms:
        tables[name] = osa.DeviceMap(1 << 14)
        tables[name].update(m, ids, pos=wl["pos"], **garbage)
    res = {"tool": "normal_depth_latency", "key_frames": N_KF, "map_points": N_MP, "observations": int(sp[-1]), "sets_above_64": int((np.diff(sp) > 64).sum()),
           "reps": args.reps}
    times = {name: [] for name in forms}
    for rep in range(args.warmup + args.reps):
        for name, fn in forms.items():   # the forms alternate repetition by repetition
            M = tables[name]
            M.update(m, ids, **garbage)
            M.read(m, ids[:1])
            t0 = time.perf_counter()
            best = fn(M)                  # (every form ends in a stream synchronisation)
            dt = time.perf_counter() - t0
            rec = M.read(m, ids)
            assert np.array_equal(best, want_best) and np.array_equal(rec["desc"], want_desc) and np.array_equal(bits(rec["pos"]), bits(wl["pos"])), (name, rep)
            expect = (garbage["normal"], garbage["min_dist"], garbage["max_dist"]) if name == "distinct" else want
            assert all(np.array_equal(bits(rec[k]), bits(w)) for k, w in zip(FIELDS[1:4], expect)), (name, rep)
            if rep >= args.warmup:
                times[name].append(dt * 1e6)
    if args.trace_child:
        return
    for name, a in times.items():
        a = np.array(a)
        res[f"{name}_med_us"], res[f"{name}_min_us"], res[f"{name}_max_us"] = round(float(np.median(a)), 1), round(float(a.min()), 1), round(float(a.max()), 1)
        forms[name](tables[name])
        if name != "host":
            res[f"{name}_upload_bytes"] = m.last_transfers()["upload_bytes"]
    t0 = time.perf_counter()
    for _ in range(20):
        host_normal_depth(wl, pre)
    res["host_numpy_part_us"] = round((time.perf_counter() - t0) / 20 * 1e6, 1)
    spread = res["distinct_max_us"] - res["distinct_min_us"]
    res["refresh_minus_distinct_us"] = round(res["refresh_med_us"] - res["distinct_med_us"], 1)
    res["refresh_within_spread"] = bool(res["refresh_med_us"] <= res["distinct_med_us"] + spread)
    res["refresh_over_host"] = round(res["refresh_med_us"] / res["host_med_us"], 3)
    if not args.no_trace:
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="normal_depth_trace_"))   # the trace's files; removed after reading
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
