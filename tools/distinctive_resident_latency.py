#!/usr/bin/env python3
"""Latency of MapPoint::ComputeDistinctiveDescriptors for the map points of one LocalMapping step (not imported by bench.py): 2000 map points with
3..30 observations each, plus a few of 100..300, on 40 resident key frames of 1000..2000 features -- once all monocular, once with every second key
frame a fisheye-stereo rig -- timed three ways on the same sets:
  * resident: ONE orbx_keyframe_distinctive_descriptors (set_ptr, two index arrays and a record per key frame go up; winners and their rows come down);
  * gather:   today's route -- the rows gathered on the host into one array, then orbx_distinctive_descriptors -- with the gather INSIDE the timed
              region.  The gather here is one numpy fancy-index over the concatenated key frames, cheaper than the adapter's walk through cv::Mat
              rows: that favours this form.  It returns indices only; the resident form also returns the winning rows;
  * cpu:      the CPU oracle on one core on rows gathered beforehand (the gather is not timed: the reference reads the rows in place).
The forms alternate repetition by repetition in one process; every output of every repetition is compared with the oracle's.  Reports median / min /
max in microseconds per form and workload (host clock around calls that end in a stream synchronisation).
Kernel-only times come from a run of their own: a child process under `rocprofv3 --kernel-trace --stats` (no counters) that alternates the two GPU
forms on the monocular workload; k_distinctive_kf (+ k_distinctive_kf_large) beside k_distinctive on the same sets, per-call average and total, once
with all sets and once with the sets of 3..30 observations only.  --no-trace skips it.
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

N_KF, N_MP, N_LARGE = 40, 2000, 8
W, H = 752.0, 480.0


def make_workload(seed, rigs, n_mp=N_MP, n_large=N_LARGE):
    """Key frames (host rows in the reference's numbering, the rig's left count or None) and the observation sets."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1000, 2001, N_KF)
    desc = [rng.integers(0, 256, (int(k), 32), dtype=np.uint8) for k in n]
    n_left = [int(0.6 * k) if rigs and i % 2 else None for i, k in enumerate(n)]
    sizes = [int(x) for x in rng.integers(3, 31, n_mp - n_large)] + [int(x) for x in rng.integers(100, 301, n_large)]
    rng.shuffle(sizes)
    obs_kf, obs_idx, set_ptr = [], [], [0]
    for sz in sizes:
        seen = rng.choice(N_KF, sz, replace=sz > N_KF)   # std::map order: ascending key frames
        cnt = 0
        for k in np.sort(seen):
            if cnt == sz:
                break
            nl = n_left[k]
            if nl is None:
                obs_kf.append(k); obs_idx.append(int(rng.integers(0, n[k]))); cnt += 1
            else:   # a rig observation: leftIndex, then rightIndex, each where it is not -1 (left only 40 %, both 40 %, right only 20 %)
                r = rng.random()
                for i in ([int(rng.integers(0, nl))] if r < 0.8 else []) + ([nl + int(rng.integers(0, n[k] - nl))] if r >= 0.4 else []):
                    if cnt < sz:
                        obs_kf.append(k); obs_idx.append(i); cnt += 1
        set_ptr.append(len(obs_kf))
    return dict(desc=desc, n_left=n_left, set_ptr=np.array(set_ptr, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_idx=np.array(obs_idx, np.int32))


def resident_key_frames(osa, m, wl, seed):
    from distinctive_sets import random_keypoints
    rng = np.random.default_rng(seed)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    kfs = []
    for d, nl in zip(wl["desc"], wl["n_left"]):
        kps = random_keypoints(rng, len(d), W, H)
        if nl is None:
            kfs.append(osa.DeviceKeyFrame.from_host(m, osa.FrameView(kps, d, 0.0, W, 0.0, H, sf), None))
        else:
            kfs.append(osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kps[:nl], d, 0.0, W, 0.0, H, sf), kps[nl:], None))
    return kfs


def forms_of(osa, ob, m, wl, kfs):
    flat = np.concatenate(wl["desc"])
    base = np.concatenate([[0], np.cumsum([len(d) for d in wl["desc"]])]).astype(np.int64)
    sp, ok, oi = wl["set_ptr"], wl["obs_kf"], wl["obs_idx"]
    rows = np.ascontiguousarray(flat[base[ok] + oi])
    want = ob.distinctive_descriptors(rows, sp)

    def resident():
        return m.DistinctiveDescriptorsKeyFrames(kfs, sp, ok, oi)[0]

    def gather():
        return m.DistinctiveDescriptors(flat[base[ok] + oi], sp)

    def cpu():
        return ob.distinctive_descriptors(rows, sp)

    return {"resident": resident, "gather": gather, "cpu": cpu}, want


def kernel_trace(out_dir, reps, n_mp, n_large):
    """One serialized rocprofv3 --kernel-trace --stats run (no counters) of a child that alternates the two GPU forms; per-kernel statistics."""
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 is not installed")
    d = Path(out_dir) / "kt"
    shutil.rmtree(d, ignore_errors=True)
    r = subprocess.run([exe, "--kernel-trace", "--stats", "-d", str(d), "-o", "kt", "--", sys.executable, str(Path(__file__).resolve()),
                        "--trace-child", "--reps", str(reps), "--map-points", str(n_mp), "--large", str(n_large)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the traced child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    dbs = sorted(d.rglob("*.db"), key=lambda p: p.stat().st_size)
    if not dbs:
        raise RuntimeError("rocprofv3 wrote no .db")
    cur = sqlite3.connect(str(dbs[-1])).execute("select name, total_calls, total_duration, average from top_kernels")
    stats = {}
    for name, calls, total, avg in cur:
        short = name.split("(")[0].split("::")[-1]
        if short in ("k_distinctive_kf", "k_distinctive_kf_large", "k_distinctive", "k_xfer"):   # (the view's durations are microseconds)
            stats[short] = {"calls": int(calls), "total_us": round(float(total), 1), "avg_us": round(float(avg), 2)}
    shutil.rmtree(d, ignore_errors=True)
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--map-points", type=int, default=N_MP)
    ap.add_argument("--large", type=int, default=N_LARGE, help="sets of 100..300 observations among the map points")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    import orb_slam3_amd as osa
    from oracle import oracle_binding as ob

    m = osa.ORBmatcher(0.6, True)
    workloads = {"monocular": make_workload(404, False, args.map_points, args.large)}
    if not args.trace_child:
        workloads["half_rigs"] = make_workload(405, True, args.map_points, args.large)
    res = {"tool": "distinctive_resident_latency", "key_frames": N_KF, "map_points": args.map_points, "reps": args.reps}
    keep = []
    for wname, wl in workloads.items():
        kfs = resident_key_frames(osa, m, wl, 7)
        keep.append(kfs)
        forms, want = forms_of(osa, ob, m, wl, kfs)
        if args.trace_child:
            forms.pop("cpu")
        sizes = np.diff(wl["set_ptr"])
        res[f"{wname}_observations"] = int(wl["set_ptr"][-1])
        res[f"{wname}_sets_above_64"] = int((sizes > 64).sum())
        res[f"{wname}_winner_not_first"] = float((want != 0).mean())
        times = {name: [] for name in forms}
        for rep in range(args.warmup + args.reps):
            for name, fn in forms.items():   # the forms alternate repetition by repetition
                t0 = time.perf_counter()
                out = fn()                    # (every entry point synchronises before it returns)
                dt = time.perf_counter() - t0
                assert np.array_equal(out, want), (wname, name, rep)
                if rep >= args.warmup:
                    times[name].append(dt * 1e6)
        for name, a in times.items():
            a = np.array(a)
            res[f"{wname}_{name}_med_us"], res[f"{wname}_{name}_min_us"], res[f"{wname}_{name}_max_us"] = (
                round(float(np.median(a)), 1), round(float(a.min()), 1), round(float(a.max()), 1))
        forms["resident"]()
        res[f"{wname}_resident_upload_bytes"] = m.last_transfers()["upload_bytes"]
        forms["gather"]()
        res[f"{wname}_gather_upload_bytes"] = m.last_transfers()["upload_bytes"]
        res[f"{wname}_resident_over_gather"] = round(res[f"{wname}_resident_med_us"] / res[f"{wname}_gather_med_us"], 3)
    if args.trace_child:
        return
    if not args.no_trace:
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="distinctive_trace_"))   # the trace's files; removed after reading
        out_dir.mkdir(parents=True, exist_ok=True)
        for tag, n_large in (("all_sets", args.large), ("small_sets", 0)):   # the same map points; without the sets of 100..300 observations
            for k, v in kernel_trace(out_dir, 20, args.map_points, n_large).items():
                for field, x in v.items():
                    res[f"trace_{tag}_{k}_{field}"] = x
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
