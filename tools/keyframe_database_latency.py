#!/usr/bin/env python3
"""Latency of the key-frame database query (not imported by bench.py).  Workload: a synthetic vocabulary with k = 10, L = 5 (100 000 words; the real
ORBvoc has 10^6), databases of 1000 and 4000 key frames of 1000 features, a 1000-feature query frame that is resident.  Per database size:
  host     the route this build's query replaces: orbx_frame_compute_bow with the ids downloaded, then the adapter's fold into mBowVec and the first
           half of KeyFrameDatabase::DetectRelocalizationCandidates as C++ on one core (std::map BowVectors, a std::vector<std::list<int>> inverted
           file: tools/keyframe_database_host_loop.cpp); `host_loop` is that C++ part alone, by its own clock
  device   orbx_frame_compute_bow without downloads + orbx_keyframe_database_query_frame (the candidate list, no full arrays), with the bytes that
           cross the link per query; `device_below_host_min`: its median lies below the host route's minimum
  kernels  the query's three kernels from one serialized rocprofv3 --kernel-trace --stats run of a child (no counters)
  add      the host time of one orbx_keyframe_database_add (it does not wait); its device cost is k_bow_vector's
40 timed repetitions, the forms alternating, every output checked in every repetition (the device's candidates, counts and score bits are the host
loop's); median (min - max) in microseconds, host clock around calls that end in a stream synchronisation.  Prints one JSON line (and writes it to
--out)."""
import argparse
import ctypes as C
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

K, L, LEVELSUP, N_FEAT, CAND_CAP = 10, 5, 4, 1000, 256
SIZES = (1000, 4000)


def stats(res, key, a):
    a = np.array(a)
    res[f"{key}_med_us"], res[f"{key}_min_us"], res[f"{key}_max_us"] = round(float(np.median(a)), 1), round(float(a.min()), 1), round(float(a.max()), 1)


def vocabulary(rng):
    """a full k-ary tree; node descriptors are noisy copies of their parent's, so that near descriptors share words"""
    n_nodes = sum(K ** d for d in range(L + 1))
    cp = np.zeros(n_nodes + 1, np.int32)
    ci, desc, wid = [], np.zeros((n_nodes, 32), np.uint8), np.full(n_nodes, -1, np.int32)
    desc[0] = rng.integers(0, 256, 32)
    first, nxt = 0, 1
    for d in range(L):
        for i in range(first, first + K ** d):
            kids = np.arange(nxt, nxt + K)
            ci.extend(kids)
            flip = rng.integers(0, 256, (K, 32), dtype=np.uint8) & rng.integers(0, 256, (K, 32), dtype=np.uint8)
            if d > 1:
                flip &= rng.integers(0, 256, (K, 32), dtype=np.uint8)
            desc[kids] = desc[i] ^ flip
            cp[i + 1] = len(ci)
            nxt += K
        first += K ** d
    cp[first + 1:] = len(ci)
    wid[first:] = np.arange(n_nodes - first)
    weights = rng.uniform(0.5, 12.0, n_nodes - first)
    weights[rng.random(len(weights)) < 0.02] = 0.0
    return cp, np.array(ci, np.int32), desc, wid, weights


def sparse_noise(rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8) & rng.integers(0, 256, shape, dtype=np.uint8) & rng.integers(0, 256, shape, dtype=np.uint8) \
        & rng.integers(0, 256, shape, dtype=np.uint8)


def setup(n_kf, want_host=True):
    import orb_slam3_amd as osa
    import bow_database_scene as B
    from test_gpu_frame_bow import H, SF, W, _keypoints
    rng = np.random.default_rng(41)
    cp, ci, nd, wi, weights = vocabulary(rng)
    voc = osa.ORBVocabulary(L, cp, ci, nd, wi).set_word_weights(weights)
    leaves = nd[wi >= 0]
    places = [leaves[rng.integers(0, len(leaves), 3000)] for _ in range(20)]       # 20 places of 3000 landmarks
    m = osa.ORBmatcher(0.75, True)
    kps = _keypoints(rng, N_FEAT)

    def view(place):
        d = places[place][rng.permutation(3000)[:N_FEAT]]
        return osa.FrameView(kps, np.ascontiguousarray(d ^ sparse_noise(rng, d.shape)), 0.0, float(W), 0.0, float(H), SF)
    host = None
    if want_host:
        so = Path(tempfile.mkdtemp(prefix="kfdb_host_")) / "host_loop.so"
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", str(so), str(Path(__file__).with_name("keyframe_database_host_loop.cpp"))], check=True)
        host = C.CDLL(str(so))
        host.kfdb_host_create.restype = C.c_void_p
        host.kfdb_host_create.argtypes = [C.c_int, C.c_void_p]
        host.kfdb_host_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        host.kfdb_host_destroy.argtypes = [C.c_void_p]
        host.kfdb_host_query.restype = C.c_double
        host.kfdb_host_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int)]
        host.db = host.kfdb_host_create(len(weights), weights.ctypes.data)
    db = osa.DeviceKeyFrameDatabase(n_kf, N_FEAT)
    add_us = []
    for s in range(n_kf):
        kf = osa.DeviceKeyFrame.from_host(m, view(s % 20), None)
        w, _ = kf.compute_bow(m, voc, LEVELSUP)
        t0 = time.perf_counter()
        db.add(m, s, kf)
        add_us.append((time.perf_counter() - t0) * 1e6)
        if host is not None:
            assert host.kfdb_host_add(host.db, w.ctypes.data, len(w)) == s
    F = osa.DeviceFrame(m, N_FEAT).load(view(3))
    return dict(m=m, voc=voc, db=db, F=F, host=host, add_us=add_us[n_kf // 2:], B=B)


def measure(res, n_kf, reps, warmup):
    S = setup(n_kf)
    m, voc, db, F, host, B = S["m"], S["voc"], S["db"], S["F"], S["host"], S["B"]
    hc, hcc, hs = np.zeros(CAND_CAP, np.int32), np.zeros(CAND_CAP, np.int32), np.zeros(CAND_CAP, np.float64)
    hn, hmx = C.c_int(0), C.c_int(0)
    times = {"host": [], "device": [], "host_loop": []}
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        w, _ = F.compute_bow(voc, LEVELSUP)
        loop_us = host.kfdb_host_query(host.db, w.ctypes.data, len(w), 0.8, hc.ctypes.data, hcc.ctypes.data, hs.ctypes.data, CAND_CAP, C.byref(hn), C.byref(hmx))
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        F.compute_bow(voc, LEVELSUP, download=False)
        got = db.query_frame(m, F, min_ratio=0.8, cand_cap=CAND_CAP, full=False)
        t_dev = time.perf_counter() - t0
        xf = m.last_transfers()
        k = hn.value
        assert 0 < k <= CAND_CAP and got["n_cand"] == k and got["max_common"] == hmx.value, (rep, k, got["n_cand"], got["max_common"], hmx.value)
        assert np.array_equal(got["cand_slot"], hc[:k]) and np.array_equal(got["cand_common"], hcc[:k]), rep
        assert np.array_equal(B.bits(got["cand_score"]), B.bits(hs[:k])), rep
        if rep >= warmup:
            times["host"].append(t_host * 1e6); times["device"].append(t_dev * 1e6); times["host_loop"].append(loop_us)
    key = f"kf{n_kf}"
    for name, a in times.items():
        stats(res, f"{key}_{name}", a)
    stats(res, f"{key}_add_host", S["add_us"])
    full = db.query_frame(m, F, min_ratio=0.8, cand_cap=CAND_CAP, full=True)
    res[f"{key}_candidates"], res[f"{key}_max_common"], res[f"{key}_slots_sharing_a_word"] = int(hn.value), int(hmx.value), int((full["n_common"] > 0).sum())
    res[f"{key}_query_words"] = int(len(F.bow_vector()[0]))
    res[f"{key}_device_upload_bytes"], res[f"{key}_device_download_bytes"] = xf["upload_bytes"], xf["download_bytes"]
    res[f"{key}_host_download_bytes"] = 8 * N_FEAT            # the word and node ids of the frame
    res[f"{key}_device_below_host_min"] = bool(res[f"{key}_device_med_us"] < res[f"{key}_host_min_us"])
    host.kfdb_host_destroy(host.db)


def child(n_kf, reps):
    S = setup(n_kf, want_host=False)
    S["F"].compute_bow(S["voc"], LEVELSUP, download=False)
    for _ in range(reps):
        S["db"].query_frame(S["m"], S["F"], min_ratio=0.8, cand_cap=CAND_CAP, full=False)


def kernels(res, out_dir, sizes):
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 is not installed")
    for n_kf in sizes:
        d = Path(out_dir) / f"kt{n_kf}"
        shutil.rmtree(d, ignore_errors=True)
        r = subprocess.run([exe, "--kernel-trace", "--stats", "-d", str(d), "-o", "kt", "--", sys.executable, str(Path(__file__).resolve()), "--child", str(n_kf),
                            "--reps", "20"], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("the traced child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        dbs = sorted(d.rglob("*.db"), key=lambda p: p.stat().st_size)
        if not dbs:
            raise RuntimeError("rocprofv3 wrote no .db")
        for name, calls, total, avg in sqlite3.connect(str(dbs[-1])).execute("select name, total_calls, total_duration, average from top_kernels"):
            for kn in ("k_bow_vector", "k_bow_score", "k_bow_select"):
                if kn in name:
                    res[f"kf{n_kf}_{kn}_calls"], res[f"kf{n_kf}_{kn}_avg_us"] = int(calls), round(float(avg), 2)   # (the view's durations are microseconds)
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES), help="key frames per database")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return
    res = {"tool": "keyframe_database_latency", "reps": args.reps, "vocabulary_words": K ** L, "features": N_FEAT, "cand_cap": CAND_CAP}
    for n_kf in args.sizes:
        measure(res, n_kf, args.reps, args.warmup)
    if not args.no_trace:
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="keyframe_database_trace_"))
        out_dir.mkdir(parents=True, exist_ok=True)
        kernels(res, out_dir, args.sizes)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
