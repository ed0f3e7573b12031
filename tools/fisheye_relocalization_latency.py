#!/usr/bin/env python3
"""Latency of Tracking::Relocalization's matching per frame of a fisheye-stereo rig (Frame::Nleft != -1, TUM-VI shape; not imported by bench.py):

    ComputeBoW over N = N_left + N_right rows -> SearchByBoW(pKF, F) of ORBmatcher.cc:283-392 for K candidate key frames (related and unrelated,
    ~2000 features: both cameras of another frame) -> one SearchByProjection window search (10, 100) over the LEFT camera

timed three ways on the same inputs, for K = 1, 8, 32:
  * cpu:    the CPU oracle on one core (transform + FeatureVector on the host, K x search_by_bow_frame_fisheye, the window search);
  * calls:  host-pointer entry points -- orbx_bow_transform, the FeatureVector built on the host, K x orbx_search_by_bow_frame_fisheye,
            orbx_search_by_projection_window over the left view;
  * handle: orbx_frame_load_host_fisheye, orbx_frame_compute_bow_fisheye (word ids downloaded, as the adapter needs them for mBowVec), ONE
            orbx_frame_search_by_bow_fisheye for all K, orbx_frame_search_by_projection_window_fisheye.
Every output of every form is compared with the oracle's.  Prints one JSON line: the median and p90 (microseconds) of each form and K."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

W = H = 512


def featvec(osa, node, kept):
    """FeatureVector of the kept features (vectorised: the host folding an adapter does in C++ costs about as much)"""
    nk = node[kept]
    order = np.argsort(nk, kind="stable")
    nodes, starts = np.unique(nk[order], return_index=True)
    fv = osa.FeatureVector.__new__(osa.FeatureVector)
    fv.node_id = nodes.astype(np.uint32)
    fv.node_ptr = np.append(starts, len(order)).astype(np.int32)
    fv.index = kept[order].astype(np.int32)
    return fv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    from test_gpu_matcher import _random_vocabulary

    rng = np.random.default_rng(3)
    canvas = synth.make_canvas(11, size=2048)
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    frames = []   # per rig frame: (mvKeys, mvKeysRight, all N descriptors)
    for t in range(6):
        left, right = synth.make_stereo_pair(11, t, W, H, canvas)
        _, kl, dl = ex(left, None, (0, 0))
        _, kr, dr = ex(right, None, (0, 0))
        frames.append((kl, kr, np.concatenate([dl, dr]).reshape(-1, 32)))
    sf = ex.GetScaleFactors()
    # a vocabulary of ~10^4 leaves (k = 10, L = 4) whose node descriptors are sampled from the frames' descriptors; ~5 % stop words
    cp, ci, nd, wi = _random_vocabulary(rng, 10, 4, ragged=False)
    pool = np.concatenate([f[2] for f in frames])
    nd = pool[rng.integers(0, len(pool), len(nd))] ^ np.packbits(rng.random((len(nd), 256)) < 0.03, axis=1, bitorder="little")
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.05] = 0.0
    voc = osa.ORBVocabulary(4, cp, ci, nd, wi).set_word_weights(weights)
    levelsup = 2   # node ids two levels below the root (ORB-SLAM3: levelsup 4 of its 6-level vocabulary)

    def cpu_fv(desc):
        w, node = ob.bow_transform(cp, ci, nd, wi, 4, levelsup, desc)
        return w, node, featvec(osa, node, np.nonzero(weights[w] > 0)[0])

    kl, kr, dc = frames[5]
    nl, N = len(kl), len(dc)
    ang_c = np.concatenate([kl["angle"], kr["angle"]]).astype(np.float32)
    F = osa.FrameView(kl, dc[:nl], 0.0, float(W), 0.0, float(H), sf)   # the left view (N_left, mvKeys): the window search's host form
    FL = osa.FrameView(kl, dc, 0.0, float(W), 0.0, float(H), sf)       # the fisheye load: mvKeys, the descriptors of all N rows
    l2r, r2l = np.full(nl, -1, np.int32), np.full(N - nl, -1, np.int32)
    grid = ob.OracleGrid(kl, 0.0, float(W), 0.0, float(H))
    # key frames: both cameras of the other five frames (related) and random ones (unrelated), 80 % of their features with a map point;
    # angles from mvKeys / mvKeysRight
    kf_pool = []
    for j in range(32):
        fk = frames[(j // 2) % 5] if j % 2 == 0 else frames[j % 5]
        ang = np.concatenate([fk[0]["angle"], fk[1]["angle"]]).astype(np.float32)
        d = fk[2] if j % 2 == 0 else rng.integers(0, 256, (len(ang), 32), dtype=np.uint8)
        kf_pool.append((d, ang, (rng.random(len(ang)) < 0.8).astype(np.uint8), cpu_fv(d)[2], fk[0]))
    k0 = kf_pool[0][4]
    lvl = np.clip(k0["octave"], 0, 7)
    q = dict(x=k0["x"] - 2.0, y=k0["y"] - 1.0, r=(10.0 * sf[lvl]).astype(np.float32), min_level=lvl - 1, max_level=lvl + 1, angle=k0["angle"],
             desc=kf_pool[0][0][:len(k0)])
    occ = np.zeros(N, np.uint8)

    m = osa.ORBmatcher(0.75, True)
    mw = osa.ORBmatcher(0.9, True)
    D = osa.DeviceFrame(m, 4000)

    def run_cpu(K):
        w, node, fv = cpu_fv(dc)
        res = [ob.search_by_bow_frame_fisheye(d, ang, v, f, dc, ang_c, nl, fv, 0.75, True) for d, ang, v, f, _ in kf_pool[:K]]
        n, wm = ob.search_by_projection_window(grid, dc[:nl], q, 100.0, True, False, occ[:nl])
        return w, res, (n, np.concatenate([wm, np.full(N - nl, -1, np.int32)]))

    def run_calls(K):
        w, node = m.BowTransform(voc, dc, levelsup)
        fv = featvec(osa, node, np.nonzero(weights[w] > 0)[0])   # the adapter's host folding
        res = [m.SearchByBoWFrameFisheye(d, ang, v, f, dc, ang_c, nl, fv) for d, ang, v, f, _ in kf_pool[:K]]
        n, wm = mw.SearchByProjectionWindow(F, q, 100.0, True, occ[:nl])
        return w, res, (n, np.concatenate([wm, np.full(N - nl, -1, np.int32)]))

    def run_handle(K):
        D.load_fisheye(FL, kr, l2r, r2l)
        w, _ = D.compute_bow_fisheye(voc, levelsup)
        nm, match = m.SearchByBoWDeviceFisheye(D, [(d, ang, v, f) for d, ang, v, f, _ in kf_pool[:K]])
        win = m.SearchByProjectionWindowFisheye(D, q, 100.0, True, occ)   # (window matchers take the caller's check_orientation; nnratio unused)
        return w, [(int(nm[k]), match[k]) for k in range(K)], win

    def same(x, y):
        w1, r1, (n1, m1) = x
        w2, r2, (n2, m2) = y
        return (np.array_equal(w1, w2) and len(r1) == len(r2) and all(a_ == b_ and np.array_equal(c, e) for (a_, c), (b_, e) in zip(r1, r2))
                and n1 == n2 and np.array_equal(np.maximum(m1, -1), m2))

    result = {"frame_features": [int(nl), int(N - nl)], "keyframe_features": int(np.median([len(p[1]) for p in kf_pool])), "reps": a.reps}
    for K in [int(x) for x in a.ks.split(",")]:
        want = run_cpu(K)
        assert same(run_calls(K), want) and same(run_handle(K), want), K
        times = {"cpu": [], "calls": [], "handle": []}
        fns = {"cpu": run_cpu, "calls": run_calls, "handle": run_handle}
        for rep in range(a.warmup + a.reps):
            for name in ("cpu", "calls", "handle"):   # the forms alternate rep by rep
                t0 = time.perf_counter()
                out = fns[name](K)
                dt = time.perf_counter() - t0
                if rep >= a.warmup:
                    times[name].append(dt * 1e6)
                if name != "cpu" and rep % 10 == 0:
                    assert same(out, want), (name, K, rep)
        for name, ts in times.items():
            result[f"{name}_k{K}_median_us"] = round(float(np.median(ts)), 1)
            result[f"{name}_k{K}_p90_us"] = round(float(np.percentile(ts, 90)), 1)
        result[f"matches_k{K}"] = [int(n) for n, _ in want[1]]
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
