#!/usr/bin/env python3
"""Latency of the BoW-guided matchers with resident key frames against today's entry points (not imported by bench.py).  Three cases, each timed on
the same inputs in one process, the forms alternating repetition by repetition:

  frame          SearchByBoW(pKF_k, F) of a resident frame (loaded, BoW computed: not timed) against K = 1, 8, 32 candidates
                   cpu:      K x the CPU oracle's search_by_bow_frame, one core
                   host:     ONE orbx_frame_search_by_bow, the key frames as host arrays (descriptors, angles, flags, FeatureVector uploaded)
                   resident: ONE orbx_frame_search_by_bow_resident on DeviceKeyFrames with BoW (flags and records uploaded)
  keyframes      SearchByBoW(pKF1, pKF2_k) of one key frame against K = 1, 8, 32 key frames
                   cpu:      K x the oracle's search_by_bow_keyframes
                   host:     K x orbx_search_by_bow_keyframes (both sides uploaded per call)
                   resident: ONE orbx_keyframe_search_by_bow
  triangulation  one SearchForTriangulation between two pinhole key frames, both gates on the device
                   cpu:      the oracle's search_for_triangulation_pinhole
                   host:     orbx_search_for_triangulation_pinhole
                   resident: orbx_keyframe_search_for_triangulation

Every output of every repetition of the two device forms is compared with the oracle's.  Each case runs in a child process of its own under a time
limit of its own (--case-timeout); the first case that fails or runs out of time ends the run.  Prints one JSON line with the median and p90
(microseconds) of each form and writes it to --out (profiles/keyframe_bow.json by default)."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

W, H = 752, 480
CASES = ("frame", "keyframes", "triangulation")


def featvec(osa, node, kept):
    nk = node[kept]
    order = np.argsort(nk, kind="stable")
    nodes, starts = np.unique(nk[order], return_index=True)
    fv = osa.FeatureVector.__new__(osa.FeatureVector)
    fv.node_id = nodes.astype(np.uint32)
    fv.node_ptr = np.append(starts, len(order)).astype(np.int32)
    fv.index = kept[order].astype(np.int32)
    return fv


def timed(fns, want_of, same, reps, warmup):
    """fns: name -> callable; every output of every repetition of a device form is compared with want_of()."""
    want = want_of()
    times = {name: [] for name in fns}
    for rep in range(warmup + reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                times[name].append(dt * 1e6)
            if name != "cpu":
                assert same(out, want), (name, rep)
    return {name: (round(float(np.median(ts)), 1), round(float(np.percentile(ts, 90)), 1)) for name, ts in times.items()}


def run_case(case, a):
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    from test_gpu_matcher import _random_vocabulary

    rng = np.random.default_rng(3)
    canvas = synth.make_canvas(1)
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    frames = [ex(synth.frame_from_canvas(canvas, t, W, H, 1000 + t), None, (0, 1000)) for t in range(6)]
    sf = ex.GetScaleFactors()
    sg = (sf * sf).astype(np.float32)
    isg = (np.float32(1.0) / sg).astype(np.float32)
    # the vocabulary of tools/relocalization_latency.py: k = 10, L = 4, node descriptors sampled from the frames' descriptors, ~5 % stop words
    cp, ci, nd, wi = _random_vocabulary(rng, 10, 4, ragged=False)
    pool = np.concatenate([f[2] for f in frames])
    nd = pool[rng.integers(0, len(pool), len(nd))] ^ np.packbits(rng.random((len(nd), 256)) < 0.03, axis=1, bitorder="little")
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.05] = 0.0
    voc = osa.ORBVocabulary(4, cp, ci, nd, wi).set_word_weights(weights)
    levelsup = 2

    def cpu_fv(desc):
        w, node = ob.bow_transform(cp, ci, nd, wi, 4, levelsup, desc)
        return featvec(osa, node, np.nonzero(weights[w] > 0)[0])

    m = osa.ORBmatcher(0.75, True)
    # key frames: the other five frames (related) and random ones (unrelated), 80 % of their features with a map point; host arrays and resident
    kfs = []
    for j in range(32):
        k = frames[(j // 2) % 5][1] if j % 2 == 0 else frames[j % 5][1]
        d = frames[(j // 2) % 5][2] if j % 2 == 0 else rng.integers(0, 256, (len(k), 32), dtype=np.uint8)
        dev = osa.DeviceKeyFrame.from_host(m, osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), sf), isg)
        dev.compute_bow(m, voc, levelsup, download=False)
        kfs.append(dict(k=k, d=d, ang=np.ascontiguousarray(k["angle"]), valid=(rng.random(len(k)) < 0.8).astype(np.uint8), fv=cpu_fv(d), dev=dev))
    rows_same = lambda x, y: len(x) == len(y) and all(int(n1) == int(n2) and np.array_equal(r1, r2) for (n1, r1), (n2, r2) in zip(x, y))   # noqa: E731
    result = {"case": case, "reps": a.reps, "key_frame_features": int(np.mean([len(q["d"]) for q in kfs]))}
    ks = [int(x) for x in a.ks.split(",")]

    if case == "frame":
        _, kc, dc = frames[5]
        D = osa.DeviceFrame(m, 2000).load(osa.FrameView(kc, dc, 0.0, float(W), 0.0, float(H), sf))
        D.compute_bow(voc, levelsup, download=False)
        fv_f = cpu_fv(dc)
        result["frame_features"] = int(len(kc))
        for K in ks:
            sub = kfs[:K]
            host_args = [(q["d"], q["ang"], q["valid"], q["fv"]) for q in sub]
            devs, valid = [q["dev"] for q in sub], [q["valid"] for q in sub]

            def cpu():
                return [ob.search_by_bow_frame(q["d"], q["ang"], q["valid"], q["fv"], dc, kc["angle"], fv_f, 0.75, True) for q in sub]

            def host():
                nm, match = m.SearchByBoWDevice(D, host_args)
                return list(zip(nm, match))

            def resident():
                nm, match = m.SearchByBoWResident(D, devs, valid)
                return list(zip(nm, match))

            for name, (med, p90) in timed(dict(cpu=cpu, host=host, resident=resident), cpu, rows_same, a.reps, a.warmup).items():
                result[f"{name}_k{K}_median_us"], result[f"{name}_k{K}_p90_us"] = med, p90
            result[f"matches_k{K}"] = [int(n) for n, _ in cpu()]
    elif case == "keyframes":
        one = kfs[0]
        for K in ks:
            sub = [kfs[(j + 2) % 32] for j in range(K)]   # (from key frame 2 on: another view of the scene first)
            devs, valid = [q["dev"] for q in sub], [q["valid"] for q in sub]

            def cpu():
                return [ob.search_by_bow_keyframes(one["d"], one["ang"], one["valid"], one["fv"], q["d"], q["ang"], q["valid"], q["fv"], 0.75, True) for q in sub]

            def host():
                return [m.SearchByBoWKeyFrames(one["d"], one["ang"], one["valid"], one["fv"], q["d"], q["ang"], q["valid"], q["fv"]) for q in sub]

            def resident():
                nm, m12 = m.SearchByBoWKeyFramesResident(one["dev"], devs, one["valid"], valid)
                return list(zip(nm, m12))

            for name, (med, p90) in timed(dict(cpu=cpu, host=host, resident=resident), cpu, rows_same, a.reps, a.warmup).items():
                result[f"{name}_k{K}_median_us"], result[f"{name}_k{K}_p90_us"] = med, p90
            result[f"matches_k{K}"] = [int(n) for n, _ in cpu()]
    else:
        q1, q2 = kfs[0], kfs[2]
        skip1 = (rng.random(len(q1["d"])) < 0.3).astype(np.uint8)
        skip2 = (rng.random(len(q2["d"])) < 0.3).astype(np.uint8)
        Kc = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]])
        t = np.array([0.11, 0.004, 0.01])
        th = 0.01
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        F12 = (np.linalg.inv(Kc).T @ tx @ R @ np.linalg.inv(Kc)).astype(np.float32)
        ep = (410.0, 236.0)
        m6 = osa.ORBmatcher(0.6, True)

        def cpu():
            return [ob.search_for_triangulation_pinhole(q1["k"], q1["d"], skip1, None, q1["fv"], q2["k"], q2["d"], skip2, None, q2["fv"], sf, sg, F12, ep, False, True)]

        def host():
            return [m6.SearchForTriangulationPinhole(q1["k"], q1["d"], skip1, q1["fv"], q2["k"], q2["d"], skip2, q2["fv"], sf, sg, F12, ep)]

        def resident():
            return [m6.SearchForTriangulationResident(q1["dev"], q2["dev"], skip1, skip2, sg, F12, ep)]

        for name, (med, p90) in timed(dict(cpu=cpu, host=host, resident=resident), cpu, rows_same, a.reps, a.warmup).items():
            result[f"{name}_median_us"], result[f"{name}_p90_us"] = med, p90
        result["matches"] = int(cpu()[0][0])
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keyframe_bow.json"))
    ap.add_argument("--case", default="", help="run one case in this process (what the driver starts per case)")
    ap.add_argument("--case-timeout", type=int, default=240, help="seconds each case's process may take")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a)
        return 0
    out = {}
    for case in CASES:   # a fresh process per case, each under its own time limit; nothing more is started after a failure
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case, "--reps", str(a.reps), "--warmup", str(a.warmup), "--ks", a.ks]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.case_timeout)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {a.case_timeout} s", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{case}: exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}", file=sys.stderr)
            return 1
        out[case] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
