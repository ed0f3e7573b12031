#!/usr/bin/env python3
"""Latency of the BoW-guided matchers with resident FISHEYE-STEREO key frames against today's entry points (not imported by bench.py).  A
TUM-VI-shaped rig: frames and key frames of about 1000 + 1000 features, the vocabulary shape of tools/keyframe_bow_latency.py.  Three cases, each timed
on the same inputs, the forms alternating repetition by repetition:

  frame          SearchByBoW(pKF_k, F), F.Nleft != -1, of a resident rig frame (loaded, BoW computed: not timed) against K = 1, 8, 32 candidates
                   cpu:      K x the CPU oracle's search_by_bow_frame_fisheye, one core
                   host:     ONE orbx_frame_search_by_bow_fisheye, the key frames as host arrays
                   resident: ONE orbx_frame_search_by_bow_resident_fisheye on rig DeviceKeyFrames with BoW
  keyframes      SearchByBoW(pKF1, pKF2_k) between rig key frames (left cameras only) against K = 1, 8, 32 key frames
                   cpu:      K x the oracle's search_by_bow_keyframes with the right camera's features masked
                   host:     K x orbx_search_by_bow_keyframes with the same masks (both sides uploaded per call)
                   resident: ONE orbx_keyframe_search_by_bow_fisheye
  triangulation  one SearchForTriangulation between two rig key frames looking at common points, KannalaBrandt8::epipolarConstrain on the device
                   cpu:      the oracle's search_for_triangulation_kb8
                   host:     orbx_search_for_triangulation_kb8
                   resident: orbx_keyframe_search_for_triangulation_fisheye

Every output of every repetition of the two device forms is compared with the oracle's.  The measurement is ONE child process under one time limit
(--timeout); a failure or the limit ends the run.  Prints one JSON line with the median and p90 (microseconds) of each form and writes it to --out
(profiles/keyframe_bow_fisheye.json by default)."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

W, H = 752, 480


def measure(a):
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    from keyframe_bow_latency import featvec, timed
    from test_gpu_matcher import _random_vocabulary

    rng = np.random.default_rng(3)
    canvas = synth.make_canvas(1)
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    frames = [ex(synth.frame_from_canvas(canvas, t, W, H, 1000 + t), None, (0, 1000)) for t in range(7)]   # frame t + 1 plays frame t's right camera
    sf = ex.GetScaleFactors()
    sg = (sf * sf).astype(np.float32)
    isg = (np.float32(1.0) / sg).astype(np.float32)
    tri = synth.make_fisheye_keyframes(rng, 1450)                                                          # two key frames of about 2000 features
    # the vocabulary of tools/keyframe_bow_latency.py: k = 10, L = 4, node descriptors sampled from the descriptors at hand, ~5 % stop words
    cp, ci, nd, wi = _random_vocabulary(rng, 10, 4, ragged=False)
    pool = np.concatenate([f[2] for f in frames] + [np.asarray(tri[2]).reshape(-1, 32), np.asarray(tri[6]).reshape(-1, 32)])
    nd = pool[rng.integers(0, len(pool), len(nd))] ^ np.packbits(rng.random((len(nd), 256)) < 0.03, axis=1, bitorder="little")
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.05] = 0.0
    voc = osa.ORBVocabulary(4, cp, ci, nd, wi).set_word_weights(weights)
    levelsup = 2

    def cpu_fv(desc):
        w, node = ob.bow_transform(cp, ci, nd, wi, 4, levelsup, desc)
        return featvec(osa, node, np.nonzero(weights[w] > 0)[0])

    def rig_kf(m, kl, kr, d, valid):
        view = osa.FrameView(kl, d, 0.0, float(W), 0.0, float(H), sf)
        dev = osa.DeviceKeyFrame.from_host_fisheye(m, view, kr, isg)
        dev.compute_bow_fisheye(m, voc, levelsup, download=False)
        k = np.concatenate([kl, kr])
        left = valid.copy()
        left[len(kl):] = 0                                  # SearchByBoW(pKF1, pKF2) skips the right camera's features
        return dict(k=k, nl=len(kl), d=d, ang=np.ascontiguousarray(k["angle"]), valid=valid, left=left, fv=cpu_fv(d), dev=dev, view=view, kr=kr)

    m = osa.ORBmatcher(0.75, True)
    # key frames: pairs of the first six frames (related) and random descriptors (unrelated), 80 % of their features with a map point
    kfs = []
    for j in range(32):
        (_, kl, dl), (_, kr, dr) = frames[(j // 2) % 5], frames[(j // 2) % 5 + 1]
        d = np.concatenate([dl, dr]).reshape(-1, 32) if j % 2 == 0 else rng.integers(0, 256, (len(kl) + len(kr), 32), dtype=np.uint8)
        kfs.append(rig_kf(m, kl, kr, d, (rng.random(len(d)) < 0.8).astype(np.uint8)))
    rows_same = lambda x, y: len(x) == len(y) and all(int(n1) == int(n2) and np.array_equal(r1, r2) for (n1, r1), (n2, r2) in zip(x, y))   # noqa: E731
    out = {"reps": a.reps, "key_frame_features": int(np.mean([len(q["d"]) for q in kfs]))}
    ks = [int(x) for x in a.ks.split(",")]

    # ---- frame against K candidates ----
    res = out["frame"] = {}
    (_, kl, dl), (_, kr, dr) = frames[5], frames[6]
    dc = np.concatenate([dl, dr]).reshape(-1, 32)
    angc = np.concatenate([kl["angle"], kr["angle"]]).astype(np.float32)
    D = osa.DeviceFrame(m, 2200).load_fisheye(osa.FrameView(kl, dc, 0.0, float(W), 0.0, float(H), sf), kr, np.full(len(kl), -1, np.int32),
                                              np.full(len(kr), -1, np.int32))
    D.compute_bow_fisheye(voc, levelsup, download=False)
    fv_f = cpu_fv(dc)
    res["frame_features"] = [int(len(kl)), int(len(kr))]
    for K in ks:
        sub = kfs[:K]
        host_args = [(q["d"], q["ang"], q["valid"], q["fv"]) for q in sub]
        devs, valid = [q["dev"] for q in sub], [q["valid"] for q in sub]

        def cpu():
            return [ob.search_by_bow_frame_fisheye(q["d"], q["ang"], q["valid"], q["fv"], dc, angc, len(kl), fv_f, 0.75, True) for q in sub]

        def host():
            return list(zip(*m.SearchByBoWDeviceFisheye(D, host_args)))

        def resident():
            return list(zip(*m.SearchByBoWResidentFisheye(D, devs, valid)))

        for name, (med, p90) in timed(dict(cpu=cpu, host=host, resident=resident), cpu, rows_same, a.reps, a.warmup).items():
            res[f"{name}_k{K}_median_us"], res[f"{name}_k{K}_p90_us"] = med, p90
        res[f"matches_k{K}"] = [int(n) for n, _ in cpu()]

    # ---- key frame against K key frames ----
    res = out["keyframes"] = {}
    one = kfs[0]
    for K in ks:
        sub = [kfs[(j + 2) % 32] for j in range(K)]   # (from key frame 2 on: another view of the scene first)
        devs, valid = [q["dev"] for q in sub], [q["valid"] for q in sub]

        def cpu():
            return [ob.search_by_bow_keyframes(one["d"], one["ang"], one["left"], one["fv"], q["d"], q["ang"], q["left"], q["fv"], 0.75, True) for q in sub]

        def host():
            return [m.SearchByBoWKeyFrames(one["d"], one["ang"], one["left"], one["fv"], q["d"], q["ang"], q["left"], q["fv"]) for q in sub]

        def resident():
            return list(zip(*m.SearchByBoWKeyFramesResidentFisheye(one["dev"], devs, one["valid"], valid)))

        for name, (med, p90) in timed(dict(cpu=cpu, host=host, resident=resident), cpu, rows_same, a.reps, a.warmup).items():
            res[f"{name}_k{K}_median_us"], res[f"{name}_k{K}_p90_us"] = med, p90
        res[f"matches_k{K}"] = [int(n) for n, _ in cpu()]

    # ---- one KB8 triangulation call ----
    res = out["triangulation"] = {}
    k1, nl1, d1, _, k2, nl2, d2, _, R12, t12, cams = tri
    d1, d2 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32), np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
    sg8 = (np.array([1.2 ** i for i in range(8)], np.float32) ** 2).astype(np.float32)
    q1 = rig_kf(m, k1[:nl1], k1[nl1:], d1, np.ones(len(d1), np.uint8))
    q2 = rig_kf(m, k2[:nl2], k2[nl2:], d2, np.ones(len(d2), np.uint8))
    skip1 = (rng.random(len(d1)) < 0.2).astype(np.uint8)
    skip2 = (rng.random(len(d2)) < 0.2).astype(np.uint8)
    m6 = osa.ORBmatcher(0.6, True)
    res["features"] = [int(len(d1)), int(len(d2))]

    def cpu():
        return [ob.search_for_triangulation_kb8(k1, nl1, d1, skip1, q1["fv"], k2, nl2, d2, skip2, q2["fv"], sg8, sg8, cams, cams, R12, t12, False, True)]

    def host():
        return [m6.SearchForTriangulationKB8(k1, nl1, d1, skip1, q1["fv"], k2, nl2, d2, skip2, q2["fv"], sg8, sg8, cams, cams, R12, t12, False)]

    def resident():
        return [m6.SearchForTriangulationResidentKB8(q1["dev"], q2["dev"], skip1, skip2, sg8, sg8, cams, cams, R12, t12, False)]

    for name, (med, p90) in timed(dict(cpu=cpu, host=host, resident=resident), cpu, rows_same, a.reps, a.warmup).items():
        res[f"{name}_median_us"], res[f"{name}_p90_us"] = med, p90
    res["matches"] = int(cpu()[0][0])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keyframe_bow_fisheye.json"))
    ap.add_argument("--measure", action="store_true", help="measure in this process (what the driver starts)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring process may take")
    a = ap.parse_args()
    if a.measure:
        measure(a)
        return 0
    cmd = [sys.executable, str(Path(__file__).resolve()), "--measure", "--reps", str(a.reps), "--warmup", str(a.warmup), "--ks", a.ks]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.timeout} s", file=sys.stderr)
        return 1
    if r.returncode != 0:
        print(f"exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}", file=sys.stderr)
        return 1
    line = r.stdout.strip().splitlines()[-1]
    json.loads(line)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
