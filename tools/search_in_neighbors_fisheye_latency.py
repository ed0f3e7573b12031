#!/usr/bin/env python3
"""Latency of the Fuse loop of LocalMapping::SearchInNeighbors on a fisheye-stereo rig (not imported by bench.py): n_mp map points of the current key
frame fused into K target key frames of about 1000 + 1000 features -- per target Fuse(pKFi, vpMapPointMatches) and Fuse(pKFi, vpMapPointMatches, true)
-- for K = 1, 8, 20, 40, timed four ways on the same inputs:

  * cpu:     the CPU oracle on one core, 2 K times: the gates of ORBmatcher::Fuse (oracle is_in_frustum_checks + the strict image edge and the
             viewing-angle gate in float32 numpy) and fuse_search on that camera's grid;
  * calls:   2 K x orbx_fuse_search (host-pointer entry point: that camera's features uploaded and their grid rebuilt per call) on PRE-PROJECTED
             queries -- the projection (KannalaBrandt8::project on the host) is not timed, which favours this form;
  * layer2:  ONE orbx_keyframe_fuse_search_fisheye on K resident key frames, the same pre-projected queries (projection not timed);
  * layer3:  ONE orbx_keyframe_fuse_map_points_fisheye: projection on the device, everything timed.

The forms alternate repetition by repetition in one process; every output of every repetition is compared with the composed reference of
tests/test_gpu_keyframe_fisheye.py.  Prints one JSON line (and writes it to --out): median and p90 in microseconds per form and K, and the ratios
layer3(K=20) / calls(K=20), layer2(K=40) / layer2(K=1), layer3(K=40) / layer3(K=1), layer3(K=1) / calls(K=1)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="1,8,20,40")
    ap.add_argument("--n-mp", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(",")]
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    import test_gpu_keyframe_fisheye as T

    f32 = np.float32
    kmax = max(ks)
    sc = synth.make_fisheye_fuse_scene(np.random.default_rng(4040), kmax, args.n_mp, n_clutter=(490, 490))
    mp, isg, sf = sc["map_points"], sc["inv_level_sigma2"], sc["scale_factors"]
    want_i, want_d, want_p, recs, _ = T._reference(ob, sc, range(kmax))
    sides = [[T._side(sc, k, s) for s in (0, 1)] for k in range(kmax)]               # (keypoints, descriptor rows, index offset) per camera
    bnd = [[float(x) for x in sc["bounds"][k]] for k in range(kmax)]
    host = [[osa.FrameView(kps, desc, *bnd[k], sf) for kps, desc, _ in sides[k]] for k in range(kmax)]
    grids = [[ob.OracleGrid(kps, *bnd[k]) for kps, _, _ in sides[k]] for k in range(kmax)]
    qs = [tuple(q for _, q in recs[k]) for k in range(kmax)]
    m = osa.ORBmatcher(0.6, True)
    kfs = [T._host_kf(osa, m, sc, k) for k in range(kmax)]

    def cpu(K):
        out = []
        for k in range(K):
            b = sc["bounds"][k]
            for s in (0, 1):
                view = sc["views"][k][s]
                o = ob.is_in_frustum_checks(view, b, sc["log_scale_factor"], len(sf), -2.0, mp["pos"], mp["normal"], mp["min_dist"], mp["max_dist"])
                PO = mp["pos"] - view[2][None, :]
                z = f32(0)
                dot = ((z + PO[:, 0] * mp["normal"][:, 0]) + PO[:, 1] * mp["normal"][:, 1]) + PO[:, 2] * mp["normal"][:, 2]
                dist = np.sqrt(((z + PO[:, 0] * PO[:, 0]) + PO[:, 1] * PO[:, 1]) + PO[:, 2] * PO[:, 2])
                ok = (o["in_view"] == 1) & (o["proj_x"] != b[1]) & (o["proj_y"] != b[3]) & ~(dot.astype(np.float64) < 0.5 * dist.astype(np.float64))
                sel = np.nonzero(ok)[0]
                lv = o["level"][sel]
                q = dict(u=o["proj_x"][sel], v=o["proj_y"][sel], ur=np.zeros(len(sel), f32), r=(f32(T.TH) * sf[lv]).astype(f32), level=lv,
                         desc=mp["desc"][sel])
                bi, bd = ob.fuse_search(grids[k][s], sides[k][s][1], None, isg, q)
                out.append((sel, np.where(bi >= 0, bi + sides[k][s][2], -1), bd))
        return out

    def calls(K):
        out = []
        for k in range(K):
            for s in (0, 1):
                bi, bd = m.FuseSearch(host[k][s], qs[k][s], isg)
                out.append((np.where(bi >= 0, bi + sides[k][s][2], -1), bd))
        return out

    forms = {
        "cpu": cpu,
        "calls": calls,
        "layer2": lambda K: [row for pair in m.FuseSearchKeyFramesFisheye(kfs[:K], qs[:K]) for row in pair],
        "layer3": lambda K: m.FuseMapPointsFisheye(kfs[:K], sc["views"][:K], mp, T.TH, sc["log_scale_factor"]),
    }

    def verify(name, K, out):
        if name == "layer3":
            assert np.array_equal(out[0], want_i[:K]) and np.array_equal(out[1], want_d[:K]) and np.array_equal(out[2], want_p[:K]), (name, K)
            return
        assert len(out) == 2 * K
        for p, row in enumerate(out):
            k, s = divmod(p, 2)
            sel = recs[k][s][0]
            if name == "cpu":
                assert np.array_equal(row[0], sel), (name, K, k, s)
                row = row[1:]
            assert np.array_equal(row[0], want_i[k, s, sel]) and np.array_equal(row[1], want_d[k, s, sel]), (name, K, k, s)

    times = {name: {K: [] for K in ks} for name in forms}
    for rep in range(args.warmup + args.reps):
        for K in ks:
            for name, fn in forms.items():   # the forms alternate repetition by repetition
                t0 = time.perf_counter()
                out = fn(K)                   # (every entry point synchronises before it returns)
                dt = time.perf_counter() - t0
                verify(name, K, out)
                if rep >= args.warmup:
                    times[name][K].append(dt * 1e6)
    res = {"tool": "search_in_neighbors_fisheye_latency", "n_mp": args.n_mp, "reps": args.reps,
           "left_features_per_key_frame": int(np.mean([len(s[0][0]) for s in sides])),
           "right_features_per_key_frame": int(np.mean([len(s[1][0]) for s in sides])),
           "pairs_projected": float(want_p.mean()), "pairs_within_th_low": float((want_d <= T.TH_LOW).mean())}
    for name in forms:
        for K in ks:
            a = np.array(times[name][K])
            res[f"{name}_k{K}_med_us"] = round(float(np.median(a)), 1)
            res[f"{name}_k{K}_p90_us"] = round(float(np.percentile(a, 90)), 1)
    med = lambda name, K: res[f"{name}_k{K}_med_us"]   # noqa: E731
    if 20 in ks:
        res["layer3_k20_over_calls_k20"] = round(med("layer3", 20) / med("calls", 20), 3)
    if 1 in ks and 40 in ks:
        res["layer2_k40_over_k1"] = round(med("layer2", 40) / med("layer2", 1), 2)
        res["layer3_k40_over_k1"] = round(med("layer3", 40) / med("layer3", 1), 2)
    if 1 in ks:
        res["layer3_k1_over_two_calls"] = round(med("layer3", 1) / med("calls", 1), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
