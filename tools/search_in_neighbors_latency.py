#!/usr/bin/env python3
"""Latency of the Fuse loop of LocalMapping::SearchInNeighbors (not imported by bench.py): n_mp map points of the current key frame fused into K
target key frames of about 1000 features, for K = 1, 8, 20, 40, timed four ways on the same inputs:

  * cpu:     the CPU oracle on one core, K times: the gates of ORBmatcher::Fuse (oracle is_in_frustum + the strict image edge and the viewing-angle
             gate in float32 numpy) and fuse_search on the key frame's grid;
  * calls:   K x orbx_fuse_search (host-pointer entry point: the key frame uploaded and its grid rebuilt per call) on PRE-PROJECTED queries -- the
             projection is not timed, which favours this form;
  * layer2:  ONE orbx_keyframe_fuse_search on K resident key frames, the same pre-projected queries (projection not timed);
  * layer3:  ONE orbx_keyframe_fuse_map_points: projection on the device, everything timed.

The forms alternate repetition by repetition in one process; every output of every repetition is compared with the composed reference of
tests/test_gpu_keyframe.py.  Prints one JSON line (and writes it to --out): median and p90 in microseconds per form and K, and the ratios
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
    from oracle import oracle_binding as ob
    import test_gpu_keyframe as T

    f32 = np.float32
    kmax = max(ks)
    sc = T._scene(4040, kmax, args.n_mp)
    mp, isg, sf = sc["map_points"], sc["inv_level_sigma2"], sc["scale_factors"]
    want_i, want_d, want_p, recs, _ = T._reference(ob, sc, range(kmax))
    views = [T._view(osa, sc, k) for k in range(kmax)]
    qs = [q for _, q in recs]
    grids = [ob.OracleGrid(v.keypoints_un, v.min_x, v.max_x, v.min_y, v.max_y) for v in views]
    m = osa.ORBmatcher(0.6, True)
    kfs = [osa.DeviceKeyFrame.from_host(m, v, isg) for v in views]

    def cpu(K):
        out = []
        for k in range(K):
            Rcw, tcw, Ow = sc["poses"][k]
            cam, b = sc["cams"][k], sc["bounds"][k]
            o = ob.is_in_frustum(Rcw, tcw, Ow, (cam[0], cam[1], cam[2], cam[3], cam[9]), b, sc["log_scale_factor"], len(sf), -2.0, mp["pos"],
                                 mp["normal"], mp["min_dist"], mp["max_dist"])
            PO = mp["pos"] - Ow[None, :]
            z = f32(0)
            dot = ((z + PO[:, 0] * mp["normal"][:, 0]) + PO[:, 1] * mp["normal"][:, 1]) + PO[:, 2] * mp["normal"][:, 2]
            dist = np.sqrt(((z + PO[:, 0] * PO[:, 0]) + PO[:, 1] * PO[:, 1]) + PO[:, 2] * PO[:, 2])
            ok = (o["in_view"] == 1) & (o["proj_x"] != b[1]) & (o["proj_y"] != b[3]) & ~(dot.astype(np.float64) < 0.5 * dist.astype(np.float64))
            sel = np.nonzero(ok)[0]
            lv = o["level"][sel]
            q = dict(u=o["proj_x"][sel], v=o["proj_y"][sel], ur=o["proj_xr"][sel], r=(f32(T.TH) * sf[lv]).astype(f32), level=lv, desc=mp["desc"][sel])
            out.append((sel,) + ob.fuse_search(grids[k], views[k].descriptors, views[k].u_right, isg, q))
        return out

    def check_rows(K, rows, what):
        for k in range(K):
            sel = recs[k][0]
            assert np.array_equal(rows[k][0], want_i[k, sel]) and np.array_equal(rows[k][1], want_d[k, sel]), (what, K, k)

    forms = {
        "cpu": cpu,
        "calls": lambda K: [m.FuseSearch(views[k], qs[k], isg) for k in range(K)],
        "layer2": lambda K: m.FuseSearchKeyFrames(kfs[:K], qs[:K]),
        "layer3": lambda K: m.FuseMapPoints(kfs[:K], sc["cams"][:K], sc["poses"][:K], mp, T.TH, sc["log_scale_factor"]),
    }

    def verify(name, K, out):
        if name == "cpu":
            for k, (sel, bi, bd) in enumerate(out):
                assert np.array_equal(sel, recs[k][0]) and np.array_equal(bi, want_i[k, sel]) and np.array_equal(bd, want_d[k, sel]), (name, K, k)
        elif name == "layer3":
            assert np.array_equal(out[0], want_i[:K]) and np.array_equal(out[1], want_d[:K]) and np.array_equal(out[2], want_p[:K]), (name, K)
        else:
            check_rows(K, out, name)

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
    res = {"tool": "search_in_neighbors_latency", "n_mp": args.n_mp, "reps": args.reps,
           "features_per_key_frame": int(np.mean([len(v.keypoints_un) for v in views])),
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
        res["layer3_k1_over_one_call"] = round(med("layer3", 1) / med("calls", 1), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
