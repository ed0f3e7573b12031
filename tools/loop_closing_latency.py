#!/usr/bin/env python3
"""Latency of LoopClosing's Sim3 matcher calls on resident key frames (not imported by bench.py): n_mp map points against K key frames of about
1000 features (synth.make_fuse_scene's defaults), timed three ways on the same inputs.

Search form -- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) for K targets, K = 1, 3, 8:
  * cpu:    the CPU oracle on one core, K times: the composed gates (tests/sim3_scene.py) and search_by_projection_window on the key frame's grid;
  * calls:  K x orbx_search_by_projection_window (host-pointer entry point: the key frame uploaded and its grid rebuilt per call) on PRE-PROJECTED
            queries -- the host projection is not timed, which favours this form;
  * sim3:   ONE orbx_keyframe_search_by_projection_sim3: projection on the device, everything timed.
Fuse form -- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) for K targets, K = 1, 8, 20, 40:
  * cpu:    the oracle's gates and its gate-less fuse_search, K times;
  * layer2: ONE orbx_keyframe_fuse_search(use_chi2 = 0) on the resident key frames with PRE-PROJECTED queries (projection not timed);
  * sim3:   ONE orbx_keyframe_fuse_map_points_sim3, everything timed.

The forms alternate repetition by repetition in one process; every output of every repetition is compared with the composed reference.  Prints one
JSON line (and writes it to --out): median and p90 in microseconds per form and K."""
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
    ap.add_argument("--search-ks", default="1,3,8")
    ap.add_argument("--fuse-ks", default="1,8,20,40")
    ap.add_argument("--n-mp", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sks = [int(k) for k in args.search_ks.split(",")]
    fks = [int(k) for k in args.fuse_ks.split(",")]
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    import sim3_scene as S
    import test_gpu_keyframe as T

    f32 = np.float32
    kmax = max(sks + fks)
    TH_S, RATIO, TH_F = 8.0, 1.5, 4.0          # LoopClosing.cc:964 (th 8, ratioHamming 1.5); SearchAndFuse's th = 4
    sc = synth.make_fuse_scene(np.random.default_rng(4040), kmax, args.n_mp)
    mp, log_sf = sc["map_points"], sc["log_scale_factor"]
    max_dist = float(f32(S.TH_LOW) * f32(RATIO))
    sref = S.search_reference(ob, sc, range(max(sks)), TH_S, RATIO, 0)
    fi, fd, _, frecs = S.fuse_reference(ob, sc, range(max(fks)), TH_F)
    views = [T._view(osa, sc, k, u_right=False) for k in range(kmax)]
    grids = [S.grid_of(ob, sc, k) for k in range(kmax)]
    m = osa.ORBmatcher(0.6, True)
    kfs = [osa.DeviceKeyFrame.from_host(m, v, None) for v in views]

    def cpu_search(K):
        out = []
        for k in range(K):
            ok, u, v, lvl, _ = S.gates(ob, sc, k, 0)
            sel = np.nonzero(ok)[0]
            q = dict(x=u[sel], y=v[sel], r=(f32(TH_S) * sc["scale_factors"][lvl[sel]]).astype(f32), min_level=(lvl[sel] - 1).astype(np.int32),
                     max_level=lvl[sel].astype(np.int32), desc=np.ascontiguousarray(mp["desc"][sel]))
            nm, mm = ob.search_by_projection_window(grids[k], views[k].descriptors, q, max_dist, False)
            out.append((nm, np.where(mm >= 0, sel[np.maximum(mm, 0)], -1)))
        return out

    def calls_search(K):
        out = []
        for k in range(K):
            sel, q = sref["recs"][k]
            nm, mm = m.SearchByProjectionWindow(views[k], q, max_dist, False)
            out.append((nm, np.where(mm >= 0, sel[np.maximum(mm, 0)], -1)))
        return out

    def sim3_search(K):
        nm, match, _, _ = m.SearchByProjectionSim3KeyFrames(kfs[:K], sc["cams"][:K], sc["poses"][:K], mp, TH_S, RATIO, log_sf, want_projected=False)
        return list(zip(nm, match))

    def cpu_fuse(K):
        out = []
        for k in range(K):
            ok, u, v, lvl, _ = S.gates(ob, sc, k, 0)
            sel = np.nonzero(ok)[0]
            q = dict(u=u[sel], v=v[sel], ur=np.zeros(len(sel), f32), r=(f32(TH_F) * sc["scale_factors"][lvl[sel]]).astype(f32),
                     level=lvl[sel].astype(np.int32), desc=np.ascontiguousarray(mp["desc"][sel]))
            out.append((sel,) + ob.fuse_search(grids[k], views[k].descriptors, None, None, q))
        return out

    def layer2_fuse(K):
        rows = m.FuseSearchKeyFrames(kfs[:K], [q for _, q in frecs[:K]], use_chi2=False)
        return [(frecs[k][0],) + rows[k] for k in range(K)]

    def sim3_fuse(K):
        bi, bd, _ = m.FuseMapPointsSim3(kfs[:K], sc["cams"][:K], sc["poses"][:K], mp, TH_F, log_sf, want_projected=False)
        return bi, bd

    def verify_search(name, K, out):
        for k, (nm, match) in enumerate(out):
            assert int(nm) == int(sref["nm"][k]) and np.array_equal(match, sref["match"][k]), (name, K, k)

    def verify_fuse(name, K, out):
        if name == "sim3":
            assert np.array_equal(out[0], fi[:K]) and np.array_equal(out[1], fd[:K]), (name, K)
        else:
            for k, (sel, bi, bd) in enumerate(out):
                assert np.array_equal(sel, frecs[k][0]) and np.array_equal(bi, fi[k, sel]) and np.array_equal(bd, fd[k, sel]), (name, K, k)

    groups = {"search": (sks, {"cpu": cpu_search, "calls": calls_search, "sim3": sim3_search}, verify_search),
              "fuse": (fks, {"cpu": cpu_fuse, "layer2": layer2_fuse, "sim3": sim3_fuse}, verify_fuse)}
    times = {g: {name: {K: [] for K in ks} for name in forms} for g, (ks, forms, _) in groups.items()}
    for rep in range(args.warmup + args.reps):
        for g, (ks, forms, verify) in groups.items():
            for K in ks:
                for name, fn in forms.items():   # the forms alternate repetition by repetition
                    t0 = time.perf_counter()
                    out = fn(K)                   # (every entry point synchronises before it returns)
                    dt = time.perf_counter() - t0
                    verify(name, K, out)
                    if rep >= args.warmup:
                        times[g][name][K].append(dt * 1e6)
    res = {"tool": "loop_closing_latency", "n_mp": args.n_mp, "reps": args.reps,
           "features_per_key_frame": int(np.mean([len(v.keypoints_un) for v in views])),
           "pairs_projected": float(sref["projected"].mean()), "pairs_matched": float(sref["nm"].sum()) / sref["projected"].size,
           "fuse_pairs_within_th_low": float((fd <= S.TH_LOW).mean())}
    for g, (ks, forms, _) in groups.items():
        for name in forms:
            for K in ks:
                a = np.array(times[g][name][K])
                res[f"{g}_{name}_k{K}_med_us"] = round(float(np.median(a)), 1)
                res[f"{g}_{name}_k{K}_p90_us"] = round(float(np.percentile(a, 90)), 1)
    med = lambda g, name, K: res[f"{g}_{name}_k{K}_med_us"]   # noqa: E731
    for K in sks:
        res[f"search_sim3_over_calls_k{K}"] = round(med("search", "sim3", K) / med("search", "calls", K), 3)
    for K in fks:
        res[f"fuse_sim3_over_layer2_k{K}"] = round(med("fuse", "sim3", K) / med("fuse", "layer2", K), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
