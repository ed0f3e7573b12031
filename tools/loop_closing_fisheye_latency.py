#!/usr/bin/env python3
"""Latency of LoopClosing's Sim3 matcher calls on FISHEYE-STEREO resident key frames (not imported by bench.py): tools/loop_closing_latency.py for
rigs.  n_mp map points against K rig key frames (synth.make_fisheye_fuse_scene's defaults), timed three ways on the same inputs; the members read the
left camera only.

Search form -- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) for K targets, K = 1, 3, 8:
  * cpu:    the CPU oracle on one core, K times: the composed gates (tests/sim3_fisheye_scene.py) and search_by_projection_window on the left grid;
  * calls:  K x orbx_search_by_projection_window on the LEFT camera's host arrays (today's path on a rig: the features uploaded and the grid rebuilt
            per call) on PRE-PROJECTED queries -- the host's KannalaBrandt8 projection is not timed, which favours this form;
  * sim3:   ONE orbx_keyframe_search_by_projection_sim3_fisheye: projection on the device, everything timed.
Fuse form -- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) for K targets, K = 1, 8, 20, 40:
  * cpu:    the oracle's gates and its gate-less fuse_search on the left features, K times;
  * calls:  K x orbx_fuse_search (gate-less, the left camera's host arrays) on PRE-PROJECTED queries (projection not timed);
  * sim3:   ONE orbx_keyframe_fuse_map_points_sim3_fisheye, everything timed.

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
    import sim3_fisheye_scene as S

    f32 = np.float32
    kmax = max(sks + fks)
    TH_S, RATIO, TH_F = 8.0, 1.5, 4.0          # LoopClosing.cc:964 (th 8, ratioHamming 1.5); SearchAndFuse's th = 4
    sc = synth.make_fisheye_fuse_scene(np.random.default_rng(4040), kmax, args.n_mp)
    mp, log_sf = sc["map_points"], sc["log_scale_factor"]
    max_dist = float(f32(S.TH_LOW) * f32(RATIO))
    sref = S.search_reference(ob, sc, range(max(sks)), TH_S, RATIO, 0)
    fi, fd, _, frecs = S.fuse_reference(ob, sc, range(max(fks)), TH_F)
    b = [float(x) for x in sc["bounds"][0]]
    views = [osa.FrameView(*S.left_side(sc, k)[:2], *b, sc["scale_factors"]) for k in range(kmax)]   # the left camera's host arrays
    grids = [S.grid_of(ob, sc, k) for k in range(kmax)]
    lv = S.left_views(sc, range(kmax))
    m = osa.ORBmatcher(0.6, True)
    kfs = [osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(sc["key_frames"][k]["kps_left"], sc["key_frames"][k]["desc"], *b, sc["scale_factors"]),
                                                sc["key_frames"][k]["kps_right"], None) for k in range(kmax)]
    nls = [S.left_side(sc, k)[2] for k in range(kmax)]

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
        nm, match, _, _ = m.SearchByProjectionSim3KeyFramesFisheye(kfs[:K], lv[:K], mp, TH_S, RATIO, log_sf, want_projected=False)
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

    def calls_fuse(K):
        return [(frecs[k][0],) + tuple(m.FuseSearch(views[k], frecs[k][1], None)) for k in range(K)]

    def sim3_fuse(K):
        bi, bd, _ = m.FuseMapPointsSim3Fisheye(kfs[:K], lv[:K], mp, TH_F, log_sf, want_projected=False)
        return bi, bd

    def verify_search(name, K, out):
        for k, (nm, match) in enumerate(out):   # (the resident form's rows span N_left + N_right, the others' N_left)
            want = sref["match"][k] if name == "sim3" else sref["match"][k][:nls[k]]
            assert int(nm) == int(sref["nm"][k]) and np.array_equal(match, want), (name, K, k)

    def verify_fuse(name, K, out):
        if name == "sim3":
            assert np.array_equal(out[0], fi[:K]) and np.array_equal(out[1], fd[:K]), (name, K)
        else:
            for k, (sel, bi, bd) in enumerate(out):
                assert np.array_equal(sel, frecs[k][0]) and np.array_equal(bi, fi[k, sel]) and np.array_equal(bd, fd[k, sel]), (name, K, k)

    groups = {"search": (sks, {"cpu": cpu_search, "calls": calls_search, "sim3": sim3_search}, verify_search),
              "fuse": (fks, {"cpu": cpu_fuse, "calls": calls_fuse, "sim3": sim3_fuse}, verify_fuse)}
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
    res = {"tool": "loop_closing_fisheye_latency", "n_mp": args.n_mp, "reps": args.reps,
           "left_features_per_key_frame": int(np.mean(nls)),
           "right_features_per_key_frame": int(np.mean([len(kf["kps_right"]) for kf in sc["key_frames"]])),
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
        res[f"fuse_sim3_over_calls_k{K}"] = round(med("fuse", "sim3", K) / med("fuse", "calls", K), 3)
    # the one call's median below the separate calls' median by more than the larger p90 - median spread of the two
    for g, K in (("search", 8), ("fuse", 20)):
        if K in groups[g][0]:
            spread = max(res[f"{g}_{n}_k{K}_p90_us"] - med(g, n, K) for n in ("sim3", "calls"))
            res[f"{g}_k{K}_gain_us"] = round(med(g, "calls", K) - med(g, "sim3", K), 1)
            res[f"{g}_k{K}_spread_us"] = round(spread, 1)
            res[f"{g}_k{K}_faster_beyond_spread"] = bool(med(g, "calls", K) - med(g, "sim3", K) > spread)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
