#!/usr/bin/env python3
"""Latency of the causal per-frame chain Tracking runs for every frame (not imported by bench.py):

    extract -> M2 (TrackWithMotionModel, th) -> M2 at 2*th -> isInFrustum (n_mp local map points) -> M1 (SearchLocalPoints)

timed two ways on the same inputs:
  * calls:  host-pointer entry points -- orbx_search_by_projection_frame x 2, orbx_is_in_frustum + orbx_search_by_projection_mappoints
            (the projection records go to the host, become search windows there and come back);
  * handle: orbx_frame_load_host once, orbx_frame_search_by_projection_frame x 2, orbx_frame_search_local_points (one call).
Every chain's outputs are compared with the CPU oracle's (computed once per input frame).  Prints one JSON line: the median and p90
of each form over --chains chains (the forms alternate chain by chain)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

W, H = 752, 480
CAM4 = (458.654, 457.296, 367.215, 248.375)


def scene(rng, ex, canvas, t, n_mp, synth):
    prev = synth.frame_from_canvas(canvas, 2 * t, W, H, 7000 + 2 * t)
    img = synth.frame_from_canvas(canvas, 2 * t + 1, W, H, 7001 + 2 * t)
    _, k0, d0 = ex(prev, None, (0, 1000))
    q = dict(u=k0["x"] - 2.0, v=k0["y"] - 1.0, ur=np.zeros(len(k0), np.float32), octave=k0["octave"], angle=k0["angle"], desc=d0,
             has_obs=(rng.random(len(k0)) < 0.9).astype(np.uint8))
    _, k, _ = ex(img, None, (0, 1000))
    fx, fy, cx, cy = CAM4
    src = rng.integers(0, len(k), n_mp)
    z = rng.uniform(1.0, 30.0, n_mp)
    pos = np.stack([(k["x"][src] - cx) / fx * z, (k["y"][src] - cy) / fy * z, z], axis=1)
    out = rng.random(n_mp) < 0.3
    pos[out] = rng.uniform(-20, 20, (out.sum(), 3))
    pos = pos.astype(np.float32)
    normal = pos / np.linalg.norm(pos, axis=1, keepdims=True) + rng.normal(0, 0.3, pos.shape)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    mx = (np.linalg.norm(pos, axis=1) * 1.2 ** k["octave"][src] * rng.uniform(0.9, 1.1, n_mp)).astype(np.float32)
    mn = (mx / 1.2 ** 7).astype(np.float32)
    return dict(img=img, q=q, pos=pos, normal=normal, mn=mn, mx=mx, eligible=(rng.random(n_mp) < 0.9).astype(np.uint8),
                has_obs=np.ones(n_mp, np.uint8), src=src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--n-mp", type=int, default=10000)
    ap.add_argument("--th", type=float, default=15.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    rng = np.random.default_rng(1)
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    m = osa.ORBmatcher(0.8, True)
    canvas = synth.make_canvas(1)
    sf = ex.GetScaleFactors()
    lsf = np.float32(np.log(np.float32(1.2)))
    Rcw, tcw = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    Ow = np.zeros(3, np.float32)
    cam10 = CAM4 + (0, 0, 0, 0, 0, 0.0)
    bounds = np.array([0.0, W, 0.0, H], np.float32)
    scenes = [scene(rng, ex, canvas, t, a.n_mp, synth) for t in range(a.frames)]
    want = []
    for s in scenes:   # the oracle's chain, once per input frame
        _, k, d = ex(s["img"], None, (0, 1000))
        grid = ob.OracleGrid(k, 0.0, float(W), 0.0, float(H))
        m2 = [ob.search_by_projection_frame(grid, d, sf, s["q"], th, 0, True, None, None) for th in (a.th, 2 * a.th)]
        fr = ob.is_in_frustum(Rcw, tcw, Ow, CAM4 + (0.0,), bounds, lsf, 8, 0.5, s["pos"], s["normal"], s["mn"], s["mx"])
        iv = fr["in_view"] & s["eligible"]
        mp = dict(proj_x=fr["proj_x"], proj_y=fr["proj_y"], proj_xr=fr["proj_xr"], level=fr["level"], view_cos=fr["view_cos"],
                  desc=_noisy(rng, d[s["src"]]), in_view=iv, has_obs=s["has_obs"])
        s["desc"] = mp["desc"]
        m1 = ob.search_by_projection_mappoints(grid, d, sf, mp, 1.0, 0.8)
        want.append(dict(m2=m2, iv=iv, m1=m1))
    D = osa.DeviceFrame(m, 2000)

    def chain_calls(s):
        _, k, d = ex(s["img"], None, (0, 1000))
        F = osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), sf)
        r = [m.SearchByProjectionFrame(F, s["q"], th, 0, None) for th in (a.th, 2 * a.th)]
        fr = m.isInFrustum(cam10, (Rcw, tcw, Ow), bounds, lsf, 8, 0.5, s["pos"], s["normal"], s["mn"], s["mx"])
        iv = fr["in_view"] & s["eligible"]
        mp = dict(proj_x=fr["proj_x"], proj_y=fr["proj_y"], proj_xr=fr["proj_xr"], level=fr["level"], view_cos=fr["view_cos"], desc=s["desc"],
                  in_view=iv, has_obs=s["has_obs"])
        return r, iv, m.SearchByProjection(F, mp, 1.0, None)

    def chain_handle(s):
        _, k, d = ex(s["img"], None, (0, 1000))
        D.load(osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), sf))
        r = [m.SearchByProjectionFrame(D, s["q"], th, 0, None) for th in (a.th, 2 * a.th)]
        n, fm, iv = m.SearchLocalPoints(D, cam10, (Rcw, tcw, Ow), lsf, 0.5, s["pos"], s["normal"], s["mn"], s["mx"], s["desc"], s["eligible"],
                                        s["has_obs"], 1.0)
        return r, iv, (n, fm)

    def check(res, w):
        r, iv, m1 = res
        for (n, cm), (on, ocm) in zip(r, w["m2"]):
            assert n == on and np.array_equal(cm, ocm), "M2 differs from the oracle"
        assert np.array_equal(iv, w["iv"]), "in_view differs from the oracle"
        assert m1[0] == w["m1"][0] and np.array_equal(m1[1], w["m1"][1]), "M1 differs from the oracle"

    times = {"calls": [], "handle": []}
    for i in range(a.warmup + a.chains):
        for form, fn in (("calls", chain_calls), ("handle", chain_handle)):
            s = scenes[i % len(scenes)]
            t0 = time.perf_counter()
            res = fn(s)
            dt = (time.perf_counter() - t0) * 1e6
            check(res, want[i % len(scenes)])
            if i >= a.warmup:
                times[form].append(dt)
    out = {"chain": "extract -> M2 -> M2 at 2*th -> isInFrustum (%d) -> M1 (%d)" % (a.n_mp, a.n_mp), "chains": a.chains, "frames": a.frames,
           "features": [int(len(ex(s["img"], None, (0, 1000))[1])) for s in scenes], "oracle_checked": "every chain"}
    for form, t in times.items():
        out[form] = {"median_us": round(float(np.median(t)), 1), "p90_us": round(float(np.percentile(t, 90)), 1), "min_us": round(float(np.min(t)), 1)}
    out["saved_us"] = round(out["calls"]["median_us"] - out["handle"]["median_us"], 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


def _noisy(rng, d):
    return d ^ np.packbits(rng.random((len(d), 256)) < 0.05, axis=1, bitorder="little")


if __name__ == "__main__":
    main()
