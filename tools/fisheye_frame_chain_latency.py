#!/usr/bin/env python3
"""Latency of the per-frame tracking chain of a fisheye-stereo rig (TUM-VI-shaped: ~1000 + 1000 features, 10 000 local map points; not
imported by bench.py):

    M2 (TrackWithMotionModel, th) -> M2 at 2*th -> isInFrustumChecks x 2 (left, right) -> M1 (SearchLocalPoints)

timed three ways on the same inputs, the forms alternating chain by chain:
  * calls:  host-pointer entry points -- orbx_search_by_projection_frame_fisheye x 2, orbx_is_in_frustum_checks (both cameras) and
            orbx_search_by_projection_mappoints_fisheye (the projection records go to the host, become windows there and come back);
  * handle: orbx_frame_load_host_fisheye, orbx_frame_search_by_projection_frame_fisheye x 2, orbx_frame_search_local_points_fisheye;
  * oracle: the same chain on one CPU core of the oracle.
Every output is compared with the oracle's.  Also timed alone: one orbx_frame_search_local_points_fisheye call (against the oracle's
isInFrustumChecks x 2 + M1) and one host-pointer fisheye M1.  Prints one JSON line (median / p90 per form)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def stats(t):
    return {"median_us": round(float(np.median(t)), 1), "p90_us": round(float(np.percentile(t, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n-mp", type=int, default=10000)
    ap.add_argument("--th", type=float, default=7.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import orb_slam3_amd as osa
    from oracle import oracle_binding as ob
    from test_gpu_frame_fisheye import W, H, _features_at, _noisy
    from test_oracle_geometry import fisheye_case, fisheye_views
    rng = np.random.default_rng(5)
    c = fisheye_case(1, n=a.n_mp)
    views = fisheye_views(fisheye_case(1), "fisheye/1")
    nlevels = int(c["nl"])
    sf = np.array([1.2 ** i for i in range(nlevels)], np.float32)
    kl, kr, desc, l2r, r2l, mp_desc = _features_at(rng, ob, c, views, 1000, nlevels)
    nl, nr = len(kl), len(kr)
    # last-frame queries: left keypoints moved by a pixel or two, their right projections at the stereo partners
    q = dict(u=kl["x"] + rng.normal(0, 1.5, nl).astype(np.float32), v=kl["y"] + rng.normal(0, 1.5, nl).astype(np.float32),
             xr=np.where(l2r >= 0, kr["x"][np.maximum(l2r, 0)], -1000).astype(np.float32),
             yr=np.where(l2r >= 0, kr["y"][np.maximum(l2r, 0)], -1000).astype(np.float32), octave=kl["octave"].astype(np.int32),
             angle=kl["angle"], desc=_noisy(rng, desc[:nl], 0.05), has_obs=np.ones(nl, np.uint8))
    eligible = (rng.random(a.n_mp) < 0.9).astype(np.uint8)
    has_obs = np.ones(a.n_mp, np.uint8)
    m = osa.ORBmatcher(0.8, True)
    left = osa.FrameView(kl, desc, 0.0, float(W), 0.0, float(H), sf)
    D = osa.DeviceFrame(m, nl + nr)
    gl, gr = ob.OracleGrid(kl, 0.0, float(W), 0.0, float(H)), ob.OracleGrid(kr, 0.0, float(W), 0.0, float(H))
    args = (c["bounds"], c["lsf"], nlevels, c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"])

    def mp_of(pv):
        el = eligible.astype(bool)
        ivl, ivr = pv[0]["in_view"].astype(bool) & el, pv[1]["in_view"].astype(bool) & el
        mp = dict(in_view=ivl.astype(np.uint8), proj_x=pv[0]["proj_x"], proj_y=pv[0]["proj_y"], level=pv[0]["level"], view_cos=pv[0]["view_cos"],
                  in_view_r=ivr.astype(np.uint8), proj_xr=pv[1]["proj_x"], proj_yr=pv[1]["proj_y"], level_r=pv[1]["level"],
                  view_cos_r=pv[1]["view_cos"], desc=mp_desc, has_obs=has_obs)
        return mp, np.stack([ivl, ivr]).astype(np.uint8)

    def chain_oracle():
        r = [ob.search_by_projection_frame_fisheye(gl, gr, desc, sf, q, th, 0, True) for th in (a.th, 2 * a.th)]
        mp, iv = mp_of([ob.is_in_frustum_checks(views[s], *args) for s in (0, 1)])
        return r, iv, ob.search_by_projection_mappoints_fisheye(gl, gr, desc, sf, l2r, r2l, mp, 1.0, 0.8)

    def chain_calls():
        r = [m.SearchByProjectionFrameFisheye(left, kr, q, th, 0) for th in (a.th, 2 * a.th)]
        pv = m.isInFrustumChecks(views, *args)
        mp, iv = mp_of([{k: v[s] for k, v in pv.items()} for s in (0, 1)])
        return r, iv, m.SearchByProjectionFisheye(left, kr, l2r, r2l, mp, 1.0)

    def chain_handle():
        D.load_fisheye(left, kr, l2r, r2l)
        r = [m.SearchByProjectionFrameFisheye(D, None, q, th, 0) for th in (a.th, 2 * a.th)]
        n, fm, iv = m.SearchLocalPointsFisheye(D, views, c["lsf"], c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"], mp_desc, eligible, has_obs)
        return r, iv, (n, fm)

    want = chain_oracle()

    def check(res):
        r, iv, m1 = res
        for (n, cm), (on, ocm) in zip(r, want[0]):
            assert n == on and np.array_equal(np.maximum(cm, -1), np.maximum(ocm, -1)), "M2 differs from the oracle"
        assert np.array_equal(iv, want[1]), "in_view differs from the oracle"
        assert m1[0] == want[2][0] and np.array_equal(m1[1], want[2][1]), "M1 differs from the oracle"

    times = {"calls": [], "handle": [], "oracle_1core": [], "local_points_call": [], "local_points_oracle_1core": [], "host_m1_call": []}
    mp_host, _ = mp_of([ob.is_in_frustum_checks(views[s], *args) for s in (0, 1)])
    for i in range(a.warmup + a.chains):
        for form, fn in (("calls", chain_calls), ("handle", chain_handle), ("oracle_1core", chain_oracle)):
            if form == "oracle_1core" and i % 5:
                continue   # (the CPU chain is slow and deterministic: one in five chains)
            t0 = time.perf_counter()
            res = fn()
            dt = (time.perf_counter() - t0) * 1e6
            check(res)
            if i >= a.warmup:
                times[form].append(dt)
        t0 = time.perf_counter()
        n, fm, iv = m.SearchLocalPointsFisheye(D, views, c["lsf"], c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"], mp_desc, eligible, has_obs)
        t1 = time.perf_counter()
        hn, hfm = m.SearchByProjectionFisheye(left, kr, l2r, r2l, mp_host, 1.0)
        t2 = time.perf_counter()
        assert n == want[2][0] and np.array_equal(fm, want[2][1]) and hn == n and np.array_equal(hfm, fm)
        if i >= a.warmup:
            times["local_points_call"].append((t1 - t0) * 1e6)
            times["host_m1_call"].append((t2 - t1) * 1e6)
        if i >= a.warmup and i % 5 == 0:
            t0 = time.perf_counter()
            mp, _ = mp_of([ob.is_in_frustum_checks(views[s], *args) for s in (0, 1)])
            ob.search_by_projection_mappoints_fisheye(gl, gr, desc, sf, l2r, r2l, mp, 1.0, 0.8)
            times["local_points_oracle_1core"].append((time.perf_counter() - t0) * 1e6)
    out = {"chain": "M2 -> M2 at 2*th -> isInFrustumChecks x 2 (%d) -> M1 (%d), fisheye rig" % (a.n_mp, a.n_mp), "chains": a.chains,
           "features": [nl, nr], "m1_matches": int(want[2][0]), "oracle_checked": "every chain"}
    for form, t in times.items():
        out[form] = stats(t)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
