"""Fisheye-stereo frames on the device-resident frame handle (orbx_frame_load_host_fisheye / orbx_frame_load_stereo_fisheye_batch and the handle
forms of the fisheye M1 / M2 and SearchLocalPoints).  Every result is compared bit for bit with the host-pointer fisheye forms and the CPU oracle
(search_by_projection_{mappoints,frame}_fisheye, is_in_frustum_checks).  Features [0, N_left) are the left camera's, [N_left, N) the right one's."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = 512, 512
SF = np.array([1.2 ** i for i in range(8)], np.float32)


def _noisy(rng, d, p):
    return d ^ np.packbits(rng.random((len(d), 256)) < p, axis=1, bitorder="little")


def _kps(rng, n, packed=False):
    import orb_slam3_amd as osa
    k = np.zeros(n, osa.KP_DTYPE)
    k["octave"] = rng.integers(0, 3 if packed else 8, n)
    sc = (1.2 ** k["octave"]).astype(np.float32)
    if packed:   # a few hundred features in a small region: long contention chains
        k["x"] = rng.uniform(200, 260, n).astype(np.float32)
        k["y"] = rng.uniform(200, 250, n).astype(np.float32)
    else:
        k["x"] = (rng.uniform(10, W - 10, n) / sc).round().astype(np.float32) * sc
        k["y"] = (rng.uniform(10, H - 10, n) / sc).round().astype(np.float32) * sc
    k["size"] = 31.0 * sc
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.integers(7, 200, n).astype(np.float32)
    k["class_id"] = -1
    return k


def _rig_frame(rng, nl, nr, packed=False, n_pairs=None):
    """A rig frame: left / right keypoints, descriptors of all N rows (right rows near-copies of their partners), l2r / r2l."""
    kl, kr = _kps(rng, nl, packed), _kps(rng, nr, packed)
    if packed:
        protos = rng.integers(0, 256, (6, 32), dtype=np.uint8)
        dl, dr = _noisy(rng, protos[rng.integers(0, 6, nl)], 0.08), _noisy(rng, protos[rng.integers(0, 6, nr)], 0.08)
    else:
        dl, dr = rng.integers(0, 256, (nl, 32), dtype=np.uint8), rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    l2r, r2l = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
    k = min(nl, nr) if n_pairs is None else min(nl, nr, n_pairs)
    if k:
        il, ir = rng.permutation(nl)[:k], rng.permutation(nr)[:k]
        l2r[il], r2l[ir] = ir, il
        dr[ir] = _noisy(rng, dl[il], 0.03)
    return kl, kr, np.concatenate([dl, dr]).reshape(-1, 32), l2r, r2l


def _left_view(kl, desc):
    import orb_slam3_amd as osa
    return osa.FrameView(kl, desc, 0.0, float(W), 0.0, float(H), SF)


def _grids(oracle, kl, kr):
    return oracle.OracleGrid(kl, 0.0, float(W), 0.0, float(H)), oracle.OracleGrid(kr, 0.0, float(W), 0.0, float(H))


def _mp(rng, kl, kr, desc, n_mp, noise=2.0):
    nl, nr = len(kl), len(kr)
    src = rng.integers(0, max(nl, 1), n_mp)
    srcr = rng.integers(0, max(nr, 1), n_mp)
    kls = kl[src] if nl else np.zeros(n_mp, kl.dtype)
    krs = kr[srcr] if nr else np.zeros(n_mp, kr.dtype)
    level = kls["octave"].astype(np.int32)       # (levels out of range: test_levels_out_of_range_drop_that_camera)
    level_r = np.where(rng.random(n_mp) < 0.9, krs["octave"], -1).astype(np.int32)
    dsrc = desc[src] if nl else rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    return dict(in_view=(rng.random(n_mp) < 0.8).astype(np.uint8), proj_x=kls["x"] + rng.normal(0, noise, n_mp).astype(np.float32),
                proj_y=kls["y"] + rng.normal(0, noise, n_mp).astype(np.float32), level=level,
                view_cos=rng.choice(np.array([0.99, 0.998, np.nextafter(np.float32(0.998), np.float32(1)), 0.9995], np.float32), n_mp),
                in_view_r=(rng.random(n_mp) < 0.7).astype(np.uint8), proj_xr=krs["x"] + rng.normal(0, noise, n_mp).astype(np.float32),
                proj_yr=krs["y"] + rng.normal(0, noise, n_mp).astype(np.float32), level_r=level_r,
                view_cos_r=rng.choice(np.array([0.99, 0.9995], np.float32), n_mp), desc=_noisy(rng, dsrc, 0.05),
                has_obs=(rng.random(n_mp) < 0.9).astype(np.uint8))


def _q(rng, kl, kr, desc, n_q, noise=3.0):
    nl = len(kl)
    src = rng.integers(0, max(nl, 1), n_q)
    kls = kl[src] if nl else _kps(rng, n_q)
    dsrc = desc[src] if nl else rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    octave = kls["octave"].astype(np.int32)
    octave[rng.random(n_q) < 0.02] = 8
    return dict(u=kls["x"] + rng.normal(0, noise, n_q).astype(np.float32), v=kls["y"] + rng.normal(0, noise, n_q).astype(np.float32),
                xr=kls["x"] + rng.normal(-4, noise, n_q).astype(np.float32), yr=kls["y"] + rng.normal(0, noise, n_q).astype(np.float32),
                octave=octave, angle=(kls["angle"] + rng.normal(0, 8, n_q)).astype(np.float32) % 360, desc=_noisy(rng, dsrc, 0.05),
                has_obs=(rng.random(n_q) < 0.9).astype(np.uint8))


def _handle(m, kl, kr, desc, l2r, r2l, cap=None):
    import orb_slam3_amd as osa
    return osa.DeviceFrame(m, cap or max(1, len(kl) + len(kr))).load_fisheye(_left_view(kl, desc), kr, l2r, r2l)


@pytest.mark.parametrize("packed", [False, True])
def test_handle_m1_equals_host_and_oracle(oracle, packed):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(31 + packed)
    nl, nr = (300, 280) if packed else (1100, 1000)
    kl, kr, desc, l2r, r2l = _rig_frame(rng, nl, nr, packed)
    mp = _mp(rng, kl, kr, desc, 900 if packed else 2500, noise=1.0 if packed else 2.0)
    occ = (rng.random(nl + nr) < 0.1).astype(np.uint8)
    gl, gr = _grids(oracle, kl, kr)
    for th, ratio in ((1.0, 0.8), (3.0, 0.8), (5.0, 0.6)):
        m = osa.ORBmatcher(ratio, True)
        F = _handle(m, kl, kr, desc, l2r, r2l)
        assert F.counts() == (nl, nr)
        for o in (None, occ):
            on, ofm = oracle.search_by_projection_mappoints_fisheye(gl, gr, desc, SF, l2r, r2l, mp, th, ratio, o)
            hn, hfm = m.SearchByProjectionFisheye(_left_view(kl, desc), kr, l2r, r2l, mp, th, frame_occupied=o)
            dn, dfm = m.SearchByProjectionFisheye(F, None, None, None, mp, th, frame_occupied=o)
            assert (hn, hfm.tolist()) == (on, ofm.tolist()), (th, ratio)
            assert (dn, dfm.tolist()) == (on, ofm.tolist()), (th, ratio)
            assert on > 50
            # stereo partners occupied on both sides
            both = np.nonzero(ofm[:nl] >= 0)[0]
            assert any(l2r[i] >= 0 and ofm[nl + l2r[i]] == ofm[i] for i in both)


@pytest.mark.parametrize("level_mode", [0, 1, 2])
@pytest.mark.parametrize("ori", [True, False])
def test_handle_m2_equals_host_and_oracle(oracle, level_mode, ori):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(41 + level_mode + 3 * ori)
    nl, nr = 1000, 900
    kl, kr, desc, l2r, r2l = _rig_frame(rng, nl, nr)
    q = _q(rng, kl, kr, desc, 1500)
    # the right-camera projection lands on the stereo partner (when there is one) of the left keypoint the query came from
    near = np.array([int(np.argmin((kl["x"] - u) ** 2 + (kl["y"] - v) ** 2)) for u, v in zip(q["u"], q["v"])])
    part = l2r[near]
    has = part >= 0
    q["xr"][has] = kr["x"][part[has]] + rng.normal(0, 2, has.sum()).astype(np.float32)
    q["yr"][has] = kr["y"][part[has]] + rng.normal(0, 2, has.sum()).astype(np.float32)
    occ = (rng.random(nl + nr) < 0.1).astype(np.uint8)
    gl, gr = _grids(oracle, kl, kr)
    m = osa.ORBmatcher(0.9, ori)
    F = _handle(m, kl, kr, desc, l2r, r2l)
    for th in (3.0, 7.0):
        on, ocm = oracle.search_by_projection_frame_fisheye(gl, gr, desc, SF, q, th, level_mode, ori, occ)
        hn, hcm = m.SearchByProjectionFrameFisheye(_left_view(kl, desc), kr, q, th, level_mode, cur_occupied=occ, raw=True)
        dn, dcm = m.SearchByProjectionFrameFisheye(F, None, q, th, level_mode, cur_occupied=occ, raw=True)
        assert (hn, hcm.tolist()) == (dn, dcm.tolist())
        assert (dn, np.maximum(dcm, -1).tolist()) == (on, np.maximum(ocm, -1).tolist())
        assert on > 50 and (dcm[nl:] >= 0).any()


@pytest.mark.parametrize("nl,nr", [(600, 0), (0, 600), (0, 0)])
def test_handle_one_camera_or_empty(oracle, nl, nr):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(51 + nl + 2 * nr)
    kl, kr, desc, l2r, r2l = _rig_frame(rng, nl, nr)
    m = osa.ORBmatcher(0.8, True)
    F = _handle(m, kl, kr, desc, l2r, r2l, cap=700)
    assert F.counts() == (nl, nr) and F.count() == nl + nr
    mp = _mp(rng, kl, kr, desc, 500)
    q = _q(rng, kl, kr, desc, 500)
    hn, hfm = m.SearchByProjectionFisheye(_left_view(kl, desc), kr, l2r, r2l, mp, 3.0)
    dn, dfm = m.SearchByProjectionFisheye(F, None, None, None, mp, 3.0)
    assert (dn, dfm.tolist()) == (hn, hfm.tolist()) and len(dfm) == nl + nr
    if nl + nr:
        gl, gr = _grids(oracle, kl, kr)
        on, ofm = oracle.search_by_projection_mappoints_fisheye(gl, gr, desc, SF, l2r, r2l, mp, 3.0, 0.8)
        assert (dn, dfm.tolist()) == (on, ofm.tolist()) and (on > 0 or nl == 0)
    hn, hcm = m.SearchByProjectionFrameFisheye(_left_view(kl, desc), kr, q, 5.0, 0, raw=True)
    dn, dcm = m.SearchByProjectionFrameFisheye(F, None, q, 5.0, 0, raw=True)
    assert (dn, dcm.tolist()) == (hn, hcm.tolist())


# ---- SearchLocalPoints on a rig: isInFrustumChecks x 2 + M1 ----
def _oracle_local_points(oracle, c, views, gl, gr, desc, l2r, r2l, mp_desc, eligible, has_obs, track_depth, th, ratio, far, th_far, occ, nlevels):
    pv = [oracle.is_in_frustum_checks(views[s], c["bounds"], c["lsf"], nlevels, c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"]) for s in (0, 1)]
    el = np.ones(len(c["pos"]), bool) if eligible is None else eligible.astype(bool)
    ivl, ivr = pv[0]["in_view"].astype(bool) & el, pv[1]["in_view"].astype(bool) & el
    dep = np.where(ivl, pv[0]["depth"], track_depth if track_depth is not None else 0)
    isfar = far & (ivl | (track_depth is not None)) & (dep > th_far)
    ok = (ivl | ivr) & ~isfar
    mp = dict(in_view=(ok & ivl).astype(np.uint8), proj_x=pv[0]["proj_x"], proj_y=pv[0]["proj_y"], level=pv[0]["level"], view_cos=pv[0]["view_cos"],
              in_view_r=(ok & ivr).astype(np.uint8), proj_xr=pv[1]["proj_x"], proj_yr=pv[1]["proj_y"], level_r=pv[1]["level"],
              view_cos_r=pv[1]["view_cos"], desc=mp_desc, has_obs=has_obs if has_obs is not None else np.ones(len(ok), np.uint8))
    n, fm = oracle.search_by_projection_mappoints_fisheye(gl, gr, desc, SF[:nlevels], l2r, r2l, mp, th, ratio, occ)
    return n, fm, np.stack([ivl, ivr]).astype(np.uint8)


def _features_at(rng, oracle, c, views, n_side, nlevels):
    """Keypoints of each camera at the projections of map points that camera sees, descriptors shared by the point."""
    import orb_slam3_amd as osa
    n_mp = len(c["pos"])
    mp_desc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    ks, ds, srcs = [], [], []
    for s in (0, 1):
        pv = oracle.is_in_frustum_checks(views[s], c["bounds"], c["lsf"], nlevels, c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"])
        vis = np.nonzero(pv["in_view"])[0]
        src = rng.choice(vis, min(n_side, len(vis)), replace=False)
        k = np.zeros(len(src), osa.KP_DTYPE)
        k["x"] = np.clip(pv["proj_x"][src] + rng.normal(0, 1.5, len(src)), 0, W - 1).astype(np.float32)
        k["y"] = np.clip(pv["proj_y"][src] + rng.normal(0, 1.5, len(src)), 0, H - 1).astype(np.float32)
        k["octave"] = np.clip(pv["level"][src] + rng.integers(-1, 1, len(src)), 0, nlevels - 1)
        k["angle"] = rng.uniform(0, 360, len(src)).astype(np.float32)
        k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
        ks.append(k)
        ds.append(_noisy(rng, mp_desc[src], 0.06))
        srcs.append(src)
    # stereo partners: features of the two cameras that come from the same map point
    l2r, r2l = np.full(len(ks[0]), -1, np.int32), np.full(len(ks[1]), -1, np.int32)
    pos_r = {int(p): j for j, p in enumerate(srcs[1])}
    for i, p in enumerate(srcs[0]):
        j = pos_r.get(int(p))
        if j is not None:
            l2r[i], r2l[j] = j, i
    return ks[0], ks[1], np.concatenate(ds).reshape(-1, 32), l2r, r2l, mp_desc


@pytest.mark.parametrize("n_mp", [3000, 10000])
def test_search_local_points_fisheye_equals_oracle_composition(oracle, n_mp):
    import orb_slam3_amd as osa
    from test_oracle_geometry import fisheye_case, fisheye_views
    rng = np.random.default_rng(61 + n_mp)
    c = fisheye_case(1, n=n_mp)
    views = fisheye_views(fisheye_case(1), "fisheye/1")
    nlevels = int(c["nl"])
    kl, kr, desc, l2r, r2l, mp_desc = _features_at(rng, oracle, c, views, 1000, nlevels)
    nl, nr = len(kl), len(kr)
    assert nl > 500 and nr > 500 and (l2r >= 0).sum() > 100
    sf = SF[:nlevels]
    gl, gr = _grids(oracle, kl, kr)
    m = osa.ORBmatcher(0.8, True)
    F = osa.DeviceFrame(m, nl + nr).load_fisheye(osa.FrameView(kl, desc, 0.0, float(W), 0.0, float(H), sf), kr, l2r, r2l)
    eligible = (rng.random(n_mp) < 0.9).astype(np.uint8)
    has_obs = (rng.random(n_mp) < 0.9).astype(np.uint8)
    occ = (rng.random(nl + nr) < 0.05).astype(np.uint8)
    pv0 = oracle.is_in_frustum_checks(views[0], c["bounds"], c["lsf"], nlevels, c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"])
    th_far = float(np.median(pv0["depth"][pv0["in_view"].astype(bool)]))
    track_depth = rng.uniform(0.5 * th_far, 1.5 * th_far, n_mp).astype(np.float32)
    cases = [(1.0, False, None, None, None, None), (3.0, False, eligible, has_obs, None, occ), (1.0, True, eligible, None, None, None),
             (1.0, True, None, has_obs, track_depth, occ)]
    right_only_far = 0
    for th, far, el, ho, td, o in cases:
        on, ofm, oiv = _oracle_local_points(oracle, c, views, gl, gr, desc, l2r, r2l, mp_desc, el, ho, td, th, 0.8, far, th_far, o, nlevels)
        dn, dfm, div = m.SearchLocalPointsFisheye(F, views, c["lsf"], c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"], mp_desc, eligible=el,
                                                  has_obs=ho, track_depth=td, th=th, far_points=far, th_far_points=th_far, frame_occupied=o)
        assert np.array_equal(div, oiv)
        assert (dn, dfm.tolist()) == (on, ofm.tolist()), (th, far, td is not None)
        assert on > 100 and (dfm[nl:] >= 0).any()
        if td is not None:
            right_only_far += int(((oiv[1] == 1) & (oiv[0] == 0) & (td > th_far)).sum())
    assert right_only_far > 0   # the corner case is exercised


def test_levels_out_of_range_drop_that_camera(oracle):
    """A predicted level outside the frame's levels cannot come out of the one call (isInFrustumChecks clamps it to the frame's levels); given to
    M1 it drops that camera's sub-query only, as the host-pointer form does.  (The reference would index mvScaleFactors out of bounds: the oracle
    is compared with those sub-queries switched off.)"""
    import orb_slam3_amd as osa
    rng = np.random.default_rng(71)
    kl, kr, desc, l2r, r2l = _rig_frame(rng, 800, 800)
    mp = _mp(rng, kl, kr, desc, 1500)
    mp["level"][::7] = 8
    mp["level_r"][::5] = 9
    gl, gr = _grids(oracle, kl, kr)
    m = osa.ORBmatcher(0.8, True)
    F = _handle(m, kl, kr, desc, l2r, r2l)
    off = dict(mp, in_view=np.where(mp["level"] >= 8, 0, mp["in_view"]).astype(np.uint8),
               in_view_r=np.where(mp["level_r"] >= 8, 0, mp["in_view_r"]).astype(np.uint8))
    off["level"] = np.minimum(mp["level"], 7)
    off["level_r"] = np.minimum(mp["level_r"], 7)
    on, ofm = oracle.search_by_projection_mappoints_fisheye(gl, gr, desc, SF, l2r, r2l, off, 3.0, 0.8)
    hn, hfm = m.SearchByProjectionFisheye(_left_view(kl, desc), kr, l2r, r2l, mp, 3.0)
    dn, dfm = m.SearchByProjectionFisheye(F, None, None, None, mp, 3.0)
    assert (dn, dfm.tolist()) == (hn, hfm.tolist()) == (on, ofm.tolist())


# ---- batch load ----
def _extract_pairs(w, h, nb, nf, first=0):
    import torch
    from orb_slam3_amd import synth
    canvas = synth.make_canvas(11, size=2048)
    pairs = [synth.make_stereo_pair(11, t, w, h, canvas) for t in range(first, first + nb)]
    left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return left, right


def test_load_stereo_fisheye_batch_equals_host_load(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    w = h = 512
    nb, nf = 4, 1000
    left, right = _extract_pairs(w, h, 2 * nb, nf)
    fs = w * h
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    rig = _rig_for_shifted_images()
    m = osa.ORBmatcher(0.8, True)
    capl, capr = None, None

    def extract(first):
        exl.extract_batch_device(left.data_ptr() + first * fs, nb, w, h, w, fs, (0, 0))
        exr.extract_batch_device(right.data_ptr() + first * fs, nb, w, h, w, fs, (0, 0))

    extract(0)
    exl.stereo_fisheye_batch_device(exr, rig)
    capl, capr = exl.batch_view().cap, exr.batch_view().cap
    sf = exl.GetScaleFactors().astype(np.float32)
    bounds = (0.0, float(w), 0.0, float(h))
    rng = np.random.default_rng(81)
    for f in (0, nb - 1):
        D = osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, f, bounds=bounds, scale_factors=sf)
        if f == nb - 1:
            extract(nb)          # the next batch right behind the load, no synchronisation in between
        # reference: the downloaded rows of frame f of the FIRST batch
        exl2, exr2 = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
        exl2.extract_batch_device(left.data_ptr(), nb, w, h, w, fs, (0, 0))
        exr2.extract_batch_device(right.data_ptr(), nb, w, h, w, fs, (0, 0))
        exl2.stereo_fisheye_batch_device(exr2, rig)
        _, _, l2r, r2l, _, _ = exl2.stereo_fisheye_download(f)
        _, kl, dl = exl2.download(f)
        _, kr, dr = exr2.download(f)
        desc = np.concatenate([dl, dr]).reshape(-1, 32)
        Hh = osa.DeviceFrame(m, capl + capr).load_fisheye(osa.FrameView(kl, desc, 0.0, float(w), 0.0, float(h), sf), kr, l2r, r2l)
        mp = _mp(rng, kl, kr, desc, 1500)
        if f == 0:
            fm_rows = m._frame_rows(D, None)
            assert fm_rows == capl + capr    # counts unknown until the first search
        dn, dfm = m.SearchByProjectionFisheye(D, None, None, None, mp, 3.0)
        assert D.counts() == (len(kl), len(kr))
        hn, hfm = m.SearchByProjectionFisheye(Hh, None, None, None, mp, 3.0)
        assert (dn, dfm.tolist()) == (hn, hfm.tolist()) and hn > 20
        q = _q(rng, kl, kr, desc, 800)
        assert m.SearchByProjectionFrameFisheye(D, None, q, 5.0, 0, raw=True)[1].tolist() == \
            m.SearchByProjectionFrameFisheye(Hh, None, q, 5.0, 0, raw=True)[1].tolist()
    # the stage is of the older batch now: refused
    with pytest.raises(_lib.OrbxError):
        osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, 0)
    exl.stereo_fisheye_batch_device(exr, rig)
    osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, 0)
    with pytest.raises(_lib.OrbxError):   # cap_left + cap_right > cap
        osa.DeviceFrame(m, capl + capr - 1).load_stereo_fisheye_batch(exl, exr, 0)
    with pytest.raises(_lib.OrbxError):   # another right extractor than the stage's
        osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exl, 0)


def _whole(a):
    """The array a wrapper handed to the library, of which the returned `a` is the leading N entries of every row."""
    return a if a.base is None else a.base


# entry points that can be the first to touch a batch-loaded fisheye handle, and the value their wrappers fill the result arrays with
PENDING = {"mappoints": -1, "frame": -1, "window_left_only": -1, "local_points": -1, "compute_bow": 0, "search_by_bow": -1}


@pytest.mark.parametrize("entry", sorted(PENDING))
def test_counts_pending_equal_counted_first(entry):
    """Two handles loaded from the same frame of a fisheye stereo stage with a capacity above N: A is counted first, B meets the call with its
    counts still on the device.  The same return value, the same entries [0, N), nothing written beyond N (the wrappers' arrays have the handle's
    capacity and keep their fill there), and B knows A's counts afterwards."""
    import orb_slam3_amd as osa
    from test_gpu_matcher import _random_vocabulary
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    w = h = 512
    nb, nf, f = 8, 1000, 3
    left, right = _extract_pairs(w, h, nb, nf)
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    exl.extract_batch_device(left.data_ptr(), nb, w, h, w, w * h, (0, 0))
    exr.extract_batch_device(right.data_ptr(), nb, w, h, w, w * h, (0, 0))
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    sf = exl.GetScaleFactors().astype(np.float32)
    bounds = (0.0, float(w), 0.0, float(h))
    (_, kl, dl), (_, kr, dr), (_, kl2, dl2) = exl.download(f), exr.download(f), exl.download(f - 1)
    desc = np.concatenate([dl, dr]).reshape(-1, 32)
    nl, nr = len(kl), len(kr)
    N, cap = nl + nr, exl.batch_view().cap + exr.batch_view().cap + 37
    assert nl > 0 and nr > 0 and N < cap
    rng = np.random.default_rng(83)
    m = osa.ORBmatcher(0.8, True)
    if entry == "mappoints":
        mp = _mp(rng, kl, kr, desc, 1500)

        def call(D):
            n, fm = m.SearchByProjectionFisheye(D, None, None, None, mp, 3.0)
            return [n], [fm]
    elif entry == "frame":
        q = _q(rng, kl, kr, desc, 800)

        def call(D):
            n, cm = m.SearchByProjectionFrameFisheye(D, None, q, 5.0, 0, raw=True)
            return [n], [cm]
    elif entry == "window_left_only":
        q = _q(rng, kl, kr, desc, 800)
        o = np.minimum(q["octave"], 7)
        qw = dict(x=q["u"], y=q["v"], r=(7.0 * sf[o]).astype(np.float32), min_level=o - 1, max_level=o + 1, angle=q["angle"], desc=q["desc"],
                  has_obs=q["has_obs"])

        def call(D):
            n, match = m.SearchByProjectionWindowFisheye(D, qw, 64.0, True, raw=True)
            assert (match[nl:] == -1).all()   # the right camera is not searched
            return [n], [match]
    elif entry == "local_points":
        from test_oracle_geometry import fisheye_case, fisheye_views
        c = fisheye_case(1, n=3000)
        views = fisheye_views(fisheye_case(1), "fisheye/1")
        mp_desc = _noisy(rng, desc[rng.integers(0, N, 3000)], 0.05)

        def call(D):
            n, fm, iv = m.SearchLocalPointsFisheye(D, views, c["lsf"], c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"], mp_desc, th=30.0)   # (wide windows: the points are not the features')
            return [n, iv], [fm]
    else:
        cp, ci, nd, wi = _random_vocabulary(rng, 4, 2, ragged=False)
        voc = osa.ORBVocabulary(2, cp, ci, _noisy(rng, desc[rng.integers(0, N, len(nd))], 0.03), wi)
        if entry == "compute_bow":
            def call(D):
                return [], list(D.compute_bow_fisheye(voc, 1))
        else:
            _, node = m.BowTransform(voc, dl2, 1)
            nodes = np.unique(node)
            kfs = [(dl2, kl2["angle"], None, osa.FeatureVector(nodes, [np.nonzero(node == x)[0] for x in nodes]))]

            def call(D):
                D.compute_bow_fisheye(voc, 1, download=False)
                nm, match = m.SearchByBoWDeviceFisheye(D, kfs)
                return [nm], [match]

    def load():
        return osa.DeviceFrame(m, cap).load_stereo_fisheye_batch(exl, exr, f, bounds=bounds, scale_factors=sf)
    A, B = load(), load()
    assert A.counts() == (nl, nr)
    (ra, a), (rb, b) = call(A), call(B)
    assert len(ra) == len(rb) and all(np.array_equal(x, y) for x, y in zip(ra, rb)), (ra, rb)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.shape[-1] == N and np.array_equal(x, y)
        for whole in (_whole(x), _whole(y)):
            assert whole.shape[-1] == cap and (whole[..., N:] == PENDING[entry]).all()
    if entry not in ("compute_bow", "local_points"):
        assert (a[0] >= 0).sum() > 20   # the call did match
    assert B.counts() == (nl, nr) and B.count() == N


# ---- refusals ----
def test_refusals(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(91)
    kl, kr, desc, l2r, r2l = _rig_frame(rng, 200, 150)
    m, m2 = osa.ORBmatcher(0.8, True), osa.ORBmatcher(0.8, True)
    Fi = _handle(m, kl, kr, desc, l2r, r2l)
    Mo = osa.DeviceFrame(m, 400).load(osa.FrameView(kl, desc[:200], 0.0, float(W), 0.0, float(H), SF))
    assert Mo.counts() == (200, -1)
    mp = _mp(rng, kl, kr, desc, 100)
    qm = dict(proj_x=mp["proj_x"], proj_y=mp["proj_y"], level=mp["level"], view_cos=mp["view_cos"], desc=mp["desc"])
    q = _q(rng, kl, kr, desc, 100)
    qw = dict(x=q["u"], y=q["v"], r=np.full(100, 5, np.float32), min_level=np.zeros(100, np.int32), max_level=np.full(100, 7, np.int32),
              angle=q["angle"], desc=q["desc"])
    bad = _lib.ORBX_E_BAD_ARG if hasattr(_lib, "ORBX_E_BAD_ARG") else None
    for call in (lambda: m.SearchByProjection(Fi, qm), lambda: m.SearchByProjectionFrame(Fi, dict(q, ur=None), 3.0),
                 lambda: m.SearchByProjectionWindow(Fi, qw, 100, True),
                 lambda: m.SearchLocalPoints(Fi, (400, 400, 256, 256, 0, 0, 0, 0, 0, 40), (np.eye(3), np.zeros(3), np.zeros(3)), np.log(1.2), 0.5,
                                             np.ones((5, 3)), np.ones((5, 3)), np.ones(5), np.ones(5) * 9, np.zeros((5, 32), np.uint8)),
                 lambda: m.SearchByProjectionFisheye(Mo, None, None, None, mp, 3.0), lambda: m.SearchByProjectionFrameFisheye(Mo, None, q, 3.0),
                 lambda: m2.SearchByProjectionFisheye(Fi, None, None, None, mp, 3.0), lambda: m2.SearchByProjectionFrameFisheye(Fi, None, q, 3.0)):
        with pytest.raises(_lib.OrbxError):
            call()
    n = np.zeros(1, np.int32)
    assert L.orbx_frame_compute_bow(m._h, Fi._h, None, 4, None, None) < 0
    assert L.orbx_frame_search_by_bow(m._h, Fi._h, 0, None, C.c_float(0.8), 1, None, 400, _lib.ptr(n)) < 0
    views = np.zeros(46, np.float32)
    P = np.ones((5, 3), np.float32)
    iv, fm = np.zeros(10, np.uint8), np.zeros(400, np.int32)
    one = np.ones(5, np.float32)
    d5 = np.zeros((5, 32), np.uint8)
    assert L.orbx_frame_search_local_points_fisheye(m._h, Mo._h, None, _lib.ptr(views), 0.18, 0.5, 5, _lib.ptr(P), _lib.ptr(P), _lib.ptr(one), _lib.ptr(one),
                                                    _lib.ptr(d5), None, None, None, 1.0, 0.8, 0, 0.0, _lib.ptr(iv), _lib.ptr(fm)) < 0
    assert L.orbx_frame_search_local_points_fisheye(m2._h, Fi._h, None, _lib.ptr(views), 0.18, 0.5, 5, _lib.ptr(P), _lib.ptr(P), _lib.ptr(one), _lib.ptr(one),
                                                    _lib.ptr(d5), None, None, None, 1.0, 0.8, 0, 0.0, _lib.ptr(iv), _lib.ptr(fm)) < 0
    # out-of-range partners are refused before anything is enqueued; the handle keeps its frame
    bl2r, br2l = l2r.copy(), r2l.copy()
    bl2r[0], br2l[0] = 150, -2
    for bl2r, br2l in ((bl2r, r2l), (l2r, br2l)):
        with pytest.raises(_lib.OrbxError):
            Fi.load_fisheye(_left_view(kl, desc), kr, bl2r, br2l)
    assert Fi.counts() == (200, 150)


def test_cpp_demo_equals_python(oracle, tmp_path):
    """tests/cpp/frame_fisheye_demo.cpp, compiled with g++ against liborbx.so: the C++ DeviceFrame / ORBmatcher overloads give the Python path's results."""
    import orb_slam3_amd as osa
    rng = np.random.default_rng(101)
    kl, kr, desc, l2r, r2l = _rig_frame(rng, 700, 650)
    mp = _mp(rng, kl, kr, desc, 1200)
    m = osa.ORBmatcher(0.75, True)
    F = _handle(m, kl, kr, desc, l2r, r2l)
    n, fm = m.SearchByProjectionFisheye(F, None, None, None, mp, 3.0)
    for name, a in (("kl", kl), ("kr", kr), ("desc", desc), ("l2r", l2r), ("r2l", r2l), ("sf", SF)):
        np.ascontiguousarray(a).tofile(tmp_path / f"{name}.bin")
    for k in ("in_view", "proj_x", "proj_y", "level", "view_cos", "in_view_r", "proj_xr", "proj_yr", "level_r", "view_cos_r", "desc", "has_obs"):
        np.ascontiguousarray(mp[k]).tofile(tmp_path / f"mp_{k}.bin")
    from orb_slam3_amd import _lib
    lib = Path(_lib.LIB_PATH)   # (the emulated library under ORBX_TEST_EMULATOR: same C ABI)
    exe = tmp_path / "demo"
    r = subprocess.run(["g++", "-std=c++17", "-O1", str(ROOT / "tests" / "cpp" / "frame_fisheye_demo.cpp"), "-o", str(exe), str(lib),
                        "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = str(Path(torch.__file__).parent / "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe), str(tmp_path), str(len(kl)), str(len(kr)), str(len(mp["proj_x"]))], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(tmp_path / "match.bin", np.int32)
    assert int(r.stdout.split()[0]) == n and got.tolist() == fm.tolist()
