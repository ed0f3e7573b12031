"""The device-resident map-point table (orbx_map / DeviceMap) and the `_map` forms of the eight one-call searches, which name their map points by
id: 4 bytes per point go up instead of 64.  Every `_map` result is compared for equality with the flat call on host-gathered rows and with the
reference the existing tests of that call compose from the oracle.  The scenes and references are the existing helpers' (tests/sim3_scene.py,
tests/sim3_fisheye_scene.py, tests/distinctive_sets.py, the builders of test_gpu_frame_handle / test_gpu_frame_fisheye / test_gpu_keyframe*);
nothing here composes a reference from the code under test.  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import ctypes as C
import threading

import numpy as np
import pytest

import distinctive_sets as DS
import sim3_fisheye_scene as SF
import sim3_scene as S
import test_gpu_frame_fisheye as FF
import test_gpu_frame_handle as FH
import test_gpu_keyframe as T
import test_gpu_keyframe_fisheye as TF
import test_gpu_keyframe_sim3 as TS
import test_gpu_keyframe_sim3_fisheye as TSF
from test_gpu_keyframe_distinctive import batch  # noqa: F401  (two 320 x 240 stereo pairs through both extractors and the fisheye stage)

pytestmark = pytest.mark.gpu

f32 = np.float32
BAD, TOO_LARGE = -2, -7
FIELDS = ("pos", "normal", "min_dist", "max_dist", "desc")
LAYOUT_ALIGN = 256   # orbx::Layout::pad (matcher_context.h): every arena buffer starts on a multiple of it and owns its size rounded up to it


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _random_points(rng, n):
    return dict(pos=rng.normal(0, 5, (n, 3)).astype(f32), normal=rng.normal(0, 1, (n, 3)).astype(f32), min_dist=rng.uniform(0.1, 1, n).astype(f32),
                max_dist=rng.uniform(5, 50, n).astype(f32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))


def _rows(mp, sel):
    return {k: np.ascontiguousarray(mp[k][sel]) for k in FIELDS}


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in FIELDS[:4]) and np.array_equal(a["desc"], b["desc"])


def _resident(osa, m, rng, mp, capacity=4096, held=2000):
    """A table of `held` live slots at random ids of [0, capacity), the points of `mp` among them in a shuffled order; returns (map, ids of mp's
    rows).  The other slots hold random points."""
    n = len(mp["pos"])
    assert n < held < capacity
    slots = rng.permutation(capacity)[:held].astype(np.int32)
    M = osa.DeviceMap(capacity)
    M.update(m, slots[:n], **_rows(mp, slice(None)))
    M.update(m, slots[n:], **_random_points(rng, held - n))
    return M, np.ascontiguousarray(slots[:n])


# ---- 1. the store ----
def test_store_round_trip_and_partial_updates():
    """1000 points under a random permutation of non-contiguous ids that include 0 and 4095: read returns every field bit for bit; then desc only
    on 300, pos + normal on an overlapping 300 and all fields on 1, each followed by a read of all 1000 that shows exactly the named fields changed.
    The updates are issued in pieces of 1, 63, 64, 65, 255, 256 and 257 ids: the scatter and gather kernels deal 64 points to a block."""
    import orb_slam3_amd as osa
    rng = np.random.default_rng(3)
    m = osa.ORBmatcher(0.6, True)
    M = osa.DeviceMap(4096)
    ids = np.concatenate([[0, 4095], 1 + rng.permutation(4094)[:998]]).astype(np.int32)
    ids = np.ascontiguousarray(ids[rng.permutation(1000)])
    assert len(np.unique(ids)) == 1000 and (np.diff(np.sort(ids)) > 1).any()
    want = _random_points(rng, 1000)
    pieces = [1, 63, 64, 65, 255, 256, 257]
    assert sum(pieces) < 1000
    at = 0
    for n in pieces + [1000 - sum(pieces)]:
        M.update(m, ids[at:at + n], **_rows(want, slice(at, at + n)))
        at += n
    assert _same(M.read(m, ids), want)
    for n in pieces:   # the gather's block edges
        assert _same(M.read(m, ids[:n]), _rows(want, slice(0, n)))

    def partial(sel, fields, sizes):
        new = _random_points(rng, len(sel))
        at = 0
        for n in sizes:
            M.update(m, ids[sel[at:at + n]], **{k: new[k][at:at + n] for k in fields})
            at += n
        assert at == len(sel)
        for k in fields:
            want[k][sel] = new[k]
        assert _same(M.read(m, ids), want), fields

    partial(np.arange(100, 400), ("desc",), [255, 45])
    partial(np.arange(250, 550), ("pos", "normal"), [257, 43])
    partial(np.array([999]), FIELDS, [1])
    partial(np.arange(0, 256), ("min_dist",), [256])
    partial(np.arange(600, 665), ("max_dist", "desc"), [65])
    assert _same(M.read(m, ids[::-1].copy()), _rows(want, slice(None, None, -1)))
    twice = np.ascontiguousarray(np.concatenate([ids[:5], ids[:5]]))   # a read may name a slot twice
    assert _same(M.read(m, twice), _rows(want, np.concatenate([np.arange(5), np.arange(5)])))


# ---- 2. SearchLocalPoints, both kinds ----
N_LOCAL = 600
LOCAL_SIZES = [1, 255, 256, 257, 600]
BOUNDS_M = (0.0, 320.0, 0.0, 240.0)


@pytest.fixture(scope="module")
def mono_local(oracle, batch):  # noqa: F811
    """The left 320 x 240 frame 1 of the batch (a few hundred features), 600 map points back-projected from its features, the oracle's frustum
    records of all of them (computed once), and a table of 2000 points that holds them under shuffled ids."""
    import orb_slam3_amd as osa
    exl = batch["keep"][0]
    _, k, d = exl.download(1)
    sf = exl.GetScaleFactors().astype(f32)
    rng = np.random.default_rng(41)
    src, pos, normal, min_d, max_d = FH._local_map(rng, k, N_LOCAL, False)
    mp = dict(pos=pos, normal=normal, min_dist=min_d, max_dist=max_d, desc=FH._noisy(rng, d[src], 0.05))
    a = 0.01
    Rcw = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], f32)
    tcw = np.array([0.02, -0.01, 0.03], f32)
    Ow = (-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32)
    lsf = f32(np.log(f32(1.2)))
    frustum = oracle.is_in_frustum(Rcw, tcw, Ow, FH.EUROC4 + (0.0,), np.array(BOUNDS_M, f32), lsf, len(sf), 0.5, pos, normal, min_d, max_d)
    assert 100 < frustum["in_view"].sum() < N_LOCAL
    m = osa.ORBmatcher(0.8, True)
    M, ids = _resident(osa, m, rng, mp)
    return dict(k=k, d=d, sf=sf, mp=mp, pose=(Rcw, tcw, Ow), lsf=lsf, frustum=frustum, m=m, M=M, ids=ids, exl=exl,
                eligible=(rng.random(N_LOCAL) < 0.9).astype(np.uint8), has_obs=(rng.random(N_LOCAL) < 0.95).astype(np.uint8),
                occ=(rng.random(len(k)) < 0.05).astype(np.uint8), grid=oracle.OracleGrid(k, *BOUNDS_M))


def _mono_frame(osa, c, pending):
    cap = len(c["k"]) + 37
    if pending:   # the count stays on the device until the call brings it home
        return osa.DeviceFrame(c["m"], c["exl"].batch_view().cap + 37).load_batch(c["exl"], 1, bounds=BOUNDS_M, scale_factors=c["sf"])
    return osa.DeviceFrame(c["m"], cap).load(osa.FrameView(c["k"], c["d"], *BOUNDS_M, c["sf"]))


def _mono_oracle(oracle, c, sel, th, far_points, th_far):
    w = {key: val[sel] for key, val in c["frustum"].items()}
    el, ho = c["eligible"][sel], c["has_obs"][sel]
    iv = w["in_view"] & el
    searched = iv.astype(bool) & ~(far_points & (w["depth"] > f32(th_far)))
    rec = dict(proj_x=w["proj_x"], proj_y=w["proj_y"], proj_xr=w["proj_xr"], level=w["level"], view_cos=w["view_cos"], desc=c["mp"]["desc"][sel],
               in_view=searched.astype(np.uint8), has_obs=ho)
    n, fm = oracle.search_by_projection_mappoints(c["grid"], c["d"], c["sf"], rec, th, 0.8, None, c["occ"])
    return n, fm, iv


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("n_mp", LOCAL_SIZES)
def test_search_local_points_map_equals_flat_and_oracle(oracle, mono_local, n_mp, pending):
    import orb_slam3_amd as osa
    c = mono_local
    m, M, mp = c["m"], c["M"], c["mp"]
    sel = np.arange(n_mp)
    cam10 = FH.EUROC4 + (0, 0, 0, 0, 0, 0.0)
    th, far_points, th_far = 3.0, True, 12.0
    F = _mono_frame(osa, c, pending)
    got = m.SearchLocalPointsMap(F, cam10, c["pose"], c["lsf"], 0.5, M, c["ids"][sel], c["eligible"][sel], c["has_obs"][sel], th, far_points, th_far,
                                 c["occ"])
    assert F.count() == len(c["k"])
    flat = m.SearchLocalPoints(_mono_frame(osa, c, pending), cam10, c["pose"], c["lsf"], 0.5, mp["pos"][sel], mp["normal"][sel], mp["min_dist"][sel],
                               mp["max_dist"][sel], mp["desc"][sel], c["eligible"][sel], c["has_obs"][sel], th, far_points, th_far, c["occ"])
    on, ofm, oiv = _mono_oracle(oracle, c, sel, th, far_points, th_far)
    for n, fm, iv in (got, flat):
        assert n == on and np.array_equal(fm, ofm) and np.array_equal(iv, oiv), (n, on)
    if n_mp == N_LOCAL:
        assert on > 50


def test_search_local_points_map_with_an_id_repeated(oracle, mono_local):
    """The same id twice is two queries with equal data: the flat form given that row twice."""
    import orb_slam3_amd as osa
    c = mono_local
    m, M, mp = c["m"], c["M"], c["mp"]
    matched = np.flatnonzero(_mono_oracle(oracle, c, np.arange(N_LOCAL), 3.0, False, 0.0)[1] >= 0)
    j = int(_mono_oracle(oracle, c, np.arange(N_LOCAL), 3.0, False, 0.0)[1][matched[0]])   # a map point that wins a feature
    sel = np.concatenate([np.arange(300), [j], np.arange(300, 400), [j]])
    cam10 = FH.EUROC4 + (0, 0, 0, 0, 0, 0.0)
    got = m.SearchLocalPointsMap(_mono_frame(osa, c, False), cam10, c["pose"], c["lsf"], 0.5, M, c["ids"][sel], c["eligible"][sel], c["has_obs"][sel],
                                 3.0, False, 0.0, c["occ"])
    flat = m.SearchLocalPoints(_mono_frame(osa, c, False), cam10, c["pose"], c["lsf"], 0.5, mp["pos"][sel], mp["normal"][sel], mp["min_dist"][sel],
                               mp["max_dist"][sel], mp["desc"][sel], c["eligible"][sel], c["has_obs"][sel], 3.0, False, 0.0, c["occ"])
    on, ofm, oiv = _mono_oracle(oracle, c, sel, 3.0, False, 0.0)
    for n, fm, iv in (got, flat):
        assert n == on and np.array_equal(fm, ofm) and np.array_equal(iv, oiv)
    assert got[1].max() < len(sel)   # positions in ids, never ids


@pytest.fixture(scope="module")
def rig_local(oracle, batch):  # noqa: F811
    """The fisheye case of test_gpu_frame_fisheye at 600 map points: a host frame whose features sit at the projections of the points (counts
    known), the rig frame 0 of the batch (counts pending), the table."""
    import orb_slam3_amd as osa
    from test_oracle_geometry import fisheye_case, fisheye_views
    rng = np.random.default_rng(67)
    c = fisheye_case(1, n=N_LOCAL)
    views = fisheye_views(fisheye_case(1), "fisheye/1")
    nlevels = int(c["nl"])
    kl, kr, desc, l2r, r2l, mp_desc = FF._features_at(rng, oracle, c, views, 300, nlevels)
    assert len(kl) > 100 and len(kr) > 100
    mp = dict(pos=c["pos"], normal=c["normal"], min_dist=c["mn"], max_dist=c["mx"], desc=mp_desc)
    m = osa.ORBmatcher(0.8, True)
    M, ids = _resident(osa, m, rng, mp)
    pv0 = oracle.is_in_frustum_checks(views[0], c["bounds"], c["lsf"], nlevels, c["cosl"], c["pos"], c["normal"], c["mn"], c["mx"])
    th_far = float(np.median(pv0["depth"][pv0["in_view"].astype(bool)]))
    exl, exr = batch["keep"][:2]
    (_, bkl, bdl), (_, bkr, bdr) = exl.download(0), exr.download(0)
    _, _, bl2r, br2l, _, _ = exl.stereo_fisheye_download(0)
    return dict(c=c, views=views, nlevels=nlevels, host=(kl, kr, desc, l2r, r2l), mp=mp, m=m, M=M, ids=ids, th_far=th_far,
                batch=(bkl, bkr, np.concatenate([bdl, bdr]).reshape(-1, 32), bl2r, br2l), ex=(exl, exr),
                eligible=(rng.random(N_LOCAL) < 0.9).astype(np.uint8), has_obs=(rng.random(N_LOCAL) < 0.9).astype(np.uint8),
                track_depth=rng.uniform(0.5 * th_far, 1.5 * th_far, N_LOCAL).astype(f32))


def _rig_frame(osa, r, pending):
    bounds = (0.0, float(FF.W), 0.0, float(FF.H))
    sf = FF.SF[:r["nlevels"]]
    if pending:
        exl, exr = r["ex"]
        return osa.DeviceFrame(r["m"], exl.batch_view().cap + exr.batch_view().cap).load_stereo_fisheye_batch(exl, exr, 0, bounds=bounds,
                                                                                                            scale_factors=exl.GetScaleFactors().astype(f32))
    kl, kr, desc, l2r, r2l = r["host"]
    return osa.DeviceFrame(r["m"], len(kl) + len(kr)).load_fisheye(osa.FrameView(kl, desc, *bounds, sf), kr, l2r, r2l)


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("n_mp", LOCAL_SIZES)
def test_search_local_points_fisheye_map_equals_flat_and_oracle(oracle, rig_local, n_mp, pending):
    """Both views, track_depth, eligible, has_obs and the occupancy mask; the frame's counts known (a host-loaded frame at the points' projections)
    and pending (the batch's rig frame, loaded with the case's bounds: wide windows, since its features are not the points')."""
    import orb_slam3_amd as osa
    r = rig_local
    m, M, mp, c, views = r["m"], r["M"], r["mp"], r["c"], r["views"]
    sel = np.arange(n_mp)
    kl, kr, desc, l2r, r2l = r["batch"] if pending else r["host"]
    th = 30.0 if pending else 3.0
    occ = (np.arange(len(kl) + len(kr)) % 19 == 0).astype(np.uint8)
    el, ho, td = r["eligible"][sel], r["has_obs"][sel], r["track_depth"][sel]
    F = _rig_frame(osa, r, pending)
    got = m.SearchLocalPointsFisheyeMap(F, views, c["lsf"], c["cosl"], M, r["ids"][sel], el, ho, td, th, True, r["th_far"], occ)
    assert F.counts() == (len(kl), len(kr))
    flat = m.SearchLocalPointsFisheye(_rig_frame(osa, r, pending), views, c["lsf"], c["cosl"], mp["pos"][sel], mp["normal"][sel], mp["min_dist"][sel],
                                      mp["max_dist"][sel], mp["desc"][sel], el, ho, td, th, True, r["th_far"], occ)
    cs = dict(c, pos=c["pos"][sel], normal=c["normal"][sel], mn=c["mn"][sel], mx=c["mx"][sel])
    gl, gr = FF._grids(oracle, kl, kr)
    on, ofm, oiv = FF._oracle_local_points(oracle, cs, views, gl, gr, desc, l2r, r2l, mp["desc"][sel], el, ho, td, th, 0.8, True, r["th_far"], occ,
                                           8 if pending else r["nlevels"])
    for n, fm, iv in (got, flat):
        assert np.array_equal(iv, oiv)
        assert (n, fm.tolist()) == (on, ofm.tolist()), (n, on)
    if n_mp == N_LOCAL and not pending:
        assert on > 50 and (ofm[len(kl):] >= 0).any()


# ---- 3. Fuse and the Sim3 pair, mono and rig ----
@pytest.fixture(scope="module")
def mono_scene(oracle):
    """sim3_scene's scene of seed 5 (K = 3, 300 map points, a make_fuse_scene scene: Fuse's inputs as well), its table and its key frames."""
    import orb_slam3_amd as osa
    sc = S.make_scene(5, 3)
    m = osa.ORBmatcher(0.6, True)
    M, ids = _resident(osa, m, np.random.default_rng(55), sc["map_points"])
    kfs = [osa.DeviceKeyFrame.from_host(m, T._view(osa, sc, k), sc["inv_level_sigma2"]) for k in range(3)]
    return dict(sc=sc, m=m, M=M, ids=ids, kfs=kfs)


@pytest.fixture(scope="module")
def rig_scene(oracle):
    import orb_slam3_amd as osa
    sc = SF.make_scene(oracle, 5, 3)
    m = osa.ORBmatcher(0.6, True)
    M, ids = _resident(osa, m, np.random.default_rng(56), sc["map_points"])
    kfs = [TF._host_kf(osa, m, sc, k) for k in range(3)]
    return dict(sc=sc, m=m, M=M, ids=ids, kfs=kfs)


def _equal_outputs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, (list, tuple)):
            _equal_outputs(x, y)
        elif x is None:
            assert y is None
        elif np.asarray(x).dtype == f32:
            assert np.array_equal(_bits(x), _bits(y))
        else:
            assert np.array_equal(x, y)


@pytest.mark.parametrize("K", [1, 3])
def test_fuse_and_sim3_map_forms_mono(oracle, mono_scene, K):
    c = mono_scene
    sc, m, M, ids, kfs = c["sc"], c["m"], c["M"], c["ids"], c["kfs"][:K]
    cams, poses, mp, lsf = sc["cams"][:K], sc["poses"][:K], sc["map_points"], sc["log_scale_factor"]
    skip, occ = TS._flags(sc, K)
    # Fuse(pKFi, vpMapPointMatches)
    got, flat = m.FuseMapPointsMap(kfs, cams, poses, M, ids, T.TH, lsf, skip), m.FuseMapPoints(kfs, cams, poses, mp, T.TH, lsf, skip)
    _equal_outputs(got, flat)
    bi, bd, pr = T._reference(oracle, sc, range(K), skip)[:3]
    assert np.array_equal(got[0], bi) and np.array_equal(got[1], bd) and np.array_equal(got[2], pr) and pr.sum() > 0.25 * pr.size
    # Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
    got, flat = m.FuseMapPointsSim3Map(kfs, cams, poses, M, ids, T.TH, lsf, skip), m.FuseMapPointsSim3(kfs, cams, poses, mp, T.TH, lsf, skip)
    _equal_outputs(got, flat)
    bi, bd, pr = S.fuse_reference(oracle, sc, range(K), T.TH, skip)[:3]
    assert np.array_equal(got[0], bi) and np.array_equal(got[1], bd) and np.array_equal(got[2], pr)
    # SearchByProjection(pKF, Scw, ...), both projection forms
    for form in (0, 1):
        got = m.SearchByProjectionSim3KeyFramesMap(kfs, cams, poses, M, ids, 8.0, 1.5, lsf, form, skip, occ, want_uv=True)
        flat = m.SearchByProjectionSim3KeyFrames(kfs, cams, poses, mp, 8.0, 1.5, lsf, form, skip, occ, want_uv=True)
        _equal_outputs(got, flat)
        ref = S.search_reference(oracle, sc, range(K), 8.0, 1.5, form, skip, occ)
        TS._assert_search_equal(got, ref)
        assert ref["nm"].sum() > 40


@pytest.mark.parametrize("K", [1, 3])
def test_fuse_and_sim3_map_forms_rig(oracle, rig_scene, K):
    c = rig_scene
    sc, m, M, ids, kfs = c["sc"], c["m"], c["M"], c["ids"], c["kfs"][:K]
    mp, lsf = sc["map_points"], sc["log_scale_factor"]
    skip, occ = TSF._flags(sc, K)
    got, flat = m.FuseMapPointsFisheyeMap(kfs, sc["views"][:K], M, ids, TF.TH, lsf, skip), m.FuseMapPointsFisheye(kfs, sc["views"][:K], mp, TF.TH, lsf, skip)
    _equal_outputs(got, flat)
    bi, bd, pr = TF._reference(oracle, sc, range(K), skip)[:3]
    assert np.array_equal(got[0], bi) and np.array_equal(got[1], bd) and np.array_equal(got[2], pr) and pr.sum() > 0.25 * pr.size
    lv = SF.left_views(sc, range(K))
    got, flat = m.FuseMapPointsSim3FisheyeMap(kfs, lv, M, ids, TF.TH, lsf, skip), m.FuseMapPointsSim3Fisheye(kfs, lv, mp, TF.TH, lsf, skip)
    _equal_outputs(got, flat)
    bi, bd, pr = SF.fuse_reference(oracle, sc, range(K), TF.TH, skip)[:3]
    assert np.array_equal(got[0], bi) and np.array_equal(got[1], bd) and np.array_equal(got[2], pr)
    for form in (0, 1):
        lv = SF.left_views(sc, range(K), form)
        got = m.SearchByProjectionSim3KeyFramesFisheyeMap(kfs, lv, M, ids, 8.0, 1.5, lsf, form, skip, occ, want_uv=True)
        flat = m.SearchByProjectionSim3KeyFramesFisheye(kfs, lv, mp, 8.0, 1.5, lsf, form, skip, occ, want_uv=True)
        _equal_outputs(got, flat)
        ref = SF.search_reference(oracle, sc, range(K), 8.0, 1.5, form, skip, occ)
        TSF._assert_search_equal(got, ref, sc, list(range(K)))
        assert ref["nm"].sum() > 20


# ---- 4. ordering: an update through one context, the search through another, no host synchronisation in between ----
def test_update_then_search_through_another_context(oracle, mono_scene):
    """A updates 500 slots and returns; B at once runs a `_map` search that names 300 of them on its own stream and must see the new values; then A
    updates again and B searches again.  From one thread, then from two threads with a lock around each call."""
    import orb_slam3_amd as osa
    c = mono_scene
    sc, kfs = c["sc"], c["kfs"]
    cams, poses, lsf = sc["cams"], sc["poses"], sc["log_scale_factor"]
    rng = np.random.default_rng(77)
    n = len(sc["map_points"]["pos"])
    A, B = osa.ORBmatcher(0.6, True), osa.ORBmatcher(0.6, True)
    M = osa.DeviceMap(1024)
    slots = rng.permutation(1024)[:500].astype(np.int32)
    ids = np.ascontiguousarray(slots[:n])
    first = sc["map_points"]
    perm = rng.permutation(n)
    second = _rows(first, perm)   # every slot changes all its fields
    wants = [B.FuseMapPointsSim3(kfs, cams, poses, pts, T.TH, lsf) for pts in (first, second)]
    assert not np.array_equal(wants[0][0], wants[1][0]) and (wants[0][1] <= T.TH_LOW).sum() > 100
    garbage = _random_points(rng, 500)

    def update(pts):
        full = {k: np.concatenate([pts[k], garbage[k][n:]]) for k in FIELDS}
        M.update(A, slots, **full)

    M.update(A, slots, **garbage)
    for rnd, pts in enumerate((first, second, first)):
        update(pts)
        _equal_outputs(B.FuseMapPointsSim3Map(kfs, cams, poses, M, ids, T.TH, lsf), wants[rnd % 2])
    # two threads, a lock around each call (the caller's Map::mMutexMapUpdate)
    lock, turn, errors = threading.Lock(), threading.Semaphore(0), []
    back = threading.Semaphore(0)

    def writer():
        try:
            for pts in (second, first, second):
                with lock:
                    update(pts)
                turn.release()
                back.acquire()
        except Exception as e:   # noqa: BLE001
            errors.append(e)
            turn.release()

    def reader():
        try:
            for rnd in (1, 0, 1):
                turn.acquire()
                with lock:
                    _equal_outputs(B.FuseMapPointsSim3Map(kfs, cams, poses, M, ids, T.TH, lsf), wants[rnd])
                back.release()
        except Exception as e:   # noqa: BLE001
            errors.append(e)
            back.release()

    ts = [threading.Thread(target=writer), threading.Thread(target=reader)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- 5. ComputeDistinctiveDescriptors straight into the table ----
def test_distinctive_descriptors_into_the_map(oracle, mono_scene):
    import orb_slam3_amd as osa
    from test_gpu_keyframe_distinctive import _mono
    D = DS.boundary_sets()
    n_sets = len(D["set_ptr"]) - 1
    rng = np.random.default_rng(9)
    m = osa.ORBmatcher(0.6, True)
    kfs = [_mono(osa, m, rng, d) for d in D["kf_desc"]]
    M = osa.DeviceMap(1024)
    set_id = np.ascontiguousarray(rng.permutation(1024)[:n_sets].astype(np.int32))
    before = _random_points(rng, n_sets)
    M.update(m, set_id, **before)
    best, desc = m.DistinctiveDescriptorsKeyFrames(kfs, D["set_ptr"], D["obs_kf"], D["obs_idx"])
    assert np.array_equal(best, oracle.distinctive_descriptors(D["rows"], D["set_ptr"]))
    got = m.DistinctiveDescriptorsKeyFramesToMap(kfs, D["set_ptr"], D["obs_kf"], D["obs_idx"], M, set_id)
    t = m.last_transfers()
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t
    assert np.array_equal(got, best) and (best < 0).sum() == 1
    after = M.read(m, set_id)
    want = dict(before, desc=np.where((best >= 0)[:, None], desc, before["desc"]))
    assert _same(after, want)
    # a following `_map` search uses the new descriptors: the scene's map points, their descriptors written by the call (one set per point, one
    # observation each: the row is the winner)
    c = mono_scene
    sc, sm, SM, ids = c["sc"], c["m"], c["M"], c["ids"]
    n = len(ids)
    new_desc = np.ascontiguousarray(sc["map_points"]["desc"][np.random.default_rng(10).permutation(n)])
    holder = _mono(osa, sm, rng, new_desc)
    one = np.arange(n + 1, dtype=np.int32)
    b1 = sm.DistinctiveDescriptorsKeyFramesToMap([holder], one, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), SM, ids)
    assert (b1 == 0).all()
    pts = dict(sc["map_points"], desc=new_desc)
    try:
        _equal_outputs(sm.FuseMapPointsSim3Map(c["kfs"], sc["cams"], sc["poses"], SM, ids, T.TH, sc["log_scale_factor"]),
                       sm.FuseMapPointsSim3(c["kfs"], sc["cams"], sc["poses"], pts, T.TH, sc["log_scale_factor"]))
    finally:
        SM.update(sm, ids, desc=sc["map_points"]["desc"])   # the fixture's table as the other tests expect it


def test_distinctive_into_the_map_with_a_bad_index_behind_pending_counts(oracle, batch):  # noqa: F811
    """Key-frame counts pending and an index equal to N: the kernel finds it, the call returns ORBX_E_BAD_ARG, nothing is written to the table, and
    the context, the key frames and the table go on working."""
    import orb_slam3_amd as osa
    m, host = batch["m"], batch["host"]
    nl, nr, rig_desc = host[0]
    rng = np.random.default_rng(12)
    M = osa.DeviceMap(64)
    set_id = np.array([5, 63, 0], np.int32)
    before = _random_points(rng, 3)
    M.update(m, set_id, **before)
    kf = [osa.DeviceKeyFrame.from_frame_fisheye(m, batch["rig_handles"][0], None)]
    with pytest.raises(osa.OrbxError) as e:
        m.DistinctiveDescriptorsKeyFramesToMap(kf, [0, 3, 4, 6], [0] * 6, [0, nl + nr, 1, 2, 3, 4], M, set_id)
    assert e.value.status == BAD
    assert _same(M.read(m, set_id), before)
    best = m.DistinctiveDescriptorsKeyFramesToMap(kf, [0, 3, 4, 6], [0] * 6, [0, nl + nr - 1, 1, 2, 3, nl], M, set_id)
    want, desc = m.DistinctiveDescriptorsKeyFrames(kf, [0, 3, 4, 6], [0] * 6, [0, nl + nr - 1, 1, 2, 3, nl])
    assert np.array_equal(best, want) and np.array_equal(M.read(m, set_id)["desc"], desc)
    assert np.array_equal(desc[1], rig_desc[2])


# ---- 6. the contract: every refusal leaves the transfer counters and the table alone ----
def _device_count():
    import torch
    try:
        return torch.cuda.device_count()
    except Exception:   # noqa: BLE001
        return 0


def test_contract(mono_scene):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    c = mono_scene
    sc, kfs = c["sc"], c["kfs"][:1]
    rng = np.random.default_rng(21)
    m = osa.ORBmatcher(0.6, True)
    M = osa.DeviceMap(256)
    live = np.array([0, 7, 100, 255, 31, 32], np.int32)
    pts = _random_points(rng, len(live))
    M.update(m, live, **pts)
    M.read(m, live)
    counters = m.last_transfers()
    h = C.c_void_p()
    assert L.orbx_map_create(0, _lib.MAX_MAP_POINTS + 1, C.byref(h)) == TOO_LARGE and not h.value
    assert L.orbx_map_create(0, 0, C.byref(h)) == BAD and L.orbx_map_create(0, 16, None) == BAD
    with pytest.raises(osa.OrbxError):
        osa.DeviceMap(_lib.MAX_MAP_POINTS + 1)

    out = {k: np.zeros_like(v) for k, v in pts.items()}
    p = {k: v.ctypes.data for k, v in pts.items()}

    def i32(*v):
        return np.array(v, np.int32)

    def update(ids, n=None, **fields):
        a = {k: (p[k] if k in fields or not fields else None) for k in FIELDS}
        return L.orbx_map_update(m._h, M._h, len(ids) if n is None else n, ids.ctypes.data if ids is not None else None, a["pos"], a["normal"],
                                 a["min_dist"], a["max_dist"], a["desc"])

    def read(ids, n=None):
        return L.orbx_map_read(m._h, M._h, len(ids) if n is None else n, ids.ctypes.data if ids is not None else None,
                               *[out[k].ctypes.data for k in FIELDS])

    def search(ids, n=None):
        from orb_slam3_amd._lib import Camera, FramePose
        n = len(ids) if n is None else n
        bi, bd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        cs, ps = (Camera * 1)(Camera(*[float(x) for x in sc["cams"][0]])), (FramePose * 1)(FramePose.make(*sc["poses"][0]))
        return L.orbx_keyframe_fuse_map_points_sim3_map(m._h, 1, m._kf_handles(kfs), cs, ps, 3.0, sc["log_scale_factor"], n, M._h,
                                                        ids.ctypes.data if ids is not None else None, None, bi.ctypes.data, bd.ctypes.data, None)

    def to_map(set_id):
        holder = c["kfs"][0]
        sp, ok, oi, best = i32(0, 1, 2), i32(0, 0), i32(0, 1), np.zeros(2, np.int32)
        return L.orbx_keyframe_distinctive_descriptors_to_map(m._h, 1, m._kf_handles([holder]), 2, sp.ctypes.data, ok.ctypes.data, oi.ctypes.data, M._h,
                                                              set_id.ctypes.data if set_id is not None else None, best.ctypes.data)

    refusals = []
    for bad in (i32(0, -1), i32(256, 7), i32(7, 8), i32(0, 2 ** 31 - 1)):   # below 0, at and above the capacity, never written
        refusals += [read(bad), search(bad), update(bad, desc=1), L.orbx_map_erase(M._h, 2, bad.ctypes.data), to_map(bad)]
    refusals += [update(i32(9), pos=1, normal=1, min_dist=1, max_dist=1)]          # a first update with a field missing
    refusals += [update(i32(7, 100, 7)), update(i32(40, 40))]                      # a duplicate id in an update
    refusals += [to_map(i32(7, 7))]                                                # a duplicate in set_id
    refusals += [read(None, 2), search(None, 2), update(None, 2), L.orbx_map_erase(M._h, 2, None), to_map(None)]   # NULL ids
    refusals += [L.orbx_map_read(m._h, None, 1, live.ctypes.data, *[None] * 5), L.orbx_map_update(None, M._h, 1, live.ctypes.data, *[None] * 5),
                 L.orbx_keyframe_fuse_map_points_sim3_map(m._h, 1, m._kf_handles(kfs), None, None, 3.0, 0.0, 2, None, live.ctypes.data, None, None, None,
                                                          None)]
    assert refusals and all(r == BAD for r in refusals), refusals
    assert m.last_transfers() == counters
    assert _same(M.read(m, live), pts)
    # an erased id, and one erased and rewritten with a field missing
    assert L.orbx_map_erase(M._h, 2, i32(7, 100).ctypes.data) == 0
    counters = m.last_transfers()
    gone = i32(0, 7)
    assert [read(gone), search(gone), update(gone, pos=1), L.orbx_map_erase(M._h, 2, gone.ctypes.data), to_map(gone),
            update(i32(100), pos=1, normal=1, min_dist=1, desc=1)] == [BAD] * 6
    assert m.last_transfers() == counters
    keep = np.array([0, 255, 31, 32], np.int32)
    assert _same(M.read(m, keep), _rows(pts, [0, 3, 4, 5]))
    M.update(m, i32(7), **_rows(pts, [1]))   # written whole again: live
    assert _same(M.read(m, i32(7, 0)), _rows(pts, [1, 0]))
    # n = 0
    counters = m.last_transfers()
    assert [update(i32(), 0), read(i32(), 0), L.orbx_map_erase(M._h, 0, None), search(i32(), 0),
            L.orbx_map_update(m._h, M._h, 0, None, *[None] * 5)] == [0] * 5
    assert m.last_transfers() == counters
    if _device_count() >= 2:   # a table of another device
        other = osa.DeviceMap(16, device=1)
        assert L.orbx_map_update(m._h, other._h, 1, i32(0).ctypes.data, *[p[k] for k in FIELDS]) == BAD
        assert L.orbx_map_read(m._h, other._h, 1, i32(0).ctypes.data, *[None] * 5) == BAD
        assert m.last_transfers() == counters


# ---- 7. transfers ----
def test_transfers_of_the_map_forms(mono_local, mono_scene):
    """orbx_matcher_debug_transfers counts run EXTENTS, alignment gaps between the buffers of a run included (matcher_context.h, flush_uploads), so
    the `_map` form's upload is 60 n_mp bytes smaller to within Layout's alignment per buffer: five arrays leave the run and the ids join it, six
    buffers.  Runs up and down, DMA submissions and k_xfer launches are equal -- the gather is not a k_xfer -- and do not depend on K.  (The counters
    hold no synchronisation count: every call ends in its one sync_and_deliver.)"""
    import orb_slam3_amd as osa
    c = mono_local
    m, cam10 = c["m"], FH.EUROC4 + (0, 0, 0, 0, 0, 0.0)
    sel = np.arange(N_LOCAL)
    mp = c["mp"]
    m.SearchLocalPoints(_mono_frame(osa, c, False), cam10, c["pose"], c["lsf"], 0.5, mp["pos"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"],
                        c["eligible"], c["has_obs"], 3.0, False, 0.0, c["occ"])
    flat = m.last_transfers()
    m.SearchLocalPointsMap(_mono_frame(osa, c, False), cam10, c["pose"], c["lsf"], 0.5, c["M"], c["ids"][sel], c["eligible"], c["has_obs"], 3.0, False, 0.0,
                           c["occ"])
    res = m.last_transfers()

    def compare(flat, res, n):
        assert abs((flat["upload_bytes"] - res["upload_bytes"]) - 60 * n) <= 6 * LAYOUT_ALIGN, (flat, res)
        for key in ("uploads", "downloads", "download_bytes", "dma_submissions", "xfer_launches"):
            assert flat[key] == res[key], (key, flat, res)
        assert res["uploads"] == 1 and res["downloads"] == 1 and res["dma_submissions"] == 0

    compare(flat, res, N_LOCAL)
    s = mono_scene
    sc, sm = s["sc"], s["m"]
    n = len(s["ids"])
    per_k = []
    for K in (1, 3):
        sm.FuseMapPoints(s["kfs"][:K], sc["cams"][:K], sc["poses"][:K], sc["map_points"], T.TH, sc["log_scale_factor"])
        flat = sm.last_transfers()
        sm.FuseMapPointsMap(s["kfs"][:K], sc["cams"][:K], sc["poses"][:K], s["M"], s["ids"], T.TH, sc["log_scale_factor"])
        res = sm.last_transfers()
        compare(flat, res, n)
        per_k.append({key: res[key] for key in ("uploads", "downloads", "dma_submissions", "xfer_launches")})
    assert per_k[0] == per_k[1], per_k
