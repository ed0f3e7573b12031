"""LoopClosing's Sim3 projection searches on FISHEYE-STEREO resident key frames: orbx_keyframe_search_by_projection_sim3_fisheye (both
SearchByProjection(KeyFrame*, Sim3f&, ...) overloads, ORBmatcher.cc:427-646) and orbx_keyframe_fuse_map_points_sim3_fisheye (SearchAndFuse's Fuse,
:1339-1455).  The members read the left camera only: a key frame is its left view, left features and N_left, the caller's rows span N_left + N_right.

The reference is COMPOSED in tests/sim3_fisheye_scene.py from the oracle and float32 numpy, independent of the code under test.  Every comparison is
equality of integers or of float bit patterns; no pair is left out, except that proj_u / proj_v are compared only where projected == 1.  The tests
that use only host arrays also run on the CPU emulator (ORBX_TEST_EMULATOR=1)."""
import ctypes as C
import os

import numpy as np
import pytest

import sim3_fisheye_scene as SF
import test_gpu_keyframe_fisheye as TF

pytestmark = pytest.mark.gpu

f32 = np.float32
TH_LOW = SF.TH_LOW
BAD, TOO_LARGE = -2, -7
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes(oracle):
    """seed -> the scene with equal bounds (the search form's limit); its conditions are asserted on the reference's output"""
    out = {}
    for seed, K in SF.SEEDS.items():
        sc = SF.make_scene(oracle, seed, K)
        SF.check_conditions(oracle, sc, range(K))
        out[seed] = sc
    return out


@pytest.fixture(scope="module")
def fuse_scenes(oracle):
    """seed -> the same scene with test_gpu_keyframe_fisheye.BOUNDS: key frame 1 has bounds of its own"""
    return {seed: SF.make_scene(oracle, seed, K, bounds=TF.BOUNDS[:K]) for seed, K in SF.SEEDS.items()}


def _counts(sc, k):
    kf = sc["key_frames"][k]
    return len(kf["kps_left"]), len(kf["desc"])


def _flags(sc, K):
    """skip: every 11th pair; occupied (N entries): every 7th left feature and EVERY right-camera entry on even k, no row on odd k."""
    n = len(sc["map_points"]["pos"])
    skip = (np.arange(K * n).reshape(K, n) % 11 == 0).astype(np.uint8)
    occ = []
    for k in range(K):
        nl, N = _counts(sc, k)
        row = (np.arange(N) % 7 == 0).astype(np.uint8)
        row[nl:] = 1                                   # entries [N_left, N) must change nothing
        occ.append(row if k % 2 == 0 else None)
    return skip, occ


def _key_frames(osa, m, sc, ks, isg="scene"):
    return [TF._host_kf(osa, m, sc, k, isg) for k in ks]


def _search(m, kfs, sc, ks, th, ratio, form, skip=None, occ=None, **kw):
    return m.SearchByProjectionSim3KeyFramesFisheye(kfs, SF.left_views(sc, ks, form), sc["map_points"], th, ratio, sc["log_scale_factor"], form, skip,
                                                    occ, want_uv=True, **kw)


def _fuse(m, kfs, sc, ks, skip=None, **kw):
    return m.FuseMapPointsSim3Fisheye(kfs, SF.left_views(sc, ks), sc["map_points"], TF.TH, sc["log_scale_factor"], skip, **kw)


def _assert_search_equal(got, ref, sc=None, ks=None):
    nm, match, pr, (pu, pv) = got
    assert np.array_equal(pr, ref["projected"]), np.nonzero(pr != ref["projected"])
    on = ref["projected"] == 1
    assert np.array_equal(_bits(pu)[on], _bits(ref["u"])[on]) and np.array_equal(_bits(pv)[on], _bits(ref["v"])[on])
    for k, (a, b) in enumerate(zip(match, ref["match"])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, np.nonzero(a != b))      # all N entries: the right camera's are -1
        if sc is not None:
            nl, N = _counts(sc, ks[k])
            assert len(a) == N and (a[nl:] == -1).all()
    assert np.array_equal(nm, ref["nm"])


# ---- 1. the search form against the composed reference ----
@pytest.mark.parametrize("th,ratio", [(8.0, 1.5), (5.0, 1.0)])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("seed", sorted(SF.SEEDS))
def test_search_form_equals_the_composed_reference(oracle, scenes, seed, form, th, ratio):
    import orb_slam3_amd as osa
    sc, K = scenes[seed], SF.SEEDS[seed]
    ref = SF.search_reference(oracle, sc, range(K), th, ratio, form)
    assert ref["nm"].sum() >= (0.1 if form == 0 else 0.05) * ref["projected"].size
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    _assert_search_equal(_search(m, kfs, sc, range(K), th, ratio, form), ref, sc, range(K))
    # the optional outputs left out
    nm, match, pr, uv = m.SearchByProjectionSim3KeyFramesFisheye(kfs, SF.left_views(sc, range(K), form), sc["map_points"], th, ratio,
                                                                 sc["log_scale_factor"], form, want_projected=False)
    assert pr is None and uv is None and np.array_equal(nm, ref["nm"]) and all(np.array_equal(a, b) for a, b in zip(match, ref["match"]))


# ---- 2. flags; the rows of one call are independent problems, each today's window search on the left camera's host arrays ----
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("seed", sorted(SF.SEEDS))
def test_flags_against_the_composed_reference(oracle, scenes, seed, form):
    import orb_slam3_amd as osa
    sc, K, th, ratio = scenes[seed], SF.SEEDS[seed], 8.0, 1.5
    skip, occ = _flags(sc, K)
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    for s, o in ((skip, None), (None, occ), (skip, occ)):
        ref = SF.search_reference(oracle, sc, range(K), th, ratio, form, s, o)
        _assert_search_equal(_search(m, kfs, sc, range(K), th, ratio, form, s, o), ref, sc, range(K))
    # occupied entries in [N_left, N) change nothing: the same rows with those entries cleared
    cleared = [None if r is None else np.where(np.arange(len(r)) < _counts(sc, k)[0], r, 0).astype(np.uint8) for k, r in enumerate(occ)]
    a, b = _search(m, kfs, sc, range(K), th, ratio, form, skip, occ), _search(m, kfs, sc, range(K), th, ratio, form, skip, cleared)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("form", [0, 1])
def test_rows_are_independent_and_equal_the_host_pointer_window_search(oracle, scenes, form):
    import orb_slam3_amd as osa
    sc, K, th, ratio = scenes[5], 3, 8.0, 1.5
    skip, occ = _flags(sc, K)
    ref = SF.search_reference(oracle, sc, range(K), th, ratio, form, skip, occ)
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    nm3, match3, pr3, (pu3, pv3) = _search(m, kfs, sc, range(K), th, ratio, form, skip, occ)
    for k in range(K):
        nm1, match1, pr1, (pu1, pv1) = _search(m, [kfs[k]], sc, [k], th, ratio, form, skip[k:k + 1], [occ[k]])
        assert nm1[0] == nm3[k] and np.array_equal(match1[0], match3[k]) and np.array_equal(pr1[0], pr3[k])
        assert np.array_equal(_bits(pu1[0]), _bits(pu3[k])) and np.array_equal(_bits(pv1[0]), _bits(pv3[k]))
        sel, q = ref["recs"][k]
        kps, desc, nl, N = SF.left_side(sc, k)
        b = [float(x) for x in sc["bounds"][k]]
        hv = osa.FrameView(kps, desc, *b, sc["scale_factors"])                           # today's path: the left camera's host arrays go up
        n, mm = m.SearchByProjectionWindow(hv, q, float(f32(TH_LOW) * f32(ratio)), False, None if occ[k] is None else occ[k][:nl])
        assert n == nm3[k] and np.array_equal(np.where(mm >= 0, sel[np.maximum(mm, 0)], -1), match3[k][:nl]), k
        assert n > 30 and (match3[k][nl:] == -1).all()


# ---- 3. the Fuse form: key frames with bounds of their own in one call ----
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("seed", sorted(SF.SEEDS))
def test_fuse_form_equals_the_composed_reference(oracle, fuse_scenes, seed, with_skip):
    import orb_slam3_amd as osa
    sc, K = fuse_scenes[seed], SF.SEEDS[seed]
    assert K == 1 or not np.array_equal(sc["bounds"][0], sc["bounds"][1])
    skip = _flags(sc, K)[0] if with_skip else None
    bi, bd, pr, recs = SF.fuse_reference(oracle, sc, range(K), TF.TH, skip)
    assert pr.mean() >= 0.5 and (bd <= TH_LOW).mean() >= 0.2
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    gi, gd, gp = _fuse(m, kfs, sc, range(K), skip)
    assert np.array_equal(gp, pr), np.nonzero(gp != pr)
    assert np.array_equal(gi, bi) and np.array_equal(gd, bd)
    for k in range(K):                                                                   # never a right-camera index, never an N_left offset
        assert (gi[k] < _counts(sc, k)[0]).all()
    # == the gate-less search on resident rig key frames fed the reference's queries for the left camera and none for the right one
    nothing = {key: val[:0] for key, val in recs[0][1].items()}
    rows = m.FuseSearchKeyFramesFisheye(kfs, [(q, nothing) for _, q in recs], use_chi2=False)
    for k, ((sel, _), ((ri, rd), _)) in enumerate(zip(recs, rows)):
        assert np.array_equal(ri, gi[k, sel]) and np.array_equal(rd, gd[k, sel]), k
    # key frames made WITHOUT inv_level_sigma2: the same rows
    oi, od, op = _fuse(m, _key_frames(osa, m, sc, range(K), None), sc, range(K), skip)
    assert np.array_equal(oi, bi) and np.array_equal(od, bd) and np.array_equal(op, pr)
    si, sd, sp = _fuse(m, kfs, sc, range(K), skip, want_projected=False)
    assert sp is None and np.array_equal(si, bi) and np.array_equal(sd, bd)
    if K > 1:
        with pytest.raises(osa.OrbxError):   # the search form takes one set of grid parameters per launch
            _search(m, kfs, sc, range(K), 8.0, 1.5, 0)


# ---- 4. key frames made three ways ----
def test_key_frames_from_a_reloaded_handle_give_the_rows_of_host_made_ones(oracle, scenes):
    import orb_slam3_amd as osa
    sc, K, th, ratio = scenes[6], 3, 8.0, 1.5
    skip, occ = _flags(sc, K)
    m = osa.ORBmatcher(0.6, True)
    D = osa.DeviceFrame(m, max(len(kf["desc"]) for kf in sc["key_frames"]) + 50)
    kfs = []
    for k in range(K):
        TF._load(osa, D, sc, k)
        kfs.append(osa.DeviceKeyFrame.from_frame_fisheye(m, D, None if k == 1 else sc["inv_level_sigma2"]))
    TF._load(osa, D, sc, 0)                                    # the handle holds another frame before anything is searched
    assert [kf.counts() for kf in kfs] == [(_counts(sc, k)[0], _counts(sc, k)[1] - _counts(sc, k)[0]) for k in range(K)]
    host = _key_frames(osa, m, sc, range(K))
    for form in (0, 1):
        got, want = _search(m, kfs, sc, range(K), th, ratio, form, skip, occ), _search(m, host, sc, range(K), th, ratio, form, skip, occ)
        ref = SF.search_reference(oracle, sc, range(K), th, ratio, form, skip, occ)
        _assert_search_equal(got, ref, sc, range(K))
        _assert_search_equal(want, ref, sc, range(K))
    bi, bd, pr, _ = SF.fuse_reference(oracle, sc, range(K), TF.TH, skip)
    for these in (kfs, host):
        gi, gd, gp = _fuse(m, these, sc, range(K), skip)
        assert np.array_equal(gp, pr) and np.array_equal(gi, bi) and np.array_equal(gd, bd)


@pytest.mark.skipif(EMULATOR, reason="extracts on the device")
def test_key_frames_from_a_batch_loaded_handle_with_their_counts_pending(oracle):
    """Rig key frames from a batch-loaded 320 x 240 pair: both counts on the device only, the right rows behind a gap (at the left extractor's
    capacity).  200 map points on features of the pair.  Each form must give the rows of a key frame rebuilt from the downloaded arrays; the Fuse
    form brings the counts home with its results, the search form through orbx_keyframe_counts' path."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from test_gpu_frame_fisheye import _extract_pairs
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    w, h, nf = 320, 240, 500
    left, right = _extract_pairs(w, h, 2, nf)
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    exl.extract_batch_device(left.data_ptr(), 2, w, h, w, w * h, (0, 0))
    exr.extract_batch_device(right.data_ptr(), 2, w, h, w, w * h, (0, 0))
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    sf = exl.GetScaleFactors().astype(f32)
    bounds = (0.0, float(w), 0.0, float(h))
    m = osa.ORBmatcher(0.6, True)
    cap = exl.batch_view().cap + exr.batch_view().cap
    D = osa.DeviceFrame(m, cap).load_stereo_fisheye_batch(exl, exr, 0, bounds=bounds, scale_factors=sf)   # the counts stay on the device
    for_fuse, for_search = [osa.DeviceKeyFrame.from_frame_fisheye(m, D, None) for _ in range(2)]
    D.load_stereo_fisheye_batch(exl, exr, 1, bounds=bounds, scale_factors=sf)                              # reloaded before the search
    _, kl, dl = exl.download(0)
    _, kr, dr = exr.download(0)
    nl, nr = len(kl), len(kr)
    assert min(nl, nr) >= 100 and nl < exl.batch_view().cap                                                # the row gap
    want = osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kl, np.concatenate([dl, dr]).reshape(-1, 32), *bounds, sf), kr, None)
    sc = synth.make_fisheye_fuse_scene(np.random.default_rng(9), 1, 8, n_clutter=0)   # (the rig: views and the scale pyramid)
    view = sc["views"][0]
    mp = TF._points_on_features(np.random.default_rng(13), view, (kl, kr), (dl, dr), sf, 100)
    lv = [view[0]]
    gi, gd, gp = m.FuseMapPointsSim3Fisheye([for_fuse], lv, mp, TF.TH, sc["log_scale_factor"])            # no synchronisation before this search
    t = m.last_transfers()
    assert t["uploads"] == 1 and t["downloads"] == 2                                                     # the results, and the 8 bytes of the counts
    assert for_fuse.counts() == (nl, nr) and for_fuse.count() == nl + nr                                  # known afterwards ...
    assert m.last_transfers() == t                                                                        # ... at no cost
    ei, ed, ep = m.FuseMapPointsSim3Fisheye([want], lv, mp, TF.TH, sc["log_scale_factor"])
    assert np.array_equal(gp, ep) and np.array_equal(gi, ei) and np.array_equal(gd, ed)
    assert gp.sum() > 100 and (gd[0] <= TH_LOW).sum() > 50 and (gi < nl).all()
    for form in (0, 1):
        views = [(view[0][0], view[0][1], view[0][2], view[0][3])]
        kf = for_search if form == 0 else for_fuse
        a = m.SearchByProjectionSim3KeyFramesFisheye([kf], views, mp, 8.0, 1.5, sc["log_scale_factor"], form, want_uv=True)
        b = m.SearchByProjectionSim3KeyFramesFisheye([want], views, mp, 8.0, 1.5, sc["log_scale_factor"], form, want_uv=True)
        assert a[0][0] == b[0][0] and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[2], b[2])
        assert np.array_equal(_bits(a[3][0]), _bits(b[3][0])) and np.array_equal(_bits(a[3][1]), _bits(b[3][1]))
        assert len(a[1][0]) == nl + nr and (a[1][0][nl:] == -1).all()
        if form == 0:
            assert a[0][0] > 50
    assert for_search.counts() == (nl, nr)


# ---- 5. refusals: each returns before anything is enqueued ----
def test_refusals_enqueue_nothing(scenes):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    sc = scenes[5]
    mp = sc["map_points"]
    n = len(mp["pos"])
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(3))
    kl, dl, nl0, _ = SF.left_side(sc, 0)
    b = [float(x) for x in sc["bounds"][0]]
    # every key frame a refusal needs is made FIRST: making one stages an upload, which starts the counters anew
    mono = osa.DeviceKeyFrame.from_host(m, osa.FrameView(kl, dl, *b, sc["scale_factors"]), None)
    kf1 = sc["key_frames"][1]
    odd = osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kf1["kps_left"], kf1["desc"], 0.0, 512.0, 0.0, 512.5, sc["scale_factors"]),
                                               kf1["kps_right"], None)                              # other image bounds
    nbig = 16000 + 1                                                                                # more LEFT features than ORBX_MAX_FRAME_FEATURES
    kb = np.zeros(nbig, osa.KP_DTYPE)
    kb["x"], kb["y"] = np.random.default_rng(3).uniform(1, 500, (2, nbig)).astype(f32)
    huge = osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kb, np.zeros((nbig + 1, 32), np.uint8), *b, sc["scale_factors"]),
                                                np.zeros(1, osa.KP_DTYPE), None)
    m1 = osa.ORBmatcher(0.6, True, device=1) if _device_count() > 1 else None                       # a second GPU, where there is one
    far = TF._host_kf(osa, m1, sc, 0) if m1 is not None else None
    _fuse(m, kfs[:1], sc, [0])                                                                      # the last call that enqueues anything
    made = m.last_transfers()
    assert made["uploads"] == 1 and made["downloads"] == 1

    def unchanged():
        assert m.last_transfers() == made, (m.last_transfers(), made)

    vp = C.c_void_p
    hs = lambda *k: (vp * len(k))(*[None if x is None else x._h.value if isinstance(x._h, vp) else x._h for x in k])   # noqa: E731
    nmax = _lib.MAX_FUSE_KEYFRAMES
    views = np.zeros(23 * (nmax + 1), f32)
    for k, v in enumerate(SF.left_views(sc, range(3))):
        views[23 * k:23 * (k + 1)] = np.concatenate([np.asarray(x, f32).ravel() for x in v])
    pts = [mp["pos"].ctypes.data, mp["normal"].ctypes.data, mp["min_dist"].ctypes.data, mp["max_dist"].ctypes.data, mp["desc"].ctypes.data]
    rows_np = [np.full(600, 7, np.int32) for _ in range(3)]
    rows = (vp * 3)(*[r.ctypes.data for r in rows_np])
    nm = np.full(3, 7, np.int32)
    bi, bd = np.full(3 * n, 7, np.int32), np.full(3 * n, 7, np.int32)
    uv = np.zeros(3 * n, f32)

    def search(K, h, form=0, r=rows, n_mp=n, nmp=nm.ctypes.data, pu=None, pv=None, points=pts, v=views.ctypes.data):
        return L.orbx_keyframe_search_by_projection_sim3_fisheye(m._h, K, h, v, 8.0, 1.5, 0.18, form, n_mp, *points, None, None, r, nmp, None, pu, pv)

    def fuse(K, h, n_mp=n, out=bi.ctypes.data, points=pts, v=views.ctypes.data):
        return L.orbx_keyframe_fuse_map_points_sim3_fisheye(m._h, K, h, v, 3.0, 0.18, n_mp, *points, None, out, bd.ctypes.data, None)

    assert search(2, hs(kfs[0], mono)) == BAD and fuse(2, hs(kfs[0], mono)) == BAD                   # a monocular key frame
    unchanged()
    assert search(2, hs(kfs[0], None)) == BAD and fuse(2, hs(kfs[0], None)) == BAD                   # a NULL key frame
    unchanged()
    assert search(1, None) == BAD and fuse(1, None) == BAD                                          # NULL rows: the key frames,
    assert search(1, hs(kfs[0]), v=None) == BAD and fuse(1, hs(kfs[0]), v=None) == BAD              # the views,
    assert search(1, hs(kfs[0]), r=None) == BAD                                                     # the match rows,
    assert search(2, hs(*kfs[:2]), r=(vp * 3)(rows_np[0].ctypes.data, None, None)) == BAD           # one match row,
    assert search(1, hs(kfs[0]), nmp=None) == BAD and fuse(1, hs(kfs[0]), out=None) == BAD          # the outputs,
    assert search(1, hs(kfs[0]), points=[None] + pts[1:]) == BAD and fuse(1, hs(kfs[0]), points=[None] + pts[1:]) == BAD   # the map points
    unchanged()
    assert search(1, hs(kfs[0]), form=2) == BAD and search(1, hs(kfs[0]), form=-1) == BAD           # projection_form not 0 / 1
    unchanged()
    assert search(1, hs(kfs[0]), pu=uv.ctypes.data) == BAD and search(1, hs(kfs[0]), pv=uv.ctypes.data) == BAD   # proj_u without proj_v
    unchanged()
    assert search(2, hs(kfs[0], odd)) == BAD                                                        # unequal bounds in the search form
    unchanged()
    many = (vp * (nmax + 1))(*[kfs[0]._h.value if isinstance(kfs[0]._h, vp) else kfs[0]._h] * (nmax + 1))
    big_rows = (vp * (nmax + 1))(*[rows_np[0].ctypes.data] * (nmax + 1))
    big_nm = np.full(nmax + 1, 7, np.int32)
    big = np.full((nmax + 1) * 4, 7, np.int32)
    assert search(nmax + 1, many, r=big_rows, nmp=big_nm.ctypes.data, n_mp=4) == TOO_LARGE           # too many key frames
    assert L.orbx_keyframe_fuse_map_points_sim3_fisheye(m._h, nmax + 1, many, views.ctypes.data, 3.0, 0.18, 4, *pts, None, big.ctypes.data,
                                                        big.ctypes.data, None) == TOO_LARGE
    unchanged()
    # too many features for the replay: more LEFT features than ORBX_MAX_FRAME_FEATURES (the Fuse form has no such limit below 65535)
    hrow = np.full(nbig + 1, 7, np.int32)
    assert search(1, hs(huge), r=(vp * 1)(hrow.ctypes.data)) == TOO_LARGE and np.all(hrow == 7)
    unchanged()
    if far is not None:                                                                             # a key frame of another device
        assert search(1, hs(far)) == BAD and fuse(1, hs(far)) == BAD
        unchanged()
    assert all(np.all(r == 7) for r in rows_np) and np.all(nm == 7) and np.all(bi == 7) and np.all(big_nm == 7)   # a refused call writes nothing
    # the two calls for monocular key frames keep refusing a rig key frame
    cams = (_lib.Camera * 1)(_lib.Camera(190.0, 190.0, 255.0, 255.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    poses = (_lib.FramePose * 1)(_lib.FramePose.make(np.eye(3, dtype=f32), np.zeros(3, f32), np.zeros(3, f32)))
    assert L.orbx_keyframe_search_by_projection_sim3(m._h, 1, hs(kfs[0]), cams, poses, 8.0, 1.5, 0.18, 0, n, *pts, None, None, rows, nm.ctypes.data,
                                                     None, None, None) == BAD
    assert L.orbx_keyframe_fuse_map_points_sim3(m._h, 1, hs(kfs[0]), cams, poses, 3.0, 0.18, n, *pts, None, bi.ctypes.data, bd.ctypes.data, None) == BAD
    unchanged()
    # n_kf = 0 and n_mp = 0 are fine: rows all -1, nmatches 0
    assert search(0, None, r=None, nmp=None, v=None) == 0 and fuse(0, None, out=None, v=None) == 0
    assert search(2, hs(*kfs[:2]), n_mp=0) == 0 and fuse(2, hs(*kfs[:2]), n_mp=0) == 0
    for k in range(2):
        N = _counts(sc, k)[1]
        assert np.all(rows_np[k][:N] == -1) and np.all(rows_np[k][N:] == 7) and nm[k] == 0
    unchanged()


def _device_count():
    if EMULATOR:
        return 1
    import torch
    return torch.cuda.device_count()


# ---- 6. degenerate shapes ----
def test_degenerate_shapes(oracle, scenes):
    import orb_slam3_amd as osa
    sc = scenes[7]
    m = osa.ORBmatcher(0.6, True)
    kf0 = sc["key_frames"][0]
    nl, N = _counts(sc, 0)
    b = [float(x) for x in sc["bounds"][0]]
    sfs = sc["scale_factors"]
    no_right = osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kf0["kps_left"], kf0["desc"][:nl], *b, sfs), kf0["kps_right"][:0], None)
    no_left = osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kf0["kps_left"][:0], kf0["desc"][nl:], *b, sfs), kf0["kps_right"], None)
    full = TF._host_kf(osa, m, sc, 0)
    assert no_right.counts() == (nl, 0) and no_left.counts() == (0, N - nl)
    v0 = SF.left_views(sc, [0])[0]
    mp = sc["map_points"]
    n = len(mp["pos"])
    bi, bd, pr, _ = SF.fuse_reference(oracle, sc, [0], TF.TH)
    gi, gd, gp = m.FuseMapPointsSim3Fisheye([no_right, no_left, full], [v0] * 3, mp, TF.TH, sc["log_scale_factor"])
    assert np.array_equal(gp, np.stack([pr[0]] * 3))                          # the projection does not depend on the features
    assert np.array_equal(gi[0], bi[0]) and np.array_equal(gd[0], bd[0]) and np.array_equal(gi[2], bi[0]) and np.array_equal(gd[2], bd[0])
    assert (gi[1] == -1).all() and (gd[1] == 256).all()                       # no left features: nothing to find
    for form in (0, 1):
        ref = SF.search_reference(oracle, sc, [0], 8.0, 1.5, form)
        v = SF.left_views(sc, [0], form)[0]
        nm, match, gp, _ = m.SearchByProjectionSim3KeyFramesFisheye([no_right, no_left, full], [v] * 3, mp, 8.0, 1.5, sc["log_scale_factor"], form)
        assert np.array_equal(gp, np.stack([ref["projected"][0]] * 3))
        assert nm[0] == ref["nm"][0] and np.array_equal(match[0], ref["match"][0][:nl]) and len(match[0]) == nl
        assert nm[1] == 0 and len(match[1]) == N - nl and (match[1] == -1).all()
        assert nm[2] == ref["nm"][0] and np.array_equal(match[2], ref["match"][0])
    none = dict(pos=np.zeros((0, 3), f32), normal=np.zeros((0, 3), f32), min_dist=np.zeros(0, f32), max_dist=np.zeros(0, f32), desc=np.zeros((0, 32), np.uint8))
    gi, gd, gp = m.FuseMapPointsSim3Fisheye([full], [v0], none, TF.TH, sc["log_scale_factor"])
    assert gi.shape == (1, 0)
    nm, match, gp, _ = m.SearchByProjectionSim3KeyFramesFisheye([full], [v0], none, 8.0, 1.5, sc["log_scale_factor"])
    assert nm[0] == 0 and len(match[0]) == N and (match[0] == -1).all()
    gi, gd, gp = m.FuseMapPointsSim3Fisheye([], [], mp, TF.TH, sc["log_scale_factor"])
    assert gi.shape == (0, n)
    nm, match, gp, _ = m.SearchByProjectionSim3KeyFramesFisheye([], [], mp, 8.0, 1.5, sc["log_scale_factor"])
    assert len(nm) == 0 and match == []


# ---- 7. the cost does not grow with K ----
def test_transfer_submissions_do_not_depend_on_k(scenes):
    import orb_slam3_amd as osa
    sc = scenes[5]
    skip, occ = _flags(sc, 3)
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(3))
    ts, tf = {}, {}
    for K in (1, 3):
        _search(m, kfs[:K], sc, range(K), 8.0, 1.5, 1, skip[:K], occ[:K])
        ts[K] = m.last_transfers()
        _fuse(m, kfs[:K], sc, range(K), skip[:K])
        tf[K] = m.last_transfers()
    for t in (ts, tf):
        assert t[1]["uploads"] == t[3]["uploads"] == 1 and t[1]["downloads"] == t[3]["downloads"] == 1, t
        assert t[1]["xfer_launches"] + t[1]["dma_submissions"] == t[3]["xfer_launches"] + t[3]["dma_submissions"] == 2, t
    n = len(sc["map_points"]["pos"])
    assert ts[1]["upload_bytes"] >= 60 * n and tf[1]["upload_bytes"] >= 60 * n            # the map points do go up (once)
    assert ts[3]["upload_bytes"] - ts[1]["upload_bytes"] < 60 * n                           # ... and not once per key frame
    assert tf[3]["upload_bytes"] - tf[1]["upload_bytes"] < 60 * n
    if "launches" in tf[1]:
        assert tf[1]["launches"] == tf[3]["launches"] and ts[1]["launches"] == ts[3]["launches"]
