"""Rectified-stereo and RGB-D depth on resident frames: orbx_rgbd_batch_device (Frame::ComputeStereoFromRGBD on the extractor's batch),
orbx_frame_load_stereo_batch / orbx_frame_load_host_stereo (mvuRight, mvDepth and the raw key points on the frame handle) and
orbx_frame_unproject_stereo (Frame::UnprojectStereo for a whole frame), against tests/stereo_resident_scene.py's float32 restatements.  Floats are
compared as uint32 bits.  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

import stereo_resident_scene as S

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD = -2             # ORBX_E_BAD_ARG
SENTINEL = f32(7.25)
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))
VIEW = S.view_of(11, S.CAMERA[:4])


def _view_tuple(v):
    return (v["R"], v["t"], v["Ow"], *[float(x) for x in v["p"]])


@pytest.fixture(scope="module")
def rgbd(canvas1):
    """One extractor with a distorting camera, a batch of 3 frames, the RGB-D stage on it; everything the tests read of it, downloaded once."""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    ex = osa.ORBextractor(500, 1.2, 8, 20, 7)
    ex.set_camera(S.CAMERA)
    frames = np.stack([synth.frame_from_canvas(canvas1, 5 * t, S.W, S.H, 700 + t) for t in range(S.FRAMES)])
    d_frames = torch.from_numpy(frames).cuda()
    imgs = S.depth_images()
    d_depth = torch.from_numpy(imgs).cuda()
    ex.extract_batch_device(d_frames.data_ptr(), S.FRAMES, S.W, S.H, S.W, S.W * S.H, (0, 0))
    ex.RGBDBatch(d_depth.data_ptr(), S.PITCH, S.PITCH * S.H, float(S.BF))
    host = []
    for f in range(S.FRAMES):
        _, k, d = ex.download(f)
        host.append(dict(kps=k, kps_un=ex.download_keypoints_un(f), desc=d, stereo=ex.stereo_download(f)))
    bv = ex.batch_view()
    return dict(ex=ex, host=host, imgs=imgs, keep=(d_frames, d_depth), cap=bv.cap, bounds=_bounds(ex), sf=ex.GetScaleFactors().astype(f32))


def _bounds(ex):
    from orb_slam3_amd import _lib
    b = np.zeros(4, f32)
    c = _lib.Camera(*[float(x) for x in S.CAMERA])
    assert _lib.lib().orbx_image_bounds(C.byref(c), S.W, S.H, _lib.ptr(b)) == 0
    return b


# ---- (1) the RGB-D stage ----
def test_rgbd_conditions_hold_on_the_reference_alone(rgbd):
    S.check_conditions_rgbd([(h["kps"], h["kps_un"]) for h in rgbd["host"]])


def test_rgbd_equals_the_member(rgbd):
    ex, cap = rgbd["ex"], rgbd["cap"]
    ur_all, d_all, nm_all = np.zeros((S.FRAMES, cap), f32), np.zeros((S.FRAMES, cap), f32), np.zeros(S.FRAMES, np.int32)
    ex.stereo_download_all(ur_all.ctypes.data, d_all.ctypes.data, nm_all.ctypes.data)
    for f, h in enumerate(rgbd["host"]):
        wur, wd, wn = S.reference_rgbd(rgbd["imgs"][f], h["kps"], h["kps_un"], S.BF)
        n = len(h["kps"])
        nm, ur, d = h["stereo"]
        assert nm == wn == nm_all[f], (f, nm, wn, nm_all[f])
        assert np.array_equal(S.bits(ur), S.bits(wur)) and np.array_equal(S.bits(d), S.bits(wd)), f
        assert np.array_equal(S.bits(ur_all[f, :n]), S.bits(wur)) and np.array_equal(S.bits(d_all[f, :n]), S.bits(wd)), f


def test_rgbd_refusals(rgbd):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    ex = rgbd["ex"]
    p = C.c_void_p(rgbd["keep"][1].data_ptr())
    fresh = osa.ORBextractor(500, 1.2, 8, 20, 7)                      # no batch yet
    refused = [L.orbx_rgbd_batch_device(None, p, S.PITCH, S.PITCH * S.H, 40.0), L.orbx_rgbd_batch_device(ex._h, None, S.PITCH, S.PITCH * S.H, 40.0),
               L.orbx_rgbd_batch_device(ex._h, p, 4 * S.W - 4, S.PITCH * S.H, 40.0), L.orbx_rgbd_batch_device(ex._h, p, S.PITCH, S.PITCH * S.H, 0.0),
               L.orbx_rgbd_batch_device(ex._h, p, S.PITCH, S.PITCH * S.H, -1.0), L.orbx_rgbd_batch_device(ex._h, p, S.PITCH, S.PITCH * S.H, float("nan")),
               L.orbx_rgbd_batch_device(fresh._h, p, S.PITCH, S.PITCH * S.H, 40.0)]
    assert refused == [BAD] * len(refused), refused
    nm, ur, d = ex.stereo_download(1)                                 # the results are the stage's still
    assert nm == rgbd["host"][1]["stereo"][0] and np.array_equal(S.bits(ur), S.bits(rgbd["host"][1]["stereo"][1]))


# ---- (2) the handle ----
def _host_view(osa, src, h, ur):
    return osa.FrameView(h["kps_un"], h["desc"], *[float(x) for x in src["bounds"]], src["sf"], ur)


def _queries(rng, h, ur, n_mp=300):
    """Map points projected near the frame's own features, with mTrackProjXR near the feature's mvuRight."""
    k = h["kps_un"]
    src = rng.integers(0, len(k), n_mp)
    px = (k["x"][src] + rng.normal(0, 1.0, n_mp)).astype(f32)
    pxr = np.where(ur[src] >= 0, px - (k["x"][src] - ur[src]) + rng.normal(0, 0.5, n_mp), 0).astype(f32)
    desc = h["desc"][src] ^ np.packbits(rng.random((n_mp, 256)) < 0.04, axis=1, bitorder="little")
    return dict(proj_x=px, proj_y=(k["y"][src] + rng.normal(0, 1.0, n_mp)).astype(f32), proj_xr=pxr, level=k["octave"][src].astype(np.int32),
                view_cos=np.full(n_mp, 0.9, f32), desc=desc, in_view=np.ones(n_mp, np.uint8), has_obs=np.ones(n_mp, np.uint8))


def _track_inputs(osa, m, src, h, ur, depth):
    """A last frame equal to the current one, its features with depth as map points at their unprojected place: they project back onto themselves."""
    pos, has = S.reference_unproject(np.stack([h["kps_un"]["x"], h["kps_un"]["y"]], axis=1), depth, VIEW)
    n = len(h["kps_un"])
    ids = np.where(has, np.arange(n), -1).astype(np.int32)
    M = osa.DeviceMap(n)
    sel = np.flatnonzero(has).astype(np.int32)
    M.update(m, sel, pos=pos[sel], normal=np.tile(f32([0, 0, 1]), (len(sel), 1)), min_dist=np.full(len(sel), 0.01, f32),
             max_dist=np.full(len(sel), 1e6, f32), desc=h["desc"][sel])
    last = osa.DeviceFrame(m, n).load(_host_view(osa, src, h, None))
    cam = (*S.CAMERA[:4], 0.0, 0.0, 0.0, 0.0, 0.0, float(S.BF))
    return M, ids, last, cam, (VIEW["R"], VIEW["t"], VIEW["Ow"])


def _handle_calls(osa, m, D, src, h, ur, depth, rng_seed, count_first):
    """Every call of the comparison on handle D, with its count pending (a batch load) or asked for first."""
    if count_first:
        assert D.count() == len(h["kps"])
    out = {}
    pos = np.full((D.cap, 3), SENTINEL, f32)
    out["unproject"] = m.UnprojectStereo(D, _view_tuple(VIEW), pos)
    t = m.last_transfers()
    assert t["uploads"] == 0 and t["dma_submissions"] <= 1 and t["downloads"] - t["dma_submissions"] == 1, t   # one run from the arena (+ a pending count)
    out["m1"] = m.SearchByProjection(D, _queries(np.random.default_rng(rng_seed), h, ur), 3.0)
    M, ids, last, cam, pose = _track_inputs(osa, m, src, h, ur, depth)
    out["m2"] = m.TrackLastFrame(D, last, cam, pose, M, ids, 7.0)[:2]
    return out


def _check_unproject(got, h, ur, depth, where):
    with_depth, gur, gd, gpos = got
    wpos, has = S.reference_unproject(np.stack([h["kps_un"]["x"], h["kps_un"]["y"]], axis=1), depth, VIEW)
    assert with_depth == int(has.sum()) and len(gur) == len(ur), where
    assert np.array_equal(S.bits(gur), S.bits(ur)) and np.array_equal(S.bits(gd), S.bits(depth)), where
    assert np.array_equal(S.bits(gpos[has]), S.bits(wpos[has])), where
    assert (gpos[~has] == SENTINEL).all(), where                      # rows without depth: the caller's values


@pytest.mark.parametrize("count_first", [False, True])
def test_rgbd_handle_batch_load_equals_host_load(rgbd, count_first):
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.9, True)
    for f in (0, 2):
        h = rgbd["host"][f]
        _, ur, depth = h["stereo"]
        raw_xy = np.stack([h["kps"]["x"], h["kps"]["y"]], axis=1).astype(f32)
        A = osa.DeviceFrame(m, rgbd["cap"]).load_stereo_batch(rgbd["ex"], f, rgbd["bounds"])
        B = osa.DeviceFrame(m, rgbd["cap"]).load_host_stereo(_host_view(osa, rgbd, h, ur), depth, raw_xy)
        a = _handle_calls(osa, m, A, rgbd, h, ur, depth, 40 + f, count_first)
        b = _handle_calls(osa, m, B, rgbd, h, ur, depth, 40 + f, True)
        _check_unproject(a["unproject"], h, ur, depth, ("batch", f))
        _check_unproject(b["unproject"], h, ur, depth, ("host", f))
        for key in ("m1", "m2"):
            assert a[key][0] == b[key][0] and np.array_equal(a[key][1], b[key][1]), (key, f)
            assert a[key][0] > 20, (key, f, a[key][0])


@pytest.fixture(scope="module")
def rectified():
    """A rectified pair through orbx_stereo_batch_device, small enough for the emulator: 2 frame pairs of 480 x 240."""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    B, w, h = 2, 480, 240
    canvas = synth.make_canvas(30, size=1200, n_shapes=900)
    pairs = [synth.make_stereo_pair(30, t, w, h, canvas) for t in range(B)]
    dl = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    dr = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    exl, exr = osa.ORBextractor(600, 1.2, 8, 20, 7), osa.ORBextractor(600, 1.2, 8, 20, 7)
    exl.extract_batch_device(dl.data_ptr(), B, w, h, w, w * h, (0, 0))
    exr.extract_batch_device(dr.data_ptr(), B, w, h, w, w * h, (0, 0))
    exl.stereo_batch_device(exr, float(S.BF), 0.15)
    host = []
    for f in range(B):
        _, k, d = exl.download(f)
        host.append(dict(kps=k, kps_un=k, desc=d, stereo=exl.stereo_download(f)))   # no camera set: mvKeysUn = mvKeys
    return dict(ex=exl, right=exr, host=host, keep=(dl, dr), cap=exl.batch_view().cap, bounds=np.array([0, w, 0, h], f32),
                sf=exl.GetScaleFactors().astype(f32), shape=(B, w, h))


@pytest.mark.parametrize("count_first", [False, True])
def test_rectified_handle_batch_load_equals_host_load(rectified, count_first):
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.9, True)
    r = rectified
    h = r["host"][1]
    nm, ur, depth = h["stereo"]
    assert nm > 30 and (depth > 0).sum() == nm
    A = osa.DeviceFrame(m, r["cap"]).load_stereo_batch(r["ex"], 1)
    B = osa.DeviceFrame(m, r["cap"]).load_host_stereo(_host_view(osa, r, h, ur), depth)     # keys_xy NULL: the undistorted points'
    a = _handle_calls(osa, m, A, r, h, ur, depth, 50, count_first)
    b = _handle_calls(osa, m, B, r, h, ur, depth, 50, True)
    _check_unproject(a["unproject"], h, ur, depth, "batch")
    _check_unproject(b["unproject"], h, ur, depth, "host")
    for key in ("m1", "m2"):
        assert a[key][0] == b[key][0] and np.array_equal(a[key][1], b[key][1]), key
        assert a[key][0] > 10, (key, a[key][0])


def test_stale_stage_is_refused_and_reloads_work_in_both_orders(rgbd):
    """Runs last on the rgbd fixture's extractor: it extracts again."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    m = osa.ORBmatcher(0.9, True)
    ex, cap = rgbd["ex"], rgbd["cap"]
    h = rgbd["host"][1]
    _, ur, depth = h["stereo"]
    D = osa.DeviceFrame(m, cap).load_stereo_batch(ex, 1, rgbd["bounds"])
    _check_unproject(m.UnprojectStereo(D, _view_tuple(VIEW), np.full((cap, 3), SENTINEL, f32)), h, ur, depth, "first")
    # a plain batch load on the same handle: no depth any more
    D.load_batch(ex, 1, rgbd["bounds"])
    before = m.last_transfers()
    pos = np.full((cap, 3), SENTINEL, f32)
    with pytest.raises(osa.OrbxError) as e:
        m.UnprojectStereo(D, _view_tuple(VIEW), pos)
    assert e.value.status == BAD and (pos == SENTINEL).all() and m.last_transfers() == before
    # ... and back, then a host load without depth, then the host load with it
    D.load_stereo_batch(ex, 1, rgbd["bounds"])
    _check_unproject(m.UnprojectStereo(D, _view_tuple(VIEW), np.full((cap, 3), SENTINEL, f32)), h, ur, depth, "again")
    D.load(_host_view(osa, rgbd, h, ur))
    with pytest.raises(osa.OrbxError):
        m.UnprojectStereo(D, _view_tuple(VIEW))
    D.load_host_stereo(_host_view(osa, rgbd, h, ur), depth, None)
    got = m.UnprojectStereo(D, _view_tuple(VIEW), np.full((cap, 3), SENTINEL, f32))
    _check_unproject(got, h, ur, depth, "host after plain")
    # refusals of the loads and of the call, nothing enqueued
    other, small = osa.ORBmatcher(0.9, True), osa.DeviceFrame(m, 8)
    v = m._new_points_views(_view_tuple(VIEW), _view_tuple(VIEW), False)[0][0]
    fd = _host_view(osa, rgbd, h, ur).c_struct()
    fd_mono = _host_view(osa, rgbd, h, None).c_struct()
    before = m.last_transfers()
    refused = [L.orbx_frame_unproject_stereo(None, D._h, C.byref(v), None, None, None, None), L.orbx_frame_unproject_stereo(m._h, None, C.byref(v), None, None, None, None),
               L.orbx_frame_unproject_stereo(m._h, D._h, None, None, None, None, None), L.orbx_frame_unproject_stereo(other._h, D._h, C.byref(v), None, None, None, None),
               L.orbx_frame_load_host_stereo(None, C.byref(fd), _lib.ptr(depth), None), L.orbx_frame_load_host_stereo(D._h, None, _lib.ptr(depth), None),
               L.orbx_frame_load_host_stereo(D._h, C.byref(fd), None, None), L.orbx_frame_load_host_stereo(D._h, C.byref(fd_mono), _lib.ptr(depth), None),
               L.orbx_frame_load_stereo_batch(None, ex._h, 1, None, None, 0), L.orbx_frame_load_stereo_batch(D._h, None, 1, None, None, 0),
               L.orbx_frame_load_stereo_batch(D._h, ex._h, -1, None, None, 0), L.orbx_frame_load_stereo_batch(D._h, ex._h, S.FRAMES, None, None, 0),
               L.orbx_frame_load_stereo_batch(small._h, ex._h, 1, None, None, 0)]
    assert refused == [BAD] * len(refused), refused
    assert m.last_transfers() == before
    _check_unproject(m.UnprojectStereo(D, _view_tuple(VIEW), np.full((cap, 3), SENTINEL, f32)), h, ur, depth, "after the refusals")
    assert L.orbx_frame_unproject_stereo(m._h, D._h, C.byref(v), None, None, None, None) == 0                # every output is optional
    # a new extraction without a stage: the stage's results are another batch's
    d_frames = rgbd["keep"][0]
    ex.extract_batch_device(d_frames.data_ptr(), S.FRAMES, S.W, S.H, S.W, S.W * S.H, (0, 0))
    assert L.orbx_frame_load_stereo_batch(D._h, ex._h, 1, None, None, 0) == BAD
    _check_unproject(m.UnprojectStereo(D, _view_tuple(VIEW), np.full((cap, 3), SENTINEL, f32)), h, ur, depth, "the handle keeps its copy")
    D.load_batch(ex, 1, rgbd["bounds"])                                # the plain load does not need one
    assert D.count() == len(h["kps"])
    ex.RGBDBatch(rgbd["keep"][1].data_ptr(), S.PITCH, S.PITCH * S.H, float(S.BF))
    D.load_stereo_batch(ex, 1, rgbd["bounds"])
    _check_unproject(m.UnprojectStereo(D, _view_tuple(VIEW), np.full((cap, 3), SENTINEL, f32)), h, ur, depth, "a stage on the new batch")


def test_two_contexts_on_two_threads(rgbd):
    import orb_slam3_amd as osa
    h = rgbd["host"][0]
    _, ur, depth = h["stereo"]
    errors = []
    turn = threading.Lock() if EMULATOR else contextlib.nullcontext()   # (the emulator runs a kernel's lanes as fibers of the calling thread)

    def worker(name):
        try:
            m = osa.ORBmatcher(0.9, True)
            D = osa.DeviceFrame(m, rgbd["cap"])
            for it in range(3):
                with turn:
                    D.load_host_stereo(_host_view(osa, rgbd, h, ur), depth, None)
                    got = m.UnprojectStereo(D, _view_tuple(VIEW), np.full((rgbd["cap"], 3), SENTINEL, f32))
                _check_unproject(got, h, ur, depth, (name, it))
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    t = threading.Thread(target=worker, args=("B",), daemon=True)
    t.start()
    worker("A")
    t.join(timeout=300)
    assert not t.is_alive(), "the second thread did not finish"
    assert not errors, errors


# ---- (3) key frames with depth and the stereo branches of CreateNewMapPoints ----
import new_points_scene as N  # noqa: E402

RECORD_STEREO = 592   # sizeof(NewPointsStereoRec): NewPoints (544) + two depth and two raw-xy pointers + mb, mbf of both key frames (orbx_matcher.hip asserts it)


def _pad(b):
    return (b + 255) // 256 * 256   # the arena's unit


def _stereo_pairs(m, sc, kfs, variant, n=None, idx1=None, idx2=None, pos=None):
    args, (inertial, far, th_far) = S.stereo_call(sc, variant)
    i1 = sc["idx1"][:n] if idx1 is None else idx1
    i2 = sc["idx2"][:n] if idx2 is None else idx2
    return m.TriangulatePairsKeyFramesStereo(kfs[0], kfs[1], *args, i1, i2, inertial, far, th_far, pos)


def _assert_pairs(got, want, where):
    """got = (n_accepted, pos, status) of a call whose pos went in filled with SENTINEL; want = (status, pos) of the reference."""
    acc, pos, st = got
    wst, wpos = want[0], want[1]
    assert np.array_equal(st, wst), (where, np.flatnonzero(st != wst)[:10], st[st != wst][:10], wst[st != wst][:10])
    ok = wst == N.OK
    assert acc == int(ok.sum()), (where, acc, int(ok.sum()))
    assert np.array_equal(S.bits(pos[ok]), S.bits(wpos[ok])), (where, np.flatnonzero((S.bits(pos) != S.bits(wpos)).any(axis=1) & ok)[:10])
    assert (pos[~ok] == SENTINEL).all(), where      # rejected pairs: the caller's values


@pytest.fixture(scope="module")
def kctx():
    """One context and the resident key frames of both seeds' scenes, made once."""
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.6, True)
    made = {}

    def get(seed):
        if seed not in made:
            sc = S.make_stereo_scene(seed)
            made[seed] = (sc, S.stereo_key_frames(osa, m, sc))
        return made[seed]
    return m, get


@pytest.mark.parametrize("n", S.PAIR_COUNTS)
def test_stereo_pairs_equal_the_reference(kctx, n):
    m, get = kctx
    sc, kfs = get(N.SEEDS[0])
    wst, wpos, info = S.stereo_reference(sc, "base")
    pos = np.full((n, 3), SENTINEL, f32)
    before = m.last_transfers()
    got = _stereo_pairs(m, sc, kfs, "base", n, pos=pos)
    assert got[1] is pos
    _assert_pairs(got, (wst[:n], wpos[:n]), n)
    t = m.last_transfers()
    if n == 0:
        assert t == before                          # nothing enqueued
        return
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t
    kf1, kf2 = sc["key_frames"]
    assert t["upload_bytes"] == 2 * _pad(4 * n) + _pad(4 * len(kf1["scale"])) + _pad(4 * len(kf2["scale"])) + RECORD_STEREO, t
    assert t["download_bytes"] == _pad(12 * n) + _pad(n) + 32, t
    # the existing form on the same key frames: the stereo pairs undecided, every other pair the same bits
    args, (inertial, far, th_far) = S.stereo_call(sc, "base")
    pos2 = np.full((n, 3), SENTINEL, f32)
    acc2, _, st2 = m.TriangulatePairsKeyFrames(kfs[0], kfs[1], *args[:5], sc["idx1"][:n], sc["idx2"][:n], inertial, far, th_far, pos2)
    stereo = info["path"][:n] != 0
    assert (st2[stereo] == N.STEREO_LEFT_TO_HOST).all() and (pos2[stereo] == SENTINEL).all()
    assert np.array_equal(st2[~stereo], got[2][~stereo]) and np.array_equal(S.bits(pos2[~stereo]), S.bits(pos[~stereo]))
    assert m.last_transfers()["upload_bytes"] == t["upload_bytes"] - (RECORD_STEREO - 544)


@pytest.mark.parametrize("variant", ["base", "inertial", "far", "turned", "shifted", "other_rig"])
def test_stereo_pairs_under_every_variant_on_the_second_seed(kctx, variant):
    m, get = kctx
    sc, kfs = get(N.SEEDS[1])
    want = S.stereo_reference(sc, variant)
    pos = np.full((len(sc["idx1"]), 3), SENTINEL, f32)
    _assert_pairs(_stereo_pairs(m, sc, kfs, variant, pos=pos), want, variant)
    if variant == "base":                            # repeated pairs, another order: a pair's outcome is its own
        order = np.concatenate([np.arange(90)[::-1], [5, 5, 5]])
        pos = np.full((len(order), 3), SENTINEL, f32)
        _assert_pairs(_stereo_pairs(m, sc, kfs, variant, idx1=sc["idx1"][order], idx2=sc["idx2"][order], pos=pos), (want[0][order], want[1][order]), "order")


def test_a_key_frame_without_depth_leaves_its_stereo_pairs_to_the_host(kctx):
    """from_host key frames hold mvuRight and no mvDepth: through the `_stereo` call a stereo observation on such a key frame is still
    STEREO_LEFT_TO_HOST, on the other key frame it is decided."""
    import orb_slam3_amd as osa
    m, get = kctx
    sc, kfs = get(N.SEEDS[0])
    n = 300
    wst, wpos, info = S.stereo_reference(sc, "base")
    kf1, kf2 = sc["key_frames"]
    s1 = kf1["u_right"][sc["idx1"][:n]] >= 0
    s2 = np.where(sc["idx2"][:n] >= 0, kf2["u_right"][np.maximum(sc["idx2"][:n], 0)] >= 0, False)
    for depth in ((False, True), (True, False), (False, False)):
        mixed = S.stereo_key_frames(osa, m, sc, depth)
        left = (s1 & (not depth[0])) | (s2 & (not depth[1]))
        want_st = np.where(left, N.STEREO_LEFT_TO_HOST, wst[:n]).astype(np.uint8)
        want_st[sc["idx2"][:n] < 0] = N.NO_MATCH
        pos = np.full((n, 3), SENTINEL, f32)
        _assert_pairs(_stereo_pairs(m, sc, mixed, "base", n, pos=pos), (want_st, wpos[:n]), depth)
        assert left.sum() >= 8


def _adhoc_stereo_scene(hosts, views, mb, mbf):
    """A scene for reference_stereo from frames made elsewhere: hosts = [dict(kps_un, kps, stereo=(n, ur, depth))] * 2."""
    kfs = []
    sf = N.scale_factors(8, 1.2)
    for h in hosts:
        k = h["kps_un"]
        kfs.append(dict(n_left=len(k), n_right=-1, x=k["x"].astype(f32), y=k["y"].astype(f32), octave=k["octave"].astype(np.int32), u_right=h["stereo"][1],
                        depth=h["stereo"][2], keys_xy=np.stack([h["kps"]["x"], h["kps"]["y"]], axis=1).astype(f32), scale=sf, sigma2=(sf * sf).astype(f32)))
    base = dict(views=views, ratio_factor=f32(1.8), inertial=0, far_points=0, th_far_points=0.0, mb=(f32(mb), f32(mb)), mbf=(f32(mbf), f32(mbf)))
    return dict(rig=False, key_frames=kfs, variants=dict(base=base))


def test_key_frames_from_depth_handles_with_pending_counts(rgbd):
    """orbx_keyframe_from_frame of handles loaded by orbx_frame_load_stereo_batch, their counts still on the device, against
    orbx_keyframe_create_host_stereo from the downloaded arrays and against the reference; a key frame from a handle without depth reports its
    stereo observations as before."""
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.6, True)
    ex, cap = rgbd["ex"], rgbd["cap"]
    hosts = [rgbd["host"][0], rgbd["host"][0]]                                       # the same frame twice, from two poses a step apart: pair (i, i) has parallel rays
    v1 = dict(S.view_of(21, S.CAMERA[:4]))
    v2 = dict(v1, Ow=(v1["Ow"] + f32([0.02, 0.0, -0.01])).astype(f32))
    v2["t"] = (-v2["R"].astype(np.float64) @ v2["Ow"].astype(np.float64)).astype(f32)
    sc = _adhoc_stereo_scene(hosts, [[v1], [v2]], 0.15, float(S.BF))
    rng = np.random.default_rng(77)
    n1, n2 = len(hosts[0]["kps"]), len(hosts[1]["kps"])
    same = rng.integers(0, n1, 100)
    idx1 = np.concatenate([[n1 - 1, 0], same, rng.integers(0, n1, 100)]).astype(np.int32)
    idx2 = np.concatenate([[0, n2 - 1], same, rng.integers(-1, n2, 100)]).astype(np.int32)
    want = S.reference_stereo(sc, "base", idx1, idx2)
    assert (want[2]["path"] >= 2).sum() >= 20 and (want[2]["path"] == 1).sum() >= 20 and (want[0] == N.OK).sum() >= 20, np.bincount(want[0])
    ex.RGBDBatch(rgbd["keep"][1].data_ptr(), S.PITCH, S.PITCH * S.H, float(S.BF))   # (an earlier test may have extracted again: the stage is this batch's)
    handles = [osa.DeviceFrame(m, cap).load_stereo_batch(ex, f, rgbd["bounds"]) for f in (0, 0)]
    pending = [osa.DeviceKeyFrame.from_frame(m, D, None) for D in handles]          # counts on the device only
    args = ((v1["R"], v1["t"], v1["Ow"], *[float(x) for x in v1["p"]]), (v2["R"], v2["t"], v2["Ow"], *[float(x) for x in v2["p"]]),
            sc["key_frames"][0]["sigma2"], sc["key_frames"][1]["sigma2"], 1.8, 0.15, float(S.BF), 0.15, float(S.BF))
    pos = np.full((len(idx1), 3), SENTINEL, f32)
    _assert_pairs(m.TriangulatePairsKeyFramesStereo(*pending, *args, idx1, idx2, pos=pos), want, "pending")
    assert [kf.count() for kf in pending] == [n1, n2]
    host_made = []
    for h in hosts:
        view = osa.FrameView(h["kps_un"], h["desc"], *[float(x) for x in rgbd["bounds"]], rgbd["sf"], h["stereo"][1])
        host_made.append(osa.DeviceKeyFrame.create_host_stereo(m, view, h["stereo"][2], np.stack([h["kps"]["x"], h["kps"]["y"]], axis=1).astype(f32), None))
    pos2 = np.full((len(idx1), 3), SENTINEL, f32)
    _assert_pairs(m.TriangulatePairsKeyFramesStereo(*host_made, *args, idx1, idx2, pos=pos2), want, "host")
    # an index N behind pending counts raises the flag: nothing is written, and everything goes on working
    again = [osa.DeviceKeyFrame.from_frame(m, D, None) for D in handles]
    bad = idx1.copy()
    bad[17] = n1
    pos3 = np.full((len(idx1), 3), SENTINEL, f32)
    with pytest.raises(osa.OrbxError) as e:
        m.TriangulatePairsKeyFramesStereo(*again, *args, bad, idx2, pos=pos3)
    assert e.value.status == BAD and (pos3 == SENTINEL).all()
    _assert_pairs(m.TriangulatePairsKeyFramesStereo(*again, *args, idx1, idx2, pos=pos3), want, "after the flag")
    # a handle without depth (a plain batch load has no mvuRight either; a host load with mvuRight): its key frame leaves stereo pairs to the host
    h = hosts[0]
    plain = osa.DeviceFrame(m, cap).load(osa.FrameView(h["kps_un"], h["desc"], *[float(x) for x in rgbd["bounds"]], rgbd["sf"], h["stereo"][1]))
    kf_plain = osa.DeviceKeyFrame.from_frame(m, plain, None)
    pos4 = np.full((len(idx1), 3), SENTINEL, f32)
    _, _, st4 = m.TriangulatePairsKeyFramesStereo(kf_plain, host_made[1], *args, idx1, idx2, pos=pos4)
    s1 = h["stereo"][1][idx1] >= 0
    assert (st4[s1 & (idx2 >= 0)] == N.STEREO_LEFT_TO_HOST).all() and (s1 & (idx2 >= 0)).sum() >= 50
    assert np.array_equal(st4[~s1], want[0][~s1])


def test_a_bad_octave_raises_the_flag(kctx):
    import orb_slam3_amd as osa
    m, get = kctx
    sc, _ = get(N.SEEDS[0])
    for side, octave in ((0, 8), (1, -1)):
        kfs_host = [dict(kf) for kf in sc["key_frames"]]
        hit = int(sc["idx1"][9] if side == 0 else sc["idx2"][9])
        kp = kfs_host[side]["kps"].copy()
        kp["octave"][hit] = octave
        kfs_host[side]["kps"] = kp
        kfs = S.stereo_key_frames(osa, m, dict(sc, key_frames=kfs_host))
        pos = np.full((64, 3), SENTINEL, f32)
        with pytest.raises(osa.OrbxError) as e:
            _stereo_pairs(m, sc, kfs, "base", 64, pos=pos)
        assert e.value.status == BAD and (pos == SENTINEL).all(), side
        pos = np.full((8, 3), SENTINEL, f32)
        wst, wpos, _ = S.stereo_reference(sc, "base")
        _assert_pairs(_stereo_pairs(m, sc, kfs, "base", 8, pos=pos), (wst[:8], wpos[:8]), side)


def test_fused_stereo_search_and_triangulate(oracle):
    """The BoW scene of the resident SearchForTriangulation tests with depth attached: the row and the return value are the plain search's, pos /
    status those of the pairs form fed with that row, and of the reference."""
    import orb_slam3_amd as osa
    from test_gpu_frame_bow import SF, Scene
    from test_gpu_keyframe_bow import ISG, SG, _stereo_pair
    bow = Scene(977, 600, 8, 4)
    m = osa.ORBmatcher(0.6, True)
    fx, fy, cx, cy, b = 458.654, 457.296, 367.215, 248.375, 0.11
    Kc = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    tx = np.array([[0, 0, 0], [0, 0, -b], [0, b, 0]])
    F = (np.linalg.inv(Kc).T @ tx @ np.linalg.inv(Kc)).astype(f32)
    eye = np.eye(3, dtype=f32)
    p4 = np.array([fx, fy, cx, cy], f32)
    views = [[dict(R=eye, t=np.zeros(3, f32), Ow=np.zeros(3, f32), p=p4)], [dict(R=eye, t=np.array([-b, 0, 0], f32), Ow=np.array([b, 0, 0], f32), p=p4)]]
    a, bq = _stereo_pair(oracle, m, bow, 2, 420, True)
    n = len(a.d)
    rng = np.random.default_rng(5)
    kfs_host, dev = [], []
    for kf in (a, bq):
        disp = kf.k["x"] - kf.ur
        depth = np.where(kf.ur >= 0, f32(b * fx) / np.where(kf.ur >= 0, disp, 1).astype(f32), f32(-1)).astype(f32)
        depth[(kf.ur >= 0) & (rng.random(n) < 0.1)] = 0.0                              # mvuRight >= 0 without a depth: UNPROJECT_FAILED where it is reached
        xy = (np.stack([kf.k["x"], kf.k["y"]], axis=1) + rng.choice([0.0, 0.5], (n, 2))).astype(f32)
        kfs_host.append(dict(n_left=n, n_right=-1, x=kf.k["x"].astype(f32), y=kf.k["y"].astype(f32), octave=kf.k["octave"].astype(np.int32), u_right=kf.ur,
                             depth=depth, keys_xy=xy, scale=SF, sigma2=SG))
        d = osa.DeviceKeyFrame.create_host_stereo(m, kf.view, depth, xy, ISG)
        d.compute_bow(m, bow.voc, 2, download=False)
        dev.append(d)
    base = dict(views=views, ratio_factor=f32(1.8), inertial=0, far_points=0, th_far_points=0.0, mb=(f32(b), f32(b)), mbf=(f32(b * fx), f32(b * fx)))
    sc = dict(rig=False, key_frames=kfs_host, variants=dict(base=base))
    v1 = (eye, views[0][0]["t"], views[0][0]["Ow"], fx, fy, cx, cy)
    v2 = (eye, views[1][0]["t"], views[1][0]["Ow"], fx, fy, cx, cy)
    seen = np.zeros(len(S.STATUS), np.int64)
    for coarse, skips in ((False, ((rng.random(n) < 0.3).astype(np.uint8), None)), (True, (None, None))):
        ep = (1e6, 1e6)
        nm, m12 = m.SearchForTriangulationResident(dev[0], dev[1], *skips, SG, F, ep, coarse, True)
        pm, pm12 = m.SearchForTriangulationResident(a.dev, bq.dev, *skips, SG, F, ep, coarse, True)     # the key frames without depth: the same search
        assert nm == pm and np.array_equal(m12, pm12) and nm > 40
        t_search = m.last_transfers()
        pos = np.full((n, 3), SENTINEL, f32)
        fn, fm12, acc, fpos, fst = m.SearchAndTriangulateResidentStereo(dev[0], dev[1], *skips, SG, SG, F, ep, v1, v2, 1.8, b, b * fx, b, b * fx, coarse, True,
                                                                        pos=pos)
        t_fused = m.last_transfers()
        assert fn == nm and np.array_equal(fm12, m12)
        idx1 = np.arange(n, dtype=np.int32)
        want = S.reference_stereo(sc, "base", idx1, m12)
        _assert_pairs((acc, fpos, fst), want, ("fused", coarse))
        ppos = np.full((n, 3), SENTINEL, f32)
        pacc, _, pst = m.TriangulatePairsKeyFramesStereo(dev[0], dev[1], v1, v2, SG, SG, 1.8, b, b * fx, b, b * fx, idx1, m12, pos=ppos)
        assert pacc == acc and np.array_equal(pst, fst) and np.array_equal(S.bits(ppos), S.bits(fpos))
        seen += np.bincount(want[0], minlength=len(S.STATUS))
        # one launch more than the search and nothing else: the record and kf1's level table ride up, pos / status / the flag come down beside the row
        assert t_fused["uploads"] == t_search["uploads"] == 1 and t_fused["downloads"] == t_search["downloads"] == 1, (t_search, t_fused)
        assert t_fused["upload_bytes"] - t_search["upload_bytes"] == _pad(4 * len(SG)) + _pad(RECORD_STEREO), (t_search, t_fused)
        assert t_fused["download_bytes"] - t_search["download_bytes"] == _pad(12 * n) + _pad(n) + 256, (t_search, t_fused)
        plain = m.SearchAndTriangulateResident(dev[0], dev[1], *skips, SG, SG, F, ep, v1, v2, 1.8, coarse, True)
        stereo = want[2]["path"] != 0
        assert (plain[4][stereo] == N.STEREO_LEFT_TO_HOST).all() and np.array_equal(plain[4][~stereo], fst[~stereo])
    assert seen[N.OK] > 20 and seen[N.NO_MATCH] > 100 and seen[N.STEREO_LEFT_TO_HOST] == 0 and (seen[2:] > 0).sum() >= 3, seen


def test_stereo_key_frames_shared_between_two_contexts_on_two_threads():
    import orb_slam3_amd as osa
    A = osa.ORBmatcher(0.6, True)
    sc = S.make_stereo_scene(N.SEEDS[0])
    kfs = S.stereo_key_frames(osa, A, sc)            # enqueued by A, handed over without a synchronisation
    want = S.stereo_reference(sc, "base")
    errors = []
    turn = threading.Lock() if EMULATOR else contextlib.nullcontext()

    def worker(name, m):
        try:
            for it in range(3):
                pos = np.full((len(sc["idx1"]), 3), SENTINEL, f32)
                with turn:
                    got = _stereo_pairs(m, sc, kfs, "base", pos=pos)
                _assert_pairs(got, want, (name, it))
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    t = threading.Thread(target=worker, args=("B", osa.ORBmatcher(0.6, True)), daemon=True)
    t.start()
    worker("A", A)
    t.join(timeout=300)
    assert not t.is_alive(), "the second thread did not finish"
    assert not errors, errors


def test_stereo_refusals_leave_the_transfer_counters_alone(kctx):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    from orb_slam3_amd._lib import KeyFrameGate, NewPointsParams, NewPointsStereo, NewPointsView, ptr
    L = _lib.lib()
    m, get = kctx
    sc, kfs = get(N.SEEDS[0])
    rig = N.device_key_frames(osa, m, N.make_scene(N.SEEDS[0], True))
    _stereo_pairs(m, sc, kfs, "base", 8)
    before = m.last_transfers()
    n = 8
    i1, i2 = np.ascontiguousarray(sc["idx1"][:n]), np.ascontiguousarray(sc["idx2"][:n])
    pos, st, acc = np.full((n, 3), SENTINEL, f32), np.full(n, 99, np.uint8), C.c_int32(-5)
    sg1, sg2 = sc["key_frames"][0]["sigma2"], sc["key_frames"][1]["sigma2"]
    par = NewPointsParams(1.8, 0, 0, 0.0, len(sg1), len(sg2), sg1.ctypes.data, sg2.ctypes.data)
    stp = NewPointsStereo(0.11, 55.0, 0.11, 55.0)
    v = NewPointsView()

    def call(kf1=kfs[0]._h, kf2=kfs[1]._h, v1=C.byref(v), p=par, s=C.byref(stp), n_=n, a=i1, b=i2, po=pos, mm=m._h):
        return L.orbx_keyframe_triangulate_pairs_stereo(mm, kf1, kf2, v1, C.byref(v), None if p is None else C.byref(p), s, n_, ptr(a), ptr(b), ptr(po),
                                                        ptr(st), C.byref(acc))
    high = i1.copy()
    high[3] = len(sc["key_frames"][0]["x"])
    wrong = NewPointsParams(1.8, 0, 0, 0.0, len(sg1) - 1, len(sg2), sg1.ctypes.data, sg2.ctypes.data)
    refused = [call(mm=None), call(kf1=None), call(kf2=None), call(v1=None), call(p=None), call(s=None), call(a=None), call(po=None), call(n_=-1),
               call(kf1=rig[0]._h), call(kf2=rig[1]._h), call(p=wrong), call(a=high)]
    g = KeyFrameGate((C.c_float * 9)(), 1e6, 1e6, 0, 1, len(sg2), sg2.ctypes.data)
    m12 = np.full(len(sc["key_frames"][0]["x"]), 77, np.int32)
    big_pos, big_st = np.full((len(m12), 3), SENTINEL, f32), np.full(len(m12), 99, np.uint8)

    def fused(kf1=kfs[0]._h, gate=C.byref(g), s=C.byref(stp), mt=m12):
        return L.orbx_keyframe_search_and_triangulate_stereo(m._h, kf1, kfs[1]._h, None, None, 1, gate, C.byref(v), C.byref(v), C.byref(par), s, ptr(mt),
                                                             ptr(big_pos), ptr(big_st), C.byref(acc))
    refused += [fused(), fused(kf1=None), fused(gate=None), fused(s=None), fused(mt=None)]   # (the key frames hold no BoW: the search refuses them)
    fd = osa.FrameView(sc["key_frames"][0]["kps"], sc["key_frames"][0]["desc"], 0.0, sc["W"], 0.0, sc["H"], sc["key_frames"][0]["scale"], None).c_struct()
    out = C.c_void_p(5)
    refused += [L.orbx_keyframe_create_host_stereo(m._h, C.byref(fd), ptr(sc["key_frames"][0]["depth"]), None, None, C.byref(out))]   # no mvuRight
    assert out.value is None
    assert refused == [BAD] * len(refused), refused
    assert m.last_transfers() == before
    assert (pos == SENTINEL).all() and (st == 99).all() and acc.value == -5 and (m12 == 77).all() and (big_pos == SENTINEL).all() and (big_st == 99).all()
    assert call(n_=0, a=None, b=None, po=None) == 0 and acc.value == 0 and m.last_transfers() == before
    want = S.stereo_reference(sc, "base")
    _assert_pairs(_stereo_pairs(m, sc, kfs, "base", n, pos=pos), (want[0][:n], want[1][:n]), "after the refusals")


def test_a_matcher_finalized_before_its_frames_destroys_them_first():
    """The collector of reference cycles finalizes a matcher and its DeviceFrames in any order (a traceback that holds both as locals is such a
    cycle): the matcher destroys the handles that are left before its context goes, and the frame's own finalizer then has nothing to do."""
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.9, True)
    D, E = osa.DeviceFrame(m, 16), osa.DeviceFrame(m, 16)
    h = D._h.value
    del E
    assert list(m._frames) == [h]
    m.__del__()                       # the owner first
    assert m._h is None and not m._frames
    D.__del__()
    assert D._h is None


def test_an_empty_frame_with_depth(rgbd):
    """n = 0 through orbx_frame_load_host_stereo: the handle has depth, UnprojectStereo returns nothing, and its key frame is made as the key frame of
    an empty handle without depth is (no launch of an empty grid)."""
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.9, True)
    empty = osa.FrameView(np.zeros(0, osa.KP_DTYPE), np.zeros((0, 32), np.uint8), 0.0, 320.0, 0.0, 240.0, rgbd["sf"], np.zeros(0, f32))
    D = osa.DeviceFrame(m, 16).load_host_stereo(empty, np.zeros(0, f32), None)
    assert D.count() == 0
    got = m.UnprojectStereo(D, _view_tuple(VIEW))
    assert got[0] == 0 and len(got[1]) == len(got[2]) == len(got[3]) == 0
    kf = osa.DeviceKeyFrame.from_frame(m, D, None)
    assert kf.count() == 0
    plain = osa.DeviceKeyFrame.from_frame(m, osa.DeviceFrame(m, 16).load(empty), None)
    assert plain.count() == 0
    kh = osa.DeviceKeyFrame.create_host_stereo(m, empty, np.zeros(0, f32), None, None)
    assert kh.count() == 0
    # the misaligned depth images the RGB-D stage refuses
    from orb_slam3_amd import _lib
    L, ex, p = _lib.lib(), rgbd["ex"], rgbd["keep"][1].data_ptr()
    assert [L.orbx_rgbd_batch_device(ex._h, C.c_void_p(p), S.PITCH + 2, S.PITCH * S.H, 40.0), L.orbx_rgbd_batch_device(ex._h, C.c_void_p(p), S.PITCH, S.PITCH * S.H + 1, 40.0),
            L.orbx_rgbd_batch_device(ex._h, C.c_void_p(p + 2), S.PITCH, S.PITCH * S.H, 40.0)] == [BAD] * 3
