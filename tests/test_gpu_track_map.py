"""The Tracking thread's searches that run from map ids on a monocular / rectified resident frame: orbx_frame_track_last_frame_map
(TrackWithMotionModel's SearchByProjection(Cur, Last, th, bMono), "M2") and orbx_frame_search_by_projection_keyframe_map (Relocalization's
SearchByProjection(Cur, pKF, sAlreadyFound, th, ORBdist), "M3").  Every output -- nmatches, the match row, projected, and proj_u / proj_v bit for
bit where projected -- is compared with the reference tests/track_scene.py composes from the oracle and with the flat handle form fed with that
reference's queries, indices mapped back to source features; section 7 does the same for the two fisheye-stereo forms (`_fisheye_map`).  Runs on
the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import ctypes as C

import numpy as np
import pytest

import track_scene as TS
from test_gpu_keyframe_distinctive import batch  # noqa: F401  (two 320 x 240 stereo pairs through both extractors: frames with pending counts)

pytestmark = pytest.mark.gpu

f32 = np.float32
BAD = -2
SIZES = [1, 255, 256, 257, 600]   # the edges of k_track_project's 256-lane block
LAYOUT_ALIGN = 256


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _table(osa, m, sc, rng):
    """The scene's points at their slots, every other slot of the 2000 that no -1 entry owns filled with random points."""
    M = osa.DeviceMap(TS.CAPACITY)
    have = sc["ids"] >= 0
    mp = sc["map_points"]
    M.update(m, sc["ids"][have], **{k: np.ascontiguousarray(v[have]) for k, v in mp.items()})
    rest = np.setdiff1d(np.arange(TS.CAPACITY, dtype=np.int32), sc["slots"]).astype(np.int32)
    M.update(m, rest, pos=rng.normal(0, 5, (len(rest), 3)).astype(f32), normal=rng.normal(0, 1, (len(rest), 3)).astype(f32),
             min_dist=rng.uniform(0.1, 1, len(rest)).astype(f32), max_dist=rng.uniform(5, 50, len(rest)).astype(f32),
             desc=rng.integers(0, 256, (len(rest), 32), dtype=np.uint8))
    return M


@pytest.fixture(scope="module")
def scene(oracle):
    import orb_slam3_amd as osa
    sc = TS.make_scene(TS.SEEDS[0])
    m = osa.ORBmatcher(0.9, True)
    return dict(sc=sc, m=m, M=_table(osa, m, sc, np.random.default_rng(5)))


def _view(osa, sc, kps, desc, u_right=None):
    return osa.FrameView(kps, desc, *TS.BOUNDS, sc["scale_factors"], u_right)


def _cur(osa, m, sc, with_ur=False):
    c = sc["cur"]
    return osa.DeviceFrame(m, len(c["kps"]) + 37).load(_view(osa, sc, c["kps"], c["desc"], c["u_right"] if with_ur else None))


def _src_view(osa, sc, n):
    return _view(osa, sc, sc["src_kps"][:n], np.zeros((n, 32), np.uint8))


def _last(osa, m, sc, n):
    return osa.DeviceFrame(m, n + 5).load(_src_view(osa, sc, n))


def _kf(osa, m, sc, n):
    return osa.DeviceKeyFrame.from_host(m, _src_view(osa, sc, n))


def _mapped(cm, sel):
    return np.where(cm >= 0, sel[np.maximum(cm, 0)], cm).astype(np.int32)


def _check(got, ref, flat):
    """got = (nm, match raw, projected, (u, v)) of the new call; ref of track_scene; flat = (nm, raw match in query indices) of the flat handle form."""
    nm, match, pr, (pu, pv) = got
    assert nm == ref["nm"], (nm, ref["nm"])
    assert np.array_equal(np.maximum(match, -1), ref["match"])
    assert np.array_equal(pr, ref["projected"])
    on = ref["projected"] == 1
    assert np.array_equal(_bits(pu)[on], _bits(ref["u"])[on]) and np.array_equal(_bits(pv)[on], _bits(ref["v"])[on])
    if flat is not None:
        assert nm == flat[0] and np.array_equal(match, _mapped(flat[1], ref["sel"]))


def _m2(oracle, osa, c, n, th=7.0, level_mode=0, orientation=True, with_ur=False, has_obs="given", occupied=True, sc=None, ids=None):
    sc = c["sc"] if sc is None else sc
    m, M = c["m"], c["M"]
    ids = sc["ids"][:n] if ids is None else ids
    ho = sc["has_obs"][:n] if has_obs == "given" else None
    occ = sc["occupied"] if occupied else None
    m.mbCheckOrientation = orientation
    try:
        got = m.TrackLastFrame(_cur(osa, m, sc, with_ur), _last(osa, m, sc, n), sc["cam"], sc["pose"], M, ids, th, level_mode, ho, occ, True, True)
        ref = TS.reference_m2(oracle, sc, th, level_mode, orientation, with_ur, ids, ho, occ)
        flat = m.SearchByProjectionFrame(_cur(osa, m, sc, with_ur), ref["q"], th, level_mode, occ, raw=True) if len(ref["sel"]) else None
    finally:
        m.mbCheckOrientation = True
    _check(got, ref, flat)
    return got, ref


def _m3(oracle, osa, c, n, th=10.0, max_dist=100.0, orientation=True, with_ur=False, occupied=True, ids=None):
    sc, m, M = c["sc"], c["m"], c["M"]
    ids = sc["ids"][:n] if ids is None else ids
    occ = sc["occupied"] if occupied else None
    got = m.SearchByProjectionKeyFrame(_cur(osa, m, sc, with_ur), _kf(osa, m, sc, n), sc["cam"], sc["pose"], sc["log_scale_factor"], M, ids, th, max_dist,
                                       orientation, occ, True, True)
    ref = TS.reference_m3(oracle, sc, th, max_dist, orientation, ids, occ)
    # (the flat window form on a handle with mvuRight applies the right-coordinate gate, which Relocalization's search does not have: compared
    # with the flat form on a frame without mvuRight only)
    flat = m.SearchByProjectionWindow(_cur(osa, m, sc, False), ref["q"], max_dist, orientation, occ, raw=True) if len(ref["sel"]) and not with_ur else None
    _check(got, ref, flat)
    return got, ref


# ---- 1. both forms at the block edges ----
@pytest.mark.parametrize("n_ids", SIZES)
def test_track_last_frame_equals_reference_and_flat(oracle, scene, n_ids):
    import orb_slam3_amd as osa
    got, ref = _m2(oracle, osa, scene, n_ids)
    if n_ids == TS.N_SRC:
        assert got[0] > 100 and (got[1] == -2).any() and got[1].max() >= 256   # source feature indices, a cleared slot


@pytest.mark.parametrize("n_ids", SIZES)
def test_search_by_projection_keyframe_equals_reference_and_flat(oracle, scene, n_ids):
    import orb_slam3_amd as osa
    got, ref = _m3(oracle, osa, scene, n_ids)
    if n_ids == TS.N_SRC:
        assert got[0] > 100 and (got[1] == -2).any() and ref["stats"]["behind_kept"] >= 1


# ---- 2. the further cases ----
@pytest.mark.parametrize("with_ur", [False, True])
@pytest.mark.parametrize("orientation", [True, False])
@pytest.mark.parametrize("level_mode", [0, 1, 2])
def test_track_last_frame_level_modes_orientation_and_u_right(oracle, scene, level_mode, orientation, with_ur):
    import orb_slam3_amd as osa
    got, _ = _m2(oracle, osa, scene, TS.N_SRC, 7.0, level_mode, orientation, with_ur)
    assert got[0] > 50 and (got[1] == -2).any() == orientation


@pytest.mark.parametrize("with_ur", [False, True])
@pytest.mark.parametrize("th,max_dist", [(10.0, 100.0), (3.0, 64.0)])
def test_search_by_projection_keyframe_thresholds(oracle, scene, th, max_dist, with_ur):
    import orb_slam3_amd as osa
    got, _ = _m3(oracle, osa, scene, TS.N_SRC, th, max_dist, True, with_ur)
    assert got[0] > 50
    _m3(oracle, osa, scene, TS.N_SRC, th, max_dist, False, with_ur, occupied=False)


def test_has_obs_null_and_given(oracle, scene):
    import orb_slam3_amd as osa
    a, _ = _m2(oracle, osa, scene, TS.N_SRC, has_obs="given", orientation=False, occupied=False)
    b, _ = _m2(oracle, osa, scene, TS.N_SRC, has_obs=None, orientation=False, occupied=False)
    assert not np.array_equal(a[1], b[1])   # a point without observations leaves its feature free for a later entry


def test_a_repeated_id(oracle, scene):
    """The same id at two source features is two queries with equal data: the later one is a near-duplicate competitor."""
    import orb_slam3_amd as osa
    sc = scene["sc"]
    _, ref = _m2(oracle, osa, scene, TS.N_SRC, orientation=False, occupied=False)
    j = int(ref["match"][ref["match"] >= 0][0])           # a source feature that wins a current feature
    k = int(np.flatnonzero((sc["ids"] >= 0) & (np.arange(TS.N_SRC) > j))[3])
    ids = sc["ids"].copy()
    ids[k] = ids[j]
    twice = dict(sc, map_points={key: v.copy() for key, v in sc["map_points"].items()})
    for key in twice["map_points"]:
        twice["map_points"][key][k] = sc["map_points"][key][j]
    _m2(oracle, osa, dict(scene, sc=twice), TS.N_SRC, orientation=False, occupied=False, ids=ids)
    c3 = dict(scene, sc=twice)
    sc3, m, M = twice, scene["m"], scene["M"]
    got = m.SearchByProjectionKeyFrame(_cur(osa, m, sc3), _kf(osa, m, sc3, TS.N_SRC), sc3["cam"], sc3["pose"], sc3["log_scale_factor"], M, ids, 10.0, 100.0,
                                       True, None, True, True)
    _check(got, TS.reference_m3(oracle, sc3, 10.0, 100.0, True, ids, None), None)
    assert c3["sc"] is twice


def test_all_ids_minus_one(scene):
    import orb_slam3_amd as osa
    sc, m, M = scene["sc"], scene["m"], scene["M"]
    ids = np.full(TS.N_SRC, -1, np.int32)
    for got in (m.TrackLastFrame(_cur(osa, m, sc), _last(osa, m, sc, TS.N_SRC), sc["cam"], sc["pose"], M, ids, 7.0, 0, None, None, True, True),
                m.SearchByProjectionKeyFrame(_cur(osa, m, sc), _kf(osa, m, sc, TS.N_SRC), sc["cam"], sc["pose"], sc["log_scale_factor"], M, ids, 10.0,
                                             100.0, True, None, True, True)):
        nm, match, pr, (pu, pv) = got
        assert nm == 0 and len(match) == len(sc["cur"]["kps"]) and (match == -1).all() and not pr.any() and not pu.any() and not pv.any()
    # no source features at all
    nm, match, pr, _ = m.TrackLastFrame(_cur(osa, m, sc), osa.DeviceFrame(m, 8).load(_src_view(osa, sc, 0)), sc["cam"], sc["pose"], M, ids[:0], 7.0)
    assert nm == 0 and (match == -1).all() and len(pr) == 0


# ---- 3. counts of cur and of the source still on the device ----
@pytest.fixture(scope="module")
def pending(oracle, batch):  # noqa: F811
    """Frame 1 of the left extractor's batch as the current frame, frame 0 as the source: a scene whose points sit at the current frame's features
    and whose source rows are frame 0's."""
    import orb_slam3_amd as osa
    exl = batch["keep"][0]
    (_, k0, d0), (_, k1, d1) = exl.download(0), exl.download(1)
    sc = TS.make_scene(TS.SEEDS[1], cur=dict(kps=k1, desc=d1), src_kps=k0)
    sc["scale_factors"] = exl.GetScaleFactors().astype(f32)   # (the extractor's own: the windows of the reference and of the frames use these)
    m = osa.ORBmatcher(0.9, True)
    return dict(sc=sc, m=m, M=_table(osa, m, sc, np.random.default_rng(6)), exl=exl, n0=len(k0), n1=len(k1))


def _batch_frame(osa, p, f):
    exl = p["exl"]
    return osa.DeviceFrame(p["m"], exl.batch_view().cap + 37).load_batch(exl, f, bounds=TS.BOUNDS, scale_factors=p["sc"]["scale_factors"])


@pytest.mark.parametrize("cur_pending,src_pending", [(True, True), (True, False), (False, True)])
def test_counts_pending_on_the_device(oracle, pending, cur_pending, src_pending):
    import orb_slam3_amd as osa
    p = pending
    sc, m, M, n0 = p["sc"], p["m"], p["M"], p["n0"]
    th = 9.0
    cur = lambda: _batch_frame(osa, p, 1) if cur_pending else _cur(osa, m, sc)                                          # noqa: E731
    F = cur()
    last = _batch_frame(osa, p, 0) if src_pending else _last(osa, m, sc, n0)
    got = m.TrackLastFrame(F, last, sc["cam"], sc["pose"], M, sc["ids"], th, 0, sc["has_obs"], None, True, True)
    assert F.count() == p["n1"] and last.count() == n0
    ref = TS.reference_m2(oracle, sc, th, 0, True, False, sc["ids"], sc["has_obs"], None)
    _check(got, ref, m.SearchByProjectionFrame(cur(), ref["q"], th, 0, None, raw=True))
    assert got[0] > 30
    # the key frame made from the pending handle keeps its count on the device as well
    F = cur()
    held = _batch_frame(osa, p, 0)
    kf = osa.DeviceKeyFrame.from_frame(m, held) if src_pending else _kf(osa, m, sc, n0)
    got = m.SearchByProjectionKeyFrame(F, kf, sc["cam"], sc["pose"], sc["log_scale_factor"], M, sc["ids"], 10.0, 100.0, True, None, True, True)
    ref = TS.reference_m3(oracle, sc, 10.0, 100.0, True, sc["ids"], None)
    _check(got, ref, m.SearchByProjectionWindow(cur(), ref["q"], 100.0, True, None, raw=True))
    assert got[0] > 30 and kf.count() == n0
    if src_pending:   # a longer id row than the source has features: the entries at and beyond its count are switched off on the device
        extra = 7
        ids = np.concatenate([sc["ids"], sc["ids"][:extra][::-1]]).astype(np.int32)
        got = m.TrackLastFrame(cur(), _batch_frame(osa, p, 0), sc["cam"], sc["pose"], M, ids, th, 0, None, None, True, True)
        ref = TS.reference_m2(oracle, sc, th, 0, True, False, sc["ids"], None, None)
        assert got[0] == ref["nm"] and np.array_equal(np.maximum(got[1], -1), ref["match"]) and not got[2][n0:].any()
        assert np.array_equal(got[2][:n0], ref["projected"])


# ---- 4. ordering: an update through one context, the search through another, no host synchronisation in between ----
def test_update_then_search_through_another_context(oracle, scene):
    import orb_slam3_amd as osa
    sc = scene["sc"]
    A, B = osa.ORBmatcher(0.9, True), osa.ORBmatcher(0.9, True)
    rng = np.random.default_rng(31)
    M = _table(osa, A, sc, rng)
    have = sc["ids"] >= 0
    moved = dict(sc, map_points=dict(sc["map_points"]))
    moved["map_points"]["desc"] = np.ascontiguousarray(sc["map_points"]["desc"][rng.permutation(TS.N_SRC)])
    refs = [TS.reference_m2(oracle, s, 7.0, 0, True, False, s["ids"], None, None) for s in (sc, moved)]
    assert refs[0]["nm"] != refs[1]["nm"]
    for rnd in (1, 0, 1):
        s = (sc, moved)[rnd]
        M.update(A, s["ids"][have], desc=np.ascontiguousarray(s["map_points"]["desc"][have]))   # returns without waiting
        got = B.TrackLastFrame(_cur(osa, B, s), _last(osa, B, s, TS.N_SRC), s["cam"], s["pose"], M, s["ids"], 7.0, 0, None, None, True, True)
        _check(got, refs[rnd], None)


# ---- 5. the contract: every refusal leaves the transfer counters and the table alone ----
def _device_count():
    import torch
    try:
        return torch.cuda.device_count()
    except Exception:   # noqa: BLE001
        return 0


def test_refusals_before_anything_is_enqueued(scene, batch):  # noqa: F811
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    from orb_slam3_amd._lib import Camera, FramePose
    L = _lib.lib()
    sc = scene["sc"]
    m, other = osa.ORBmatcher(0.9, True), osa.ORBmatcher(0.9, True)
    rng = np.random.default_rng(8)
    M = _table(osa, m, sc, rng)
    n = TS.N_SRC
    cur, last, kf = _cur(osa, m, sc), _last(osa, m, sc, n), _kf(osa, m, sc, n)
    foreign_cur, foreign_last = _cur(osa, other, sc), _last(osa, other, sc, n)
    k8 = sc["src_kps"][:8]
    rig = osa.DeviceFrame(m, 8).load_fisheye(_view(osa, sc, k8[:4], np.zeros((8, 32), np.uint8)), k8[4:], np.full(4, -1, np.int32), np.full(4, -1, np.int32))
    rig_kf = osa.DeviceKeyFrame.from_host_fisheye(m, _view(osa, sc, k8[:4], np.zeros((8, 32), np.uint8)), k8[4:])
    exl = batch["keep"][0]
    pend = osa.DeviceFrame(m, exl.batch_view().cap).load_batch(exl, 0, bounds=TS.BOUNDS, scale_factors=sc["scale_factors"])
    pend_kf = osa.DeviceKeyFrame.from_frame(m, pend)
    cam, pose = Camera(*[float(x) for x in sc["cam"]]), FramePose.make(*sc["pose"])
    cm = np.zeros(len(sc["cur"]["kps"]) + 37, np.int32)
    pu = np.zeros(2 * exl.batch_view().cap, f32)
    ids = np.ascontiguousarray(sc["ids"])
    M.read(m, ids[ids >= 0][:4])
    counters = m.last_transfers()
    before = M.read(m, ids[ids >= 0])
    counters = m.last_transfers()

    def m2(mm=m, c=cur, l=last, cam_=cam, pose_=pose, map_=M, n_=n, ids_=ids, mode=0, match=cm, u=None, v=None):
        p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else (C.byref(x) if isinstance(x, C.Structure) else x._h))  # noqa: E731
        return L.orbx_frame_track_last_frame_map(p(mm), p(c), p(l), None, p(cam_), p(pose_), p(map_), n_, p(ids_), None, 7.0, mode, 1, p(match), None,
                                                 p(u), p(v))

    def m3(mm=m, c=cur, k=kf, cam_=cam, pose_=pose, map_=M, n_=n, ids_=ids, match=cm, u=None, v=None):
        p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else (C.byref(x) if isinstance(x, C.Structure) else x._h))  # noqa: E731
        return L.orbx_frame_search_by_projection_keyframe_map(p(mm), p(c), None, p(cam_), p(pose_), sc["log_scale_factor"], p(k), p(map_), n_, p(ids_),
                                                              10.0, 100.0, 1, p(match), None, p(u), p(v))

    def with_id(j, value):
        a = ids.copy()
        a[j] = value
        return a

    first = int(np.flatnonzero(ids >= 0)[0])
    dead = int(sc["slots"][np.flatnonzero(sc["ids"] < 0)[0]])   # a slot nobody has written
    refusals = []
    for f in (m2, m3):
        refusals += [f(mm=None), f(c=None), f(cam_=None), f(pose_=None), f(map_=None), f(ids_=None), f(match=None), f(n_=-1)]   # NULL arguments
        refusals += [f(c=foreign_cur), f(mm=other)]                                                                             # the owner of cur
        refusals += [f(c=rig)]                                                                                                  # the kind of cur
        refusals += [f(u=pu), f(v=pu)]                                                                                          # proj_u without proj_v
        refusals += [f(ids_=with_id(first, -2)), f(ids_=with_id(first, TS.CAPACITY)), f(ids_=with_id(5, 2 ** 31 - 1)), f(ids_=with_id(first, dead))]
        refusals += [f(n_=n - 1), f(n_=n + 1, ids_=np.concatenate([ids, ids[:1]]))]                                             # not the source's count
    refusals += [m2(l=None), m2(l=foreign_last), m2(l=rig), m2(l=cur), m2(mode=3), m2(mode=-1)]
    refusals += [m3(k=None), m3(k=rig_kf)]
    big = np.full(exl.batch_view().cap + 1, -1, np.int32)   # above the capacity of a source whose count is pending
    refusals += [m2(l=pend, n_=len(big), ids_=big), m3(k=pend_kf, n_=len(big), ids_=big)]
    assert refusals and all(r == BAD for r in refusals), refusals
    assert m.last_transfers() == counters
    after = M.read(m, ids[ids >= 0])
    assert all(np.array_equal(before[k], after[k]) for k in before)
    if _device_count() >= 2:
        far = osa.DeviceMap(16, device=1)
        assert m2(map_=far, ids_=np.full(n, -1, np.int32)) == BAD and m3(map_=far, ids_=np.full(n, -1, np.int32)) == BAD
    # and the same handles go on working
    assert m2() >= 0 and m3() >= 0


# ---- 6. transfers ----
def test_transfers(oracle, scene):
    """One upload run, one download run, no DMA submission; the upload is smaller than the flat form's on the same scene; growing n_ids from 256 to
    512 grows it by at most 8 x 256 bytes -- an id, a flag byte and alignment, no per-entry descriptor or query record.  (The counters hold no
    synchronisation count: every call ends in its one sync_and_deliver.)"""
    import orb_slam3_amd as osa
    sc, m, M = scene["sc"], scene["m"], scene["M"]
    up = {}
    for n in (256, 512, TS.N_SRC):
        ids, ho = sc["ids"][:n], sc["has_obs"][:n]
        m.TrackLastFrame(_cur(osa, m, sc), _last(osa, m, sc, n), sc["cam"], sc["pose"], M, ids, 7.0, 0, ho, sc["occupied"], True, True)
        t2 = m.last_transfers()
        m.SearchByProjectionKeyFrame(_cur(osa, m, sc), _kf(osa, m, sc, n), sc["cam"], sc["pose"], sc["log_scale_factor"], M, ids, 10.0, 100.0, True,
                                     sc["occupied"], True, True)
        t3 = m.last_transfers()
        for t in (t2, t3):
            assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0, t
        up[n] = (t2, t3)
    for k in (0, 1):
        assert 0 < up[512][k]["upload_bytes"] - up[256][k]["upload_bytes"] <= 8 * 256, up
    n = TS.N_SRC
    r2 = TS.reference_m2(oracle, sc, 7.0, 0, True, False, sc["ids"], sc["has_obs"], sc["occupied"])
    m.SearchByProjectionFrame(_cur(osa, m, sc), r2["q"], 7.0, 0, sc["occupied"], raw=True)
    f2 = m.last_transfers()
    r3 = TS.reference_m3(oracle, sc, 10.0, 100.0, True, sc["ids"], sc["occupied"])
    m.SearchByProjectionWindow(_cur(osa, m, sc), r3["q"], 100.0, True, sc["occupied"], raw=True)
    f3 = m.last_transfers()
    for k, flat in ((0, f2), (1, f3)):
        t = up[n][k]
        assert t["upload_bytes"] < flat["upload_bytes"], (t, flat)
        assert t["uploads"] == flat["uploads"] and t["downloads"] == flat["downloads"] and t["xfer_launches"] == flat["xfer_launches"], (t, flat)


# ---- 7. the fisheye-stereo rig: both forms against the rig reference and the flat rig forms ----
@pytest.fixture(scope="module")
def rig(oracle):
    import orb_slam3_amd as osa
    sc = TS.make_rig_scene(oracle, TS.RIG_SEEDS[0])
    m = osa.ORBmatcher(0.9, True)
    return dict(sc=sc, m=m, M=_table(osa, m, sc, np.random.default_rng(7)))


def _rig_view(osa, sc, kps, desc):
    return osa.FrameView(kps, desc, *TS.RIG_BOUNDS, sc["scale_factors"])


def _rig_cur(osa, m, sc):
    c = sc["cur"]
    return osa.DeviceFrame(m, len(c["desc"]) + 11).load_fisheye(_rig_view(osa, sc, c["kps_left"], c["desc"]), c["kps_right"], c["l2r"], c["r2l"])


def _rig_src(sc, n):
    """The source truncated to n features: its first min(n, N_left) rows are the left camera's."""
    nl = min(n, sc["n_left_src"])
    return sc["src_kps"][:nl], sc["src_kps"][nl:n], dict(sc, n_left_src=nl)


def _rig_last(osa, m, sc, n):
    kl, kr, _ = _rig_src(sc, n)
    return osa.DeviceFrame(m, n + 5).load_fisheye(_rig_view(osa, sc, kl, np.zeros((n, 32), np.uint8)), kr, np.full(len(kl), -1, np.int32),
                                                  np.full(len(kr), -1, np.int32))


def _rig_kf(osa, m, sc, n):
    kl, kr, _ = _rig_src(sc, n)
    return osa.DeviceKeyFrame.from_host_fisheye(m, _rig_view(osa, sc, kl, np.zeros((n, 32), np.uint8)), kr)


def _rig_m2(oracle, osa, c, n, th=7.0, level_mode=0, orientation=True, has_obs=True, occupied=True):
    sc, m, M = c["sc"], c["m"], c["M"]
    ids = sc["ids"][:n]
    ho = sc["has_obs"][:n] if has_obs else None
    occ = sc["occupied"] if occupied else None
    m.mbCheckOrientation = orientation
    try:
        got = m.TrackLastFrameFisheye(_rig_cur(osa, m, sc), _rig_last(osa, m, sc, n), sc["view"], sc["Trl"], M, ids, th, level_mode, ho, occ, True, True)
        ref = TS.rig_reference_m2(oracle, _rig_src(sc, n)[2], th, level_mode, orientation, ids, ho, occ)
        flat = m.SearchByProjectionFrameFisheye(_rig_cur(osa, m, sc), None, ref["q"], th, level_mode, occ, raw=True) if len(ref["sel"]) else None
    finally:
        m.mbCheckOrientation = True
    _check(got, ref, flat)
    return got, ref


def _rig_m3(oracle, osa, c, n, th=10.0, max_dist=100.0, orientation=True, occupied=True):
    sc, m, M = c["sc"], c["m"], c["M"]
    ids = sc["ids"][:n]
    occ = sc["occupied"] if occupied else None
    got = m.SearchByProjectionKeyFrameFisheye(_rig_cur(osa, m, sc), _rig_kf(osa, m, sc, n), sc["view"], sc["log_scale_factor"], M, ids, th, max_dist,
                                              orientation, occ, True, True)
    ref = TS.rig_reference_m3(oracle, _rig_src(sc, n)[2], th, max_dist, orientation, ids, occ)
    flat = m.SearchByProjectionWindowFisheye(_rig_cur(osa, m, sc), ref["q"], max_dist, orientation, occ, raw=True) if len(ref["sel"]) else None
    _check(got, ref, flat)
    return got, ref


@pytest.mark.parametrize("n_ids", SIZES)
def test_rig_track_last_frame_equals_reference_and_flat(oracle, rig, n_ids):
    import orb_slam3_amd as osa
    got, ref = _rig_m2(oracle, osa, rig, n_ids)
    if n_ids == TS.N_SRC:
        nl = len(rig["sc"]["cur"]["kps_left"])
        assert got[0] > 100 and (got[1] == -2).any() and (got[1][nl:] >= 0).sum() > 20 and (got[1] >= rig["sc"]["n_left_src"]).sum() > 20


@pytest.mark.parametrize("n_ids", SIZES)
def test_rig_search_by_projection_keyframe_equals_reference_and_flat(oracle, rig, n_ids):
    import orb_slam3_amd as osa
    got, ref = _rig_m3(oracle, osa, rig, n_ids)
    if n_ids == TS.N_SRC:
        nl = len(rig["sc"]["cur"]["kps_left"])
        assert got[0] > 100 and (got[1][nl:] == -1).all() and ref["stats"]["behind_kept"] >= 1


@pytest.mark.parametrize("orientation", [True, False])
@pytest.mark.parametrize("level_mode", [0, 1, 2])
def test_rig_track_last_frame_level_modes_and_orientation(oracle, rig, level_mode, orientation):
    import orb_slam3_amd as osa
    got, _ = _rig_m2(oracle, osa, rig, TS.N_SRC, 7.0, level_mode, orientation, has_obs=level_mode != 1, occupied=level_mode != 2)
    assert got[0] > 50 and (got[1] == -2).any() == orientation


@pytest.mark.parametrize("th,max_dist", [(10.0, 100.0), (3.0, 64.0)])
def test_rig_search_by_projection_keyframe_thresholds(oracle, rig, th, max_dist):
    import orb_slam3_amd as osa
    assert _rig_m3(oracle, osa, rig, TS.N_SRC, th, max_dist, True)[0][0] > 30
    _rig_m3(oracle, osa, rig, TS.N_SRC, th, max_dist, False, occupied=False)


def test_rig_counts_pending_on_the_device(oracle, rig, batch):  # noqa: F811
    """The batch's rig frame 0 (counts pending) as the current frame and, loaded a second time, as the source; then a key frame made from it."""
    import orb_slam3_amd as osa
    sc, m, M = rig["sc"], rig["m"], rig["M"]
    exl, exr = batch["keep"][:2]
    (_, bkl, bdl), (_, bkr, bdr) = exl.download(0), exr.download(0)
    sf = exl.GetScaleFactors().astype(f32)
    n = len(bkl) + len(bkr)
    assert n >= TS.N_SRC or n > 100
    n = min(n, TS.N_SRC)

    def handle(f):
        return osa.DeviceFrame(m, exl.batch_view().cap + exr.batch_view().cap).load_stereo_fisheye_batch(exl, exr, f, bounds=TS.RIG_BOUNDS, scale_factors=sf)

    (_, skl, _), (_, skr, _) = exl.download(1), exr.download(1)
    src = np.concatenate([skl, skr])
    ns = min(len(src), TS.N_SRC)
    scp = dict(sc, scale_factors=sf, src_kps=np.ascontiguousarray(src[:len(src)]), n_left_src=len(skl),
               cur=dict(kps_left=bkl, kps_right=bkr, desc=np.concatenate([bdl, bdr]).reshape(-1, 32), l2r=None, r2l=None))
    ids = np.full(len(src), -1, np.int32)
    ids[:ns] = sc["ids"][:ns]
    F, last = handle(0), handle(1)
    got = m.TrackLastFrameFisheye(F, last, sc["view"], sc["Trl"], M, ids, 40.0, 0, None, None, True, True)
    assert F.counts() == (len(bkl), len(bkr)) and last.counts() == (len(skl), len(skr))
    ref = TS.rig_reference_m2(oracle, dict(scp, map_points={k: np.concatenate([v[:ns], v[:len(src) - ns]]) for k, v in sc["map_points"].items()}), 40.0, 0,
                              True, ids, None, None)
    _check(got, ref, None)
    held = handle(1)
    kf = osa.DeviceKeyFrame.from_frame_fisheye(m, held)
    got = m.SearchByProjectionKeyFrameFisheye(handle(0), kf, sc["view"], sc["log_scale_factor"], M, ids, 40.0, 100.0, True, None, True, True)
    ref = TS.rig_reference_m3(oracle, dict(scp, map_points={k: np.concatenate([v[:ns], v[:len(src) - ns]]) for k, v in sc["map_points"].items()}), 40.0,
                              100.0, True, ids, None)
    _check(got, ref, None)


def test_rig_refusals_and_transfers(oracle, rig, scene):
    import orb_slam3_amd as osa
    sc, m, M = rig["sc"], rig["m"], rig["M"]
    n = TS.N_SRC
    mono = scene["sc"]
    mono_cur, mono_last, mono_kf = _cur(osa, m, mono), _last(osa, m, mono, n), _kf(osa, m, mono, n)
    cur, last, kf = _rig_cur(osa, m, sc), _rig_last(osa, m, sc, n), _rig_kf(osa, m, sc, n)
    m.TrackLastFrameFisheye(cur, last, sc["view"], sc["Trl"], M, sc["ids"], 7.0, 0, sc["has_obs"], sc["occupied"], True, True)
    t2 = m.last_transfers()
    m.SearchByProjectionKeyFrameFisheye(cur, kf, sc["view"], sc["log_scale_factor"], M, sc["ids"], 10.0, 100.0, True, sc["occupied"], True, True)
    t3 = m.last_transfers()
    for t in (t2, t3):
        assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0, t
    r2 = TS.rig_reference_m2(oracle, sc, 7.0, 0, True, sc["ids"], sc["has_obs"], sc["occupied"])
    m.SearchByProjectionFrameFisheye(cur, None, r2["q"], 7.0, 0, sc["occupied"], raw=True)
    assert t2["upload_bytes"] < m.last_transfers()["upload_bytes"]
    r3 = TS.rig_reference_m3(oracle, sc, 10.0, 100.0, True, sc["ids"], sc["occupied"])
    m.SearchByProjectionWindowFisheye(cur, r3["q"], 100.0, True, sc["occupied"], raw=True)
    assert t3["upload_bytes"] < m.last_transfers()["upload_bytes"]
    counters = m.last_transfers()
    bad_id = sc["ids"].copy()
    bad_id[int(np.flatnonzero(bad_id >= 0)[0])] = TS.CAPACITY
    for call in (lambda: m.TrackLastFrameFisheye(mono_cur, last, sc["view"], sc["Trl"], M, sc["ids"], 7.0),                       # the kind of cur
                 lambda: m.TrackLastFrameFisheye(cur, mono_last, sc["view"], sc["Trl"], M, sc["ids"], 7.0),                       # the kind of last
                 lambda: m.TrackLastFrameFisheye(cur, cur, sc["view"], sc["Trl"], M, sc["ids"], 7.0),                             # cur == last
                 lambda: m.TrackLastFrameFisheye(cur, last, sc["view"], sc["Trl"], M, bad_id, 7.0),
                 lambda: m.TrackLastFrameFisheye(cur, last, sc["view"], sc["Trl"], M, sc["ids"][:-1], 7.0),                      # not the source's count
                 lambda: m.TrackLastFrame(cur, last, mono["cam"], mono["pose"], M, sc["ids"], 7.0),                              # a rig to the mono form
                 lambda: m.SearchByProjectionKeyFrameFisheye(mono_cur, kf, sc["view"], 0.18, M, sc["ids"], 10.0, 100.0),
                 lambda: m.SearchByProjectionKeyFrameFisheye(cur, mono_kf, sc["view"], 0.18, M, sc["ids"], 10.0, 100.0),
                 lambda: m.SearchByProjectionKeyFrameFisheye(cur, kf, sc["view"], 0.18, M, bad_id, 10.0, 100.0),
                 lambda: m.SearchByProjectionKeyFrame(cur, kf, mono["cam"], mono["pose"], 0.18, M, sc["ids"], 10.0, 100.0)):
        with pytest.raises(osa.OrbxError) as e:
            call()
        assert e.value.status == BAD
    assert m.last_transfers() == counters
