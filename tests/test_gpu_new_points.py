"""LocalMapping::CreateNewMapPoints' triangulation on resident key frames: orbx_keyframe_triangulate_pairs[_fisheye] and
orbx_keyframe_search_and_triangulate[_fisheye] against tests/new_points_scene.py's float32 restatement of the member (PARITY UNPINNED: the member's
text is restated, the SVD is the oracle's restated Eigen).  status must be equal and pos equal as uint32 bits where a pair is accepted; the rows of
rejected pairs keep the caller's values.  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

import new_points_scene as S
from test_gpu_keyframe_distinctive import batch  # noqa: F401  (the module-scoped fixture: key frames whose counts are still on the device)

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD = -2             # ORBX_E_BAD_ARG
RECORD = 544         # sizeof(NewPoints): four views, two key-frame records, the arena's pointers, the parameters (orbx_matcher.hip asserts it)
SENTINEL = f32(7.25)
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))


def _pad(b):
    return (b + 255) // 256 * 256   # the arena's unit


def _pairs(m, sc, kfs, variant, n=None, idx1=None, idx2=None, pos=None):
    v1, v2 = S.call_views(sc, variant)
    par = S.call_params(sc, variant)
    i1 = sc["idx1"][:n] if idx1 is None else idx1
    i2 = sc["idx2"][:n] if idx2 is None else idx2
    fn = m.TriangulatePairsKeyFramesKB8 if sc["rig"] else m.TriangulatePairsKeyFrames
    return fn(kfs[0], kfs[1], v1, v2, par["level_sigma2_1"], par["level_sigma2_2"], par["ratio_factor"], i1, i2, par["inertial"], par["far_points"],
              par["th_far_points"], pos)


def _assert_equal(got, want, where):
    """got = (n_accepted, pos, status) of a call whose pos went in filled with SENTINEL; want = (status, pos) of the reference."""
    acc, pos, st = got
    wst, wpos = want
    assert np.array_equal(st, wst), (where, np.flatnonzero(st != wst)[:10], st[st != wst][:10], wst[st != wst][:10])
    ok = wst == S.OK
    assert acc == int(ok.sum()), (where, acc, int(ok.sum()))
    assert np.array_equal(S.bits(pos[ok]), S.bits(wpos[ok])), (where, np.flatnonzero((S.bits(pos) != S.bits(wpos)).any(axis=1) & ok)[:10])
    assert (pos[~ok] == SENTINEL).all(), where      # rejected pairs: the caller's values


@pytest.fixture(scope="module")
def ctx():
    """One context and the resident key frames of every scene, made once."""
    import orb_slam3_amd as osa
    m = osa.ORBmatcher(0.6, True)
    made = {}

    def get(seed, rig):
        if (seed, rig) not in made:
            sc = S.make_scene(seed, rig)
            made[(seed, rig)] = (sc, S.device_key_frames(osa, m, sc))
        return made[(seed, rig)]
    return m, get


# ---- (1) the pairs form ----
@pytest.mark.parametrize("rig", [False, True])
@pytest.mark.parametrize("n", S.PAIR_COUNTS)
def test_pairs_equal_the_reference(ctx, rig, n):
    m, get = ctx
    sc, kfs = get(S.SEEDS[0], rig)
    wst, wpos = S.reference(sc, "base")
    pos = np.full((n, 3), SENTINEL, f32)
    before = m.last_transfers()
    got = _pairs(m, sc, kfs, "base", n, pos=pos)
    assert got[1] is pos
    _assert_equal(got, (wst[:n], wpos[:n]), (rig, n))
    t = m.last_transfers()
    if n == 0:
        assert t == before                          # nothing enqueued
        return
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t
    kf1, kf2 = sc["key_frames"]
    assert t["upload_bytes"] == 2 * _pad(4 * n) + _pad(4 * len(kf1["scale"])) + _pad(4 * len(kf2["scale"])) + RECORD, t
    assert t["download_bytes"] == _pad(12 * n) + _pad(n) + 32, t


@pytest.mark.parametrize("rig", [False, True])
@pytest.mark.parametrize("variant", ["inertial", "far", "far_inertial", "zero", "degenerate"])
def test_every_status_under_its_parameters(ctx, rig, variant):
    """mbInertial and mbFarPoints on and off (the threshold lies inside the cloud: FAR occurs), a camera centre equal to a triangulated point
    (ZERO_DIST) and the degenerate pose whose null vector has w == 0 (TRIANGULATE_FAILED), on the second seed's scene, all designed pairs."""
    m, get = ctx
    sc, kfs = get(S.SEEDS[1], rig)
    want = S.reference(sc, variant)
    expect = {"inertial": S.LOW_PARALLAX, "far": S.FAR, "far_inertial": S.FAR, "zero": S.ZERO_DIST, "degenerate": S.TRIANGULATE_FAILED}[variant]
    assert (want[0] == expect).sum() >= 3
    pos = np.full((len(sc["idx1"]), 3), SENTINEL, f32)
    _assert_equal(_pairs(m, sc, kfs, variant, pos=pos), want, (rig, variant))


def test_the_second_seed_and_repeated_pairs(ctx):
    m, get = ctx
    for rig in (False, True):
        sc, kfs = get(S.SEEDS[1], rig)
        pos = np.full((len(sc["idx1"]), 3), SENTINEL, f32)
        _assert_equal(_pairs(m, sc, kfs, "base", pos=pos), S.reference(sc, "base"), rig)
        # the same pair named three times, and in another order: a pair's outcome is its own
        order = np.concatenate([np.arange(64)[::-1], [5, 5, 5]])
        wst, wpos = S.reference(sc, "base")
        pos = np.full((len(order), 3), SENTINEL, f32)
        _assert_equal(_pairs(m, sc, kfs, "base", idx1=sc["idx1"][order], idx2=sc["idx2"][order], pos=pos), (wst[order], wpos[order]), rig)


# ---- (2) the fused form ----
def _adhoc_scene(rig, kfs_host, views, ratio_factor):
    """A scene dict for reference_new_points from key frames made elsewhere: kfs_host = [(kps_all, n_left, n_right, u_right, scale)] * 2."""
    out = []
    for k, nl, nr, ur, sf in kfs_host:
        out.append(dict(n_left=nl, n_right=nr, x=k["x"].astype(f32), y=k["y"].astype(f32), octave=k["octave"].astype(np.int32), u_right=ur, scale=sf,
                        sigma2=(sf * sf).astype(f32)))
    base = dict(views=views, ratio_factor=f32(ratio_factor), inertial=0, far_points=0, th_far_points=0.0)
    return dict(rig=rig, key_frames=out, variants=dict(base=base, far_inertial=dict(base, inertial=1, far_points=1, th_far_points=3.0)))


def _check_fused(m, sc, call_search, call_fused, a_dev, b_dev, skips, variant, where):
    """matches12 and the count equal the search's; pos / status equal the pairs form fed with that row, and the reference."""
    n, m12 = call_search(*skips)
    t_search = m.last_transfers()
    n1 = len(m12)
    pos = np.full((max(n1, 1), 3), SENTINEL, f32)
    fn, fm12, acc, fpos, fst = call_fused(*skips, variant, pos)
    t_fused = m.last_transfers()
    assert fn == n and np.array_equal(fm12, m12), where
    idx1 = np.arange(n1, dtype=np.int32)
    want = S.reference_new_points(sc, variant, idx1, m12)
    _assert_equal((acc, fpos, fst), want, where)
    ppos = np.full((n1, 3), SENTINEL, f32)
    pacc, _, pst = _pairs(m, sc, (a_dev, b_dev), variant, idx1=idx1, idx2=m12, pos=ppos)
    assert pacc == acc and np.array_equal(pst, fst) and np.array_equal(S.bits(ppos), S.bits(fpos)), where
    n_again, m12_again = call_search(*skips)                     # the search's own counters: as before
    assert n_again == n and np.array_equal(m12_again, m12) and m.last_transfers() == t_search, where
    return n, want, t_search, t_fused


def test_fused_search_and_triangulate_pinhole(oracle):
    import orb_slam3_amd as osa
    from test_gpu_frame_bow import SF, Scene
    from test_gpu_keyframe_bow import SG, _stereo_pair
    bow = Scene(977, 600, 8, 4)
    m = osa.ORBmatcher(0.6, True)
    fx, fy, cx, cy, b = 458.654, 457.296, 367.215, 248.375, 0.11
    Kc = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    tx = np.array([[0, 0, 0], [0, 0, -b], [0, b, 0]])
    F = (np.linalg.inv(Kc).T @ tx @ np.linalg.inv(Kc)).astype(f32)
    eye = np.eye(3, dtype=f32)
    views = [[dict(R=eye, t=np.zeros(3, f32), Ow=np.zeros(3, f32), p=np.array([fx, fy, cx, cy], f32))],
             [dict(R=eye, t=np.array([-b, 0, 0], f32), Ow=np.array([b, 0, 0], f32), p=np.array([fx, fy, cx, cy], f32))]]
    seen = np.zeros(len(S.STATUS), np.int64)
    for u_right in (False, True):
        a, bq = _stereo_pair(oracle, m, bow, 2, 420, u_right)
        n = len(a.d)
        sc = _adhoc_scene(False, [(a.k, n, -1, a.ur, SF), (bq.k, n, -1, bq.ur, SF)], views, 1.5 * 1.2)
        skip1, skip2 = (bow.rng.random(n) < 0.3).astype(np.uint8), (bow.rng.random(n) < 0.3).astype(np.uint8)
        for coarse, skips, variant in ((False, (skip1, skip2), "base"), (True, (skip1, None), "far_inertial"), (False, (None, None), "base"),
                                       (True, (None, skip2), "base")):
            ep = (1e6, 1e6)

            def search(s1, s2):
                return m.SearchForTriangulationResident(a.dev, bq.dev, s1, s2, SG, F, ep, coarse, True)

            def fused(s1, s2, variant, pos):
                v1, v2 = S.call_views(sc, variant)
                par = S.call_params(sc, variant)
                return m.SearchAndTriangulateResident(a.dev, bq.dev, s1, s2, par["level_sigma2_1"], par["level_sigma2_2"], F, ep, v1, v2, par["ratio_factor"],
                                                      coarse, True, par["inertial"], par["far_points"], par["th_far_points"], pos)
            nm, want, t_s, t_f = _check_fused(m, sc, search, fused, a.dev, bq.dev, skips, variant, (u_right, coarse, variant))
            assert nm > 40
            seen += np.bincount(want[0], minlength=len(S.STATUS))
            # one launch more and nothing else: the record and kf1's level table ride up, pos / status / the flag come down beside the row
            assert t_f["uploads"] == t_s["uploads"] == 1 and t_f["downloads"] == t_s["downloads"] == 1, (t_s, t_f)
            assert t_f["xfer_launches"] == t_s["xfer_launches"] == 2 and t_f["dma_submissions"] == 0, (t_s, t_f)
            assert t_f["upload_bytes"] - t_s["upload_bytes"] == _pad(4 * len(SG)) + _pad(RECORD), (t_s, t_f)
            assert t_f["download_bytes"] - t_s["download_bytes"] == _pad(12 * n) + _pad(n) + 256, (t_s, t_f)
    assert seen[S.OK] > 100 and seen[S.NO_MATCH] > 100 and seen[S.STEREO_LEFT_TO_HOST] >= 3 and (seen[2:] > 0).sum() >= 3, seen


def _rig_views(sc_tri):
    """The four views of TriScene's two key frames: the world is key frame 1's left camera; R12[0] / t12[0] = Tll (x_cam1 = T x_cam2), R12[2] / t12[2]
    = Trl Tw2."""
    def se3(R, t):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        return T
    Tw2 = se3(sc_tri.R12[0].astype(np.float64), sc_tri.t12[0].astype(np.float64))
    Trl = se3(sc_tri.R12[2].astype(np.float64), sc_tri.t12[2].astype(np.float64)) @ np.linalg.inv(Tw2)
    T2w = np.linalg.inv(Tw2)
    out = []
    for Tl in (np.eye(4), T2w):
        side = []
        for T, prm in ((Tl, sc_tri.cams[0]), (Trl @ Tl, sc_tri.cams[1])):
            R, t = T[:3, :3], T[:3, 3]
            side.append(dict(R=R.astype(f32), t=t.astype(f32), Ow=(-R.T @ t).astype(f32), p=np.asarray(prm, f32)))
        out.append(side)
    return out


def test_fused_search_and_triangulate_rig(oracle):
    import orb_slam3_amd as osa
    from test_gpu_keyframe_bow_fisheye import SF, SG, TriScene
    tri = TriScene(703, 420)
    m = osa.ORBmatcher(0.6, True)
    a, b = tri.pair(oracle, m, 2)
    sc = _adhoc_scene(True, [(a.k, a.nl, a.n - a.nl, None, SF), (b.k, b.nl, b.n - b.nl, None, SF)], _rig_views(tri), 1.5 * 1.2)
    seen = np.zeros(len(S.STATUS), np.int64)
    for coarse, skips, variant in ((False, (tri.skip1, tri.skip2), "base"), (True, (None, None), "far_inertial"), (False, (None, tri.skip2), "base")):
        def search(s1, s2):
            return m.SearchForTriangulationResidentKB8(a.dev, b.dev, s1, s2, SG, SG, tri.cams, tri.cams, tri.R12, tri.t12, coarse)

        def fused(s1, s2, variant, pos):
            v1, v2 = S.call_views(sc, variant)
            par = S.call_params(sc, variant)
            return m.SearchAndTriangulateResidentKB8(a.dev, b.dev, s1, s2, par["level_sigma2_1"], par["level_sigma2_2"], tri.cams, tri.cams, tri.R12, tri.t12,
                                                     v1, v2, par["ratio_factor"], coarse, par["inertial"], par["far_points"], par["th_far_points"], pos)
        nm, want, t_s, t_f = _check_fused(m, sc, search, fused, a.dev, b.dev, skips, variant, (coarse, variant))
        assert nm > 28
        seen += np.bincount(want[0], minlength=len(S.STATUS))
        assert t_f["uploads"] == t_s["uploads"] == 1 and t_f["downloads"] == t_s["downloads"] == 1, (t_s, t_f)
        assert t_f["xfer_launches"] == t_s["xfer_launches"] == 2 and t_f["dma_submissions"] == 0, (t_s, t_f)
        tables = 2 * _pad(4 * len(SG)) if coarse else 0          # the gate sends both level tables itself unless it is switched off
        assert t_f["upload_bytes"] - t_s["upload_bytes"] == tables + _pad(RECORD), (t_s, t_f)
        assert t_f["download_bytes"] - t_s["download_bytes"] == _pad(12 * a.n) + _pad(a.n) + 256, (t_s, t_f)
    assert seen[S.OK] > 30 and seen[S.NO_MATCH] > 100, seen


# ---- (3) counts still on the device ----
def _batch_scene(batch):  # noqa: F811
    """The two rig key frames of the batch fixture, made from batch-loaded handles: their counts are on the device only and their right rows start at
    the handle's left capacity, not at N_left.  The images are not a calibrated pair: whatever the pairs triangulate to, the reference says."""
    exl, exr = batch["keep"][:2]
    sf = exl.GetScaleFactors().astype(f32)
    host = []
    for t in (0, 1):
        (_, kl, _), (_, kr, _) = exl.download(t), exr.download(t)
        assert (len(kl), len(kr)) == batch["host"][t][:2]
        host.append((np.concatenate([kl, kr]), len(kl), len(kr), None, sf))
    base = S.make_scene(S.SEEDS[0], True)
    sc = _adhoc_scene(True, host, base["variants"]["base"]["views"], 1.5 * 1.2)
    rng = np.random.default_rng(31)
    (n1, nl1), (n2, nl2) = [(h[1] + h[2], h[1]) for h in host]
    idx1 = np.concatenate([[nl1 - 1, nl1, n1 - 1, 0], rng.integers(0, n1, 150)]).astype(np.int32)
    idx2 = np.concatenate([[nl2, nl2 - 1, 0, n2 - 1], rng.integers(-1, n2, 150)]).astype(np.int32)
    return sc, idx1, idx2, (n1, nl1, n2, nl2)


def test_pending_counts_come_home_with_the_results(batch):  # noqa: F811
    import orb_slam3_amd as osa
    m = batch["m"]
    sc, idx1, idx2, (n1, nl1, n2, nl2) = _batch_scene(batch)
    want = S.reference_new_points(sc, "base", idx1, idx2)
    assert (want[0] == S.NO_MATCH).sum() < len(idx1) - 100
    kfs = [osa.DeviceKeyFrame.from_frame_fisheye(m, D, None) for D in batch["rig_handles"]]
    pos = np.full((len(idx1), 3), SENTINEL, f32)
    _assert_equal(_pairs(m, sc, kfs, "base", idx1=idx1, idx2=idx2, pos=pos), want, "pending")
    t_pending = m.last_transfers()
    assert t_pending["uploads"] == 1 and t_pending["downloads"] == 1 and t_pending["dma_submissions"] == 0 and t_pending["xfer_launches"] == 2, t_pending
    assert [kf.counts() for kf in kfs] == [(nl1, n1 - nl1), (nl2, n2 - nl2)]
    assert m.last_transfers() == t_pending                       # the counts were at home: nothing was fetched for them
    pos = np.full((len(idx1), 3), SENTINEL, f32)
    _assert_equal(_pairs(m, sc, kfs, "base", idx1=idx1, idx2=idx2, pos=pos), want, "known")
    assert m.last_transfers()["download_bytes"] == t_pending["download_bytes"]   # (the counts ride in the flag's 32 bytes)


def test_a_bad_index_behind_pending_counts_leaves_the_outputs_alone(batch):  # noqa: F811
    """Index N of a key frame whose count only the device knows: the kernel finds it, the call returns ORBX_E_BAD_ARG, neither pos nor status nor the
    counter is written, and the context and the key frames go on working."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    m = batch["m"]
    sc, idx1, idx2, (n1, nl1, n2, nl2) = _batch_scene(batch)
    want = S.reference_new_points(sc, "base", idx1, idx2)
    for side, N in ((0, n1), (1, n2)):
        kfs = [osa.DeviceKeyFrame.from_frame_fisheye(m, D, None) for D in batch["rig_handles"]]
        bad = [idx1.copy(), idx2.copy()]
        bad[side][17] = N
        pos = np.full((len(idx1), 3), SENTINEL, f32)
        with pytest.raises(osa.OrbxError) as e:
            _pairs(m, sc, kfs, "base", idx1=bad[0], idx2=bad[1], pos=pos)
        assert e.value.status == BAD and (pos == SENTINEL).all()
        assert [kf.count() for kf in kfs] == [n1, n2]
        pos = np.full((len(idx1), 3), SENTINEL, f32)
        _assert_equal(_pairs(m, sc, kfs, "base", idx1=idx1, idx2=idx2, pos=pos), want, side)
        before = m.last_transfers()
        with pytest.raises(osa.OrbxError) as e:                  # now the host knows N: refused before anything is enqueued
            _pairs(m, sc, kfs, "base", idx1=bad[0], idx2=bad[1], pos=pos)
        assert e.value.status == BAD and m.last_transfers() == before
    del L


def test_a_bad_octave_raises_the_flag_and_leaves_the_outputs_alone(ctx):
    """A key point whose octave is outside its key frame's pyramid forms no address: the flag comes home, the call fails, the caller's arrays keep
    their values -- in both forms' shared tail (the pairs form here; the fused form delivers through the same function)."""
    import orb_slam3_amd as osa
    m, get = ctx
    for rig in (False, True):
        sc, _ = get(S.SEEDS[0], rig)
        for side, octave in ((0, len(sc["key_frames"][0]["scale"])), (1, -1)):
            kfs_host = [dict(kf) for kf in sc["key_frames"]]
            hit = int(sc["idx1"][9] if side == 0 else sc["idx2"][9])
            assert hit >= 0
            kf = kfs_host[side]
            kp = np.concatenate([kf["kps"], kf["kps_right"]])
            kp["octave"][hit] = octave
            kf["kps"], kf["kps_right"] = kp[:kf["n_left"]].copy(), kp[kf["n_left"]:].copy()
            kfs = S.device_key_frames(osa, m, dict(sc, key_frames=kfs_host))
            pos = np.full((64, 3), SENTINEL, f32)
            with pytest.raises(osa.OrbxError) as e:
                _pairs(m, sc, kfs, "base", 64, pos=pos)
            assert e.value.status == BAD and (pos == SENTINEL).all(), (rig, side)
            pos = np.full((8, 3), SENTINEL, f32)                 # pairs that do not name the key point: fine
            wst, wpos = S.reference(sc, "base")
            _assert_equal(_pairs(m, sc, kfs, "base", 8, pos=pos), (wst[:8], wpos[:8]), (rig, side))


# ---- (4) sharing ----
def test_key_frames_shared_between_two_contexts_on_two_threads():
    import orb_slam3_amd as osa
    A = osa.ORBmatcher(0.6, True)
    scenes = [S.make_scene(S.SEEDS[0], rig) for rig in (False, True)]
    kfs = [S.device_key_frames(osa, A, sc) for sc in scenes]      # enqueued by A, handed over without a synchronisation
    wants = [S.reference(sc, "base") for sc in scenes]
    errors = []
    # (the CPU emulator runs a kernel's lanes as fibers of the calling thread and is not re-entrant: there the two threads take turns)
    turn = threading.Lock() if EMULATOR else contextlib.nullcontext()

    def worker(name, m):
        try:
            for it in range(3):
                for sc, k, want in zip(scenes, kfs, wants):
                    pos = np.full((len(sc["idx1"]), 3), SENTINEL, f32)
                    with turn:
                        got = _pairs(m, sc, k, "base", pos=pos)
                    _assert_equal(got, want, (name, it, sc["rig"]))
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    t = threading.Thread(target=worker, args=("B", osa.ORBmatcher(0.6, True)), daemon=True)
    t.start()
    worker("A", A)
    t.join(timeout=300)
    assert not t.is_alive(), "the second thread did not finish"
    assert not errors, errors


# ---- (5) refusals ----
def test_refusals_leave_the_transfer_counters_alone(ctx, oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    from orb_slam3_amd._lib import KeyFrameGate, KeyFrameKb8Gate, NewPointsParams, NewPointsView, ptr
    L = _lib.lib()
    m, get = ctx
    (mono, mk), (rig, rk) = get(S.SEEDS[0], False), get(S.SEEDS[0], True)
    _pairs(m, mono, mk, "base", 8)
    before = m.last_transfers()
    n = 8
    i1, i2 = np.ascontiguousarray(mono["idx1"][:n]), np.ascontiguousarray(mono["idx2"][:n])
    r1, r2 = np.ascontiguousarray(rig["idx1"][:n]), np.ascontiguousarray(rig["idx2"][:n])
    pos, st, acc = np.full((n, 3), SENTINEL, f32), np.full(n, 99, np.uint8), C.c_int32(-5)
    sg1, sg2 = mono["key_frames"][0]["sigma2"], mono["key_frames"][1]["sigma2"]
    sgr = rig["key_frames"][0]["sigma2"]
    par = NewPointsParams(1.8, 0, 0, 0.0, len(sg1), len(sg2), sg1.ctypes.data, sg2.ctypes.data)
    rpar = NewPointsParams(1.8, 0, 0, 0.0, len(sgr), len(sgr), sgr.ctypes.data, sgr.ctypes.data)
    v = NewPointsView()
    rv = np.zeros(46, f32)
    h = m._h

    def mono_call(kf1=mk[0]._h, kf2=mk[1]._h, v1=C.byref(v), v2=C.byref(v), p=par, n_=n, a=i1, b=i2, po=pos, s=st, mm=h):
        return L.orbx_keyframe_triangulate_pairs(mm, kf1, kf2, v1, v2, None if p is None else C.byref(p), n_, ptr(a), ptr(b), ptr(po), ptr(s), C.byref(acc))

    def rig_call(kf1=rk[0]._h, kf2=rk[1]._h, v1=ptr(rv), v2=ptr(rv), p=rpar, n_=n, a=r1, b=r2):
        return L.orbx_keyframe_triangulate_pairs_fisheye(h, kf1, kf2, v1, v2, None if p is None else C.byref(p), n_, ptr(a), ptr(b), ptr(pos), ptr(st),
                                                         C.byref(acc))
    def wrong(**kw):
        q = NewPointsParams(1.8, 0, 0, 0.0, len(sg1), len(sg2), sg1.ctypes.data, sg2.ctypes.data)
        for k, val in kw.items():
            setattr(q, k, val)
        return q
    low, high, high2 = i1.copy(), i1.copy(), i2.copy()
    low[3], high[3], high2[3] = -1, len(mono["key_frames"][0]["x"]), len(mono["key_frames"][1]["x"])
    below = i2.copy()
    below[3] = -2
    refused = [mono_call(mm=None), mono_call(kf1=None), mono_call(kf2=None), mono_call(v1=None), mono_call(v2=None), mono_call(p=None),
               mono_call(a=None), mono_call(b=None), mono_call(po=None), mono_call(s=None), mono_call(n_=-1),
               mono_call(kf1=rk[0]._h), mono_call(kf2=rk[1]._h), rig_call(kf1=mk[0]._h), rig_call(kf2=mk[1]._h),          # the other kind
               mono_call(p=wrong(nlevels_1=len(sg1) - 1)), mono_call(p=wrong(nlevels_2=len(sg2) + 1)), mono_call(p=wrong(nlevels_1=len(sg2), nlevels_2=len(sg1))),
               mono_call(p=wrong(level_sigma2_1=None)), mono_call(p=wrong(level_sigma2_2=None)), rig_call(v1=None), rig_call(p=None),
               mono_call(a=low), mono_call(a=high), mono_call(b=high2), mono_call(b=below)]
    assert refused == [BAD] * len(refused), refused
    # the fused forms: their own arguments, and whatever the search refuses (key frames without BoW here)
    g = KeyFrameGate((C.c_float * 9)(), 1e6, 1e6, 0, 1, len(sg2), sg2.ctypes.data)
    gk = KeyFrameKb8Gate(sgr.ctypes.data, sgr.ctypes.data, len(sgr), (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 36)(), (C.c_float * 12)(), 0)
    m12 = np.full(len(mono["key_frames"][0]["x"]), 77, np.int32)
    big_pos, big_st = np.full((len(m12), 3), SENTINEL, f32), np.full(len(m12), 99, np.uint8)

    def fused(kf1=mk[0]._h, kf2=mk[1]._h, gate=C.byref(g), v1=C.byref(v), p=par, mt=m12, po=big_pos, s=big_st):
        return L.orbx_keyframe_search_and_triangulate(h, kf1, kf2, None, None, 1, gate, v1, C.byref(v), None if p is None else C.byref(p), ptr(mt), ptr(po),
                                                      ptr(s), C.byref(acc))
    refused = [fused(), fused(kf1=None), fused(gate=None), fused(v1=None), fused(p=None), fused(mt=None), fused(po=None), fused(s=None),
               fused(kf1=rk[0]._h), fused(p=wrong(nlevels_1=3)),
               L.orbx_keyframe_search_and_triangulate_fisheye(h, rk[0]._h, rk[1]._h, None, None, 1, C.byref(gk), ptr(rv), ptr(rv), C.byref(rpar), ptr(m12),
                                                              ptr(big_pos), ptr(big_st), C.byref(acc)),
               L.orbx_keyframe_search_and_triangulate_fisheye(h, mk[0]._h, rk[1]._h, None, None, 1, C.byref(gk), ptr(rv), ptr(rv), C.byref(rpar), ptr(m12),
                                                              ptr(big_pos), ptr(big_st), C.byref(acc))]
    assert refused == [BAD] * len(refused), refused
    assert m.last_transfers() == before
    assert (pos == SENTINEL).all() and (st == 99).all() and acc.value == -5 and (m12 == 77).all() and (big_pos == SENTINEL).all() and (big_st == 99).all()
    assert mono_call(n_=0, a=None, b=None, po=None, s=None) == 0 and acc.value == 0 and m.last_transfers() == before   # no pairs: fine, nothing enqueued
    # key frames of another device cannot be made on a one-GPU machine; the check is the kind check's neighbour (new_points_prepare)
    want = S.reference(mono, "base")
    _assert_equal(_pairs(m, mono, mk, "base", n, pos=pos), (want[0][:n], want[1][:n]), "after the refusals")
