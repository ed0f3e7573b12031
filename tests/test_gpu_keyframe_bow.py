"""BoW on device-resident key frames: KeyFrame::ComputeBoW (orbx_keyframe_compute_bow), the FeatureVector copied from the frame handle
(orbx_keyframe_bow_from_frame) and the three BoW-guided matchers with both sides resident (orbx_frame_search_by_bow_resident,
orbx_keyframe_search_by_bow, orbx_keyframe_search_for_triangulation).

Expectations come from the CPU oracle (bow_transform, search_by_bow_frame, search_by_bow_keyframes, search_for_triangulation_pinhole) on the host
arrays, with the FeatureVectors built here from the oracle's transform (stopped words dropped); every resident result is also compared with the
host-pointer entry point for the same arrays.  Every comparison is equality of integers."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from test_gpu_frame_bow import H, SF, W, Scene, _keypoints, _noisy

pytestmark = pytest.mark.gpu

f32 = np.float32
BAD, TOO_LARGE, STALE = -2, -7, -9
TH_LOW = 50
SG = (SF * SF).astype(f32)            # mvLevelSigma2
ISG = (f32(1.0) / SG).astype(f32)     # mvInvLevelSigma2
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))


class KF:
    """A key frame on the host (what the host-pointer entry points and the oracle take) and the same key frame resident with BoW."""

    def __init__(self, oracle, m, sc, levelsup, kps, desc, valid=None, u_right=None, bow=True):
        import orb_slam3_amd as osa
        self.k, self.d, self.valid, self.ur = kps, np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), valid, u_right
        self.ang = np.ascontiguousarray(kps["angle"], f32)
        self.fv = sc.featvec(oracle, self.d, levelsup)
        self.view = osa.FrameView(self.k, self.d, 0.0, float(W), 0.0, float(H), SF, u_right)
        self.dev = osa.DeviceKeyFrame.from_host(m, self.view, ISG)
        if bow:
            self.dev.compute_bow(m, sc.voc, levelsup, download=False)

    @property
    def v1(self):
        return np.ones(len(self.d), np.uint8) if self.valid is None else self.valid


def _kf(oracle, m, sc, levelsup, related=True, n=None, valid_p=0.8, valid="random", **kw):
    d, ang, v, _ = sc.keyframe(oracle, levelsup, related=related, n=n, valid_p=valid_p)
    k = _keypoints(sc.rng, len(d))
    k["angle"] = ang
    v = {"random": v, "none": None, "zero": np.zeros(len(d), np.uint8)}[valid]
    return KF(oracle, m, sc, levelsup, k, d, v, **kw)


def _stop_all(sc):
    """The scene's vocabulary with weights that stop every word."""
    import orb_slam3_amd as osa
    sc.weights = np.zeros_like(sc.weights)
    sc.voc = osa.ORBVocabulary(sc.L, sc.cp, sc.ci, sc.nd, sc.wi).set_word_weights(sc.weights)
    return sc


# ---- ComputeBoW ----
@pytest.mark.parametrize("n", [0, 1, 257, 900])
@pytest.mark.parametrize("levelsup", [0, 2, 4])   # 4 = L: one node holds every feature (the big-node path of the replay)
def test_compute_bow_ids_equal_the_oracle(oracle, n, levelsup):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    sc = Scene(600 + 10 * levelsup + n % 7, max(n, 300), 8, 4)
    m = osa.ORBmatcher(0.75, True)
    d = sc.d[:n]
    k = sc.k[:n]
    kf = osa.DeviceKeyFrame.from_host(m, osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), SF), ISG)
    w, node = kf.compute_bow(m, sc.voc, levelsup)
    ow, onode = sc.transform(oracle, d, levelsup)
    assert len(w) == n and np.array_equal(w, ow) and np.array_equal(node, onode)
    if n >= 257:
        assert (sc.weights[w] <= 0).any() and (sc.weights[w] > 0).sum() > n // 2      # some features are stopped, most are not
        if levelsup == 4:
            assert len(np.unique(node)) == 1
    w2, node2 = kf.compute_bow(m, sc.voc, levelsup)                                    # not computed again: the ids that were kept
    assert np.array_equal(w2, w) and np.array_equal(node2, node)
    L = _lib.lib()
    assert L.orbx_keyframe_compute_bow(m._h, kf._h, sc.voc._h, levelsup + 1, None, None) == BAD      # another levelsup
    other = Scene(5, 10).voc
    assert L.orbx_keyframe_compute_bow(m._h, kf._h, other._h, levelsup, None, None) == BAD           # another vocabulary
    assert L.orbx_keyframe_compute_bow(m._h, kf._h, sc.voc._h, levelsup, None, None) == 0


# ---- frame against resident key frames ----
def _frame_rows(oracle, m, sc, D, fv_f, kfs, ratio, ori):
    m.mfNNratio, m.mbCheckOrientation = ratio, ori
    nm, match = m.SearchByBoWResident(D, [q.dev for q in kfs], [q.valid for q in kfs])
    t = m.last_transfers()
    assert nm.shape == (len(kfs),) and match.shape == (len(kfs), len(sc.d))
    hn, hmatch = m.SearchByBoWDevice(D, [(q.d, q.ang, q.valid, q.fv) for q in kfs])     # today's call with the key frames as host arrays
    assert np.array_equal(nm, hn) and np.array_equal(match, hmatch)
    for k, q in enumerate(kfs):
        on, om = oracle.search_by_bow_frame(q.d, q.ang, q.v1, q.fv, sc.d, sc.k["angle"], fv_f, ratio, ori)
        assert nm[k] == on and np.array_equal(match[k], om), (k, ratio, ori, nm[k], on)
        n1, fm1 = m.SearchByBoWFrame(q.d, q.ang, q.v1, q.fv, sc.d, sc.k["angle"], fv_f)
        assert n1 == on and np.array_equal(fm1, om)
    return nm, t


def _mixed_keyframes(oracle, m, sc, levelsup, K):
    """K key frames of different sizes: related ones, and from K = 7 on one empty, one unrelated, one whose flags are all zero, one without flags."""
    kfs = [_kf(oracle, m, sc, levelsup, n=int(sc.rng.integers(80, 420))) for _ in range(K)]
    if K >= 7:
        kfs[1] = _kf(oracle, m, sc, levelsup, n=0)
        kfs[2] = _kf(oracle, m, sc, levelsup, related=False)
        kfs[4] = _kf(oracle, m, sc, levelsup, valid="zero")
        kfs[5] = _kf(oracle, m, sc, levelsup, valid="none")
    return kfs


@pytest.mark.parametrize("K", [1, 7, 9])
def test_frame_against_resident_key_frames(oracle, K):
    import orb_slam3_amd as osa
    sc = Scene(700 + K, 900, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 1000).load(sc.F)
    for levelsup in (2, 4):
        D.compute_bow(sc.voc, levelsup, download=False)
        fv_f = sc.featvec(oracle, sc.d, levelsup)
        kfs = _mixed_keyframes(oracle, m, sc, levelsup, K)
        for ratio, ori in ((0.7, True), (0.75, True), (0.9, True), (0.75, False)):
            nm, _ = _frame_rows(oracle, m, sc, D, fv_f, kfs, ratio, ori)
            good = [k for k in range(K) if not (K >= 7 and k in (1, 2, 4))]
            assert min(nm[good]) > 10, nm
            if K >= 7:
                assert nm[1] == nm[4] == 0
    nm, match = m.SearchByBoWResident(D, [])
    assert nm.shape == (0,) and match.shape == (0, 900)


def test_featurevector_without_nodes(oracle):
    import orb_slam3_amd as osa
    sc = Scene(720, 300, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 300).load(sc.F)
    D.compute_bow(sc.voc, 2, download=False)
    live = _kf(oracle, m, sc, 2)
    frame_voc = sc.voc
    _stop_all(sc)
    dead = _kf(oracle, m, sc, 2)                     # every word stopped: a FeatureVector with no nodes
    assert len(dead.fv.node_id) == 0
    other = _kf(oracle, m, sc, 2)
    nm, m12 = m.SearchByBoWKeyFramesResident(dead.dev, [other.dev, dead.dev])
    assert list(nm) == [0, 0] and (m12 == -1).all()
    with pytest.raises(osa.OrbxError):               # a key frame of another vocabulary than the frame's
        m.SearchByBoWResident(D, [live.dev, dead.dev])
    assert m.SearchByBoWResident(D, [live.dev])[0][0] > 10 and frame_voc is not sc.voc


# ---- bow_from_frame ----
def test_bow_from_frame_equals_compute_bow_and_goes_stale(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    sc = Scene(730, 600, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    cur = osa.DeviceFrame(m, 700).load(sc.F)
    cur.compute_bow(sc.voc, 2, download=False)
    fv_f = sc.featvec(oracle, sc.d, 2)
    want = [_kf(oracle, m, sc, 2, n=n) for n in (310, 0, 150)]
    D = osa.DeviceFrame(m, 500)
    got = []
    for q in want:
        D.load(q.view)
        kf = osa.DeviceKeyFrame.from_frame(m, D, ISG)
        assert L.orbx_keyframe_bow_from_frame(m._h, kf._h, D._h) == BAD            # no compute_bow since the load
        D.compute_bow(sc.voc, 2, download=False)
        assert L.orbx_keyframe_bow_from_frame(m._h, kf._h, cur._h) == BAD          # not the handle the key frame was made from
        kf.bow_from_frame(m, D)
        assert L.orbx_keyframe_bow_from_frame(m._h, kf._h, D._h) == BAD            # set once
        got.append(kf)
    late = osa.DeviceKeyFrame.from_frame(m, D, ISG)
    D.load(want[0].view)                                                           # reloaded: the handle holds another frame
    D.compute_bow(sc.voc, 2, download=False)
    assert L.orbx_keyframe_bow_from_frame(m._h, late._h, D._h) == STALE
    valid = [q.valid for q in want]
    for ori in (True, False):
        m.mbCheckOrientation = ori
        n1, r1 = m.SearchByBoWResident(cur, got, valid)
        n2, r2 = m.SearchByBoWResident(cur, [q.dev for q in want], valid)
        assert np.array_equal(n1, n2) and np.array_equal(r1, r2)
        for k, q in enumerate(want):
            on, om = oracle.search_by_bow_frame(q.d, q.ang, q.v1, q.fv, sc.d, sc.k["angle"], fv_f, 0.75, ori)
            assert n1[k] == on and np.array_equal(r1[k], om)
        assert n1[0] > 10 and n1[2] > 10
        n3, r3 = m.SearchByBoWKeyFramesResident(got[0], got, valid[0], valid)
        n4, r4 = m.SearchByBoWKeyFramesResident(want[0].dev, [q.dev for q in want], valid[0], valid)
        assert np.array_equal(n3, n4) and np.array_equal(r3, r4) and n3[0] > 50


def test_bow_from_a_batch_loaded_handle_with_its_count_on_the_device(oracle, canvas1):
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from test_gpu_matcher import _random_vocabulary
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    m = osa.ORBmatcher(0.75, True)
    frames = torch.from_numpy(np.stack([synth.frame_from_canvas(canvas1, t, W, H, 1000 + t) for t in range(3)])).cuda()
    ex.extract_batch_device(frames.data_ptr(), 3, W, H, W, W * H, (0, 1000))
    outs = [ex.download(t) for t in range(3)]
    rng = np.random.default_rng(5)
    cp, ci, nd, wi = _random_vocabulary(rng, 10, 4)
    pool = np.concatenate([o[2] for o in outs])
    nd = _noisy(rng, pool[rng.integers(0, len(pool), len(nd))], 0.03)
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.05] = 0.0
    voc = osa.ORBVocabulary(4, cp, ci, nd, wi).set_word_weights(weights)

    def fv(desc):
        w, node = oracle.bow_transform(cp, ci, nd, wi, 4, 2, desc)
        kept = np.nonzero(weights[w] > 0)[0]
        nodes = np.unique(node[kept])
        return osa.FeatureVector(nodes, [kept[node[kept] == x] for x in nodes])

    sf = ex.GetScaleFactors()
    isg = (f32(1.0) / (sf * sf)).astype(f32)
    cap = ex.batch_view().cap
    D = osa.DeviceFrame(m, cap)
    kfs = []
    for t in (0, 1):                                                    # N of neither frame ever reaches the host before the search
        D.load_batch(ex, t)
        D.compute_bow(voc, 2, download=False)
        kfs.append(osa.DeviceKeyFrame.from_frame(m, D, isg).bow_from_frame(m, D))
    own = osa.DeviceKeyFrame.from_frame(m, D, isg)                      # the same frame, BoW computed on the key frame itself, capacity > N
    w, node = own.compute_bow(m, voc, 2, cap=cap)
    assert cap > len(outs[1][1]) and np.array_equal(node, oracle.bow_transform(cp, ci, nd, wi, 4, 2, outs[1][2])[1])
    D.load_batch(ex, 2)
    D.compute_bow(voc, 2, download=False)
    nm, match = m.SearchByBoWResident(D, kfs + [own])
    _, kc, dc = outs[2]
    assert match.shape == (3, len(kc)) and [q.count() for q in kfs] == [len(outs[0][1]), len(outs[1][1])]
    fv_c = fv(dc)
    for k, t in enumerate((0, 1, 1)):
        _, kk, dk = outs[t]
        on, om = oracle.search_by_bow_frame(dk, kk["angle"], np.ones(len(dk), np.uint8), fv(dk), dc, kc["angle"], fv_c, 0.75, True)
        assert nm[k] == on and np.array_equal(match[k], om), (k, nm[k], on)
        assert on > 50
    n2, m12 = m.SearchByBoWKeyFramesResident(kfs[0], [kfs[1], own])
    on, om = oracle.search_by_bow_keyframes(outs[0][2], outs[0][1]["angle"], np.ones(len(outs[0][2]), np.uint8), fv(outs[0][2]), outs[1][2],
                                            outs[1][1]["angle"], np.ones(len(outs[1][2]), np.uint8), fv(outs[1][2]), 0.75, True)
    assert list(n2) == [on, on] and np.array_equal(m12[0], om) and np.array_equal(m12[1], om) and on > 50


# ---- key frame against key frames ----
@pytest.mark.parametrize("K", [1, 7, 9])
def test_keyframe_against_key_frames(oracle, K):
    import orb_slam3_amd as osa
    sc = Scene(800 + K, 700, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    for levelsup in (2, 4):
        kf1 = _kf(oracle, m, sc, levelsup, n=500)
        kfs = _mixed_keyframes(oracle, m, sc, levelsup, K)
        kfs[0] = kf1                                      # kf1 among kfs2
        if K >= 7:
            kfs[6] = kfs[3]                               # the same key frame twice in one call: scratch is per problem
        for ratio, ori in ((0.75, True), (0.7, False), (0.9, True)):
            m.mfNNratio, m.mbCheckOrientation = ratio, ori
            nm, m12 = m.SearchByBoWKeyFramesResident(kf1.dev, [q.dev for q in kfs], kf1.valid, [q.valid for q in kfs])
            assert m12.shape == (K, 500)
            for k, q in enumerate(kfs):
                on, om = oracle.search_by_bow_keyframes(kf1.d, kf1.ang, kf1.v1, kf1.fv, q.d, q.ang, q.v1, q.fv, ratio, ori)
                assert nm[k] == on and np.array_equal(m12[k], om), (k, ratio, ori, nm[k], on)
                hn, hm = m.SearchByBoWKeyFrames(kf1.d, kf1.ang, kf1.v1, kf1.fv, q.d, q.ang, q.v1, q.fv)
                assert hn == on and np.array_equal(hm, om)
            assert nm[0] > 100                            # a key frame against itself
            if K >= 7:
                assert nm[6] == nm[3] and np.array_equal(m12[6], m12[3]) and nm[3] > 10 and nm[1] == nm[4] == 0


def test_a_pair_at_exactly_th_low_is_refused(oracle):
    """ORBmatcher.cc:848: `if (bestDist1 < TH_LOW)` -- strict, unlike SearchByBoW(KeyFrame*, Frame&)'s `<=` (:318)."""
    import orb_slam3_amd as osa
    sc = Scene(850, 300, 8, 4, stop=0.0)              # no stop words: the single features below always enter their FeatureVector
    m = osa.ORBmatcher(0.9, False)
    D = osa.DeviceFrame(m, 8)
    k = _keypoints(sc.rng, 1)
    a = KF(oracle, m, sc, 4, k, sc.d[:1])                # levelsup = L: every feature in node 0, so the pair shares its node
    assert len(a.fv.node_id) == 1
    seen = {}
    for dist in (TH_LOW - 1, TH_LOW, TH_LOW + 1):
        bits = np.zeros(256, bool)
        bits[sc.rng.choice(256, dist, replace=False)] = True
        d2 = a.d ^ np.packbits(bits, bitorder="little")[None, :]
        b = KF(oracle, m, sc, 4, k, d2)
        assert len(b.fv.node_id) == 1
        nm, m12 = m.SearchByBoWKeyFramesResident(a.dev, [b.dev])
        on, om = oracle.search_by_bow_keyframes(a.d, a.ang, a.v1, a.fv, b.d, b.ang, b.v1, b.fv, 0.9, False)
        assert nm[0] == on and np.array_equal(m12[0], om)
        D.load(b.view)
        D.compute_bow(sc.voc, 4, download=False)
        fn, _ = m.SearchByBoWResident(D, [a.dev])
        seen[dist] = (int(nm[0]), int(fn[0]))
    assert seen == {TH_LOW - 1: (1, 1), TH_LOW: (0, 1), TH_LOW + 1: (0, 0)}, seen


# ---- triangulation ----
def _stereo_pair(oracle, m, sc, levelsup, n, u_right):
    """Two key frames seeing the same features from cameras a pure x-translation apart: epipolar lines are the rows, kf2's keypoints sit on them up
    to a noise of about the gate's width."""
    rng = sc.rng
    d1, ang, _, _ = sc.keyframe(oracle, levelsup, n=n)
    k1 = _keypoints(rng, n)
    k1["angle"] = ang
    k2 = k1.copy()
    perm = rng.permutation(n)
    k2 = k2[perm]
    k2["x"] = (k2["x"] - rng.uniform(2, 40, n)).astype(f32)
    k2["y"] = (k2["y"] + rng.normal(0, 1.2, n) * SF[k2["octave"]]).astype(f32)
    k2["angle"] = np.mod(k2["angle"] + rng.normal(0, 4, n), 360).astype(f32)
    d2 = _noisy(rng, d1[perm], 0.03)
    ur1 = np.where(rng.random(n) < 0.3, k1["x"] - 9.0, -1.0).astype(f32) if u_right else None
    ur2 = np.where(rng.random(n) < 0.3, k2["x"] - 9.0, -1.0).astype(f32) if u_right else None
    return KF(oracle, m, sc, levelsup, k1, d1, u_right=ur1), KF(oracle, m, sc, levelsup, k2, d2, u_right=ur2)


@pytest.mark.parametrize("u_right", [False, True])
def test_triangulation_between_resident_key_frames(oracle, u_right):
    import orb_slam3_amd as osa
    sc = Scene(900 + u_right, 600, 8, 4)
    m = osa.ORBmatcher(0.6, True)
    Kc = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]])
    t = np.array([0.11, 0.0, 0.0])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = (np.linalg.inv(Kc).T @ tx @ np.linalg.inv(Kc)).astype(f32)
    total = 0
    for levelsup in (2, 4):
        a, b = _stereo_pair(oracle, m, sc, levelsup, 420, u_right)
        n = len(a.d)
        skip1 = (sc.rng.random(n) < 0.3).astype(np.uint8)
        skip2 = (sc.rng.random(n) < 0.3).astype(np.uint8)
        if levelsup == 2:                                # skip flags that switch off whole nodes
            for nd_ in range(0, len(a.fv.node_id), 3):
                skip1[a.fv.index[a.fv.node_ptr[nd_]:a.fv.node_ptr[nd_ + 1]]] = 1
            for nd_ in range(1, len(b.fv.node_id), 3):
                skip2[b.fv.index[b.fv.node_ptr[nd_]:b.fv.node_ptr[nd_ + 1]]] = 1
        for ori, coarse, strict, ep in ((True, False, False, (1e6, 1e6)), (True, False, True, (300.0, 200.0)), (False, True, False, (300.0, 200.0)),
                                        (True, True, True, (410.0, 236.0)), (False, False, True, (1e6, 1e6))):
            m.mbCheckOrientation = ori
            on, om = oracle.search_for_triangulation_pinhole(a.k, a.d, skip1, a.ur, a.fv, b.k, b.d, skip2, b.ur, b.fv, SF, SG, F, ep, coarse, ori,
                                                             fma=not strict)
            hn, hm = m.SearchForTriangulationPinhole(a.k, a.d, skip1, a.fv, b.k, b.d, skip2, b.fv, SF, SG, F, ep, a.ur, b.ur, coarse, strict)
            t_host = m.last_transfers()
            n_, m12 = m.SearchForTriangulationResident(a.dev, b.dev, skip1, skip2, SG, F, ep, coarse, strict)
            t_res = m.last_transfers()
            assert n_ == on == hn and np.array_equal(m12, om) and np.array_equal(hm, om), (levelsup, ori, coarse, strict, n_, on, hn)
            assert t_res["uploads"] == 1 and t_res["downloads"] == 1
            assert t_res["upload_bytes"] <= 2 * _pad(n) + _pad(4 * len(SG)) + 2 * 512 + 256 < t_host["upload_bytes"] // 8, (t_res, t_host)
            total += n_
        m.mbCheckOrientation = True
        n0, m0 = m.SearchForTriangulationResident(a.dev, b.dev, None, None, SG, F, (1e6, 1e6))          # no flags at all
        on, om = oracle.search_for_triangulation_pinhole(a.k, a.d, np.zeros(n, np.uint8), a.ur, a.fv, b.k, b.d, np.zeros(n, np.uint8), b.ur, b.fv, SF, SG,
                                                         F, (1e6, 1e6), False, True)
        assert n0 == on and np.array_equal(m0, om) and n0 > 40
    assert total > 150


# ---- transfers ----
def _pad(b):
    return (b + 255) // 256 * 256   # the arena's unit


def test_transfers_are_flags_and_records_only(oracle):
    import orb_slam3_amd as osa
    sc = Scene(950, 900, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 900).load(sc.F)
    D.compute_bow(sc.voc, 2, download=False)
    kfs = [_kf(oracle, m, sc, 2, n=int(sc.rng.integers(300, 420))) for _ in range(9)]
    record = 512                     # per problem: its BowProblem and its pairing record, each padded to the arena's unit at most once per call
    t_f, t_k, t_h = {}, {}, {}
    for K in (1, 9):
        sub = kfs[:K]
        m.SearchByBoWResident(D, [q.dev for q in sub], [q.valid for q in sub])
        t_f[K] = m.last_transfers()
        m.SearchByBoWDevice(D, [(q.d, q.ang, q.valid, q.fv) for q in sub])
        t_h[K] = m.last_transfers()
        m.SearchByBoWKeyFramesResident(kfs[0].dev, [q.dev for q in sub], kfs[0].valid, [q.valid for q in sub])
        t_k[K] = m.last_transfers()
        flags = sum(_pad(len(q.d)) for q in sub)
        assert t_f[K]["upload_bytes"] <= flags + K * record + 512, (K, t_f[K])                              # nothing that grows with 32 x N
        assert t_k[K]["upload_bytes"] <= flags + K * _pad(len(kfs[0].d)) + K * record + 512, (K, t_k[K])
        assert t_f[K]["upload_bytes"] < t_h[K]["upload_bytes"] // 8, (t_f[K], t_h[K])
    for t in (t_f, t_k):
        assert t[1]["uploads"] == t[9]["uploads"] == 1 and t[1]["downloads"] == t[9]["downloads"] == 1, t
        assert t[1]["xfer_launches"] + t[1]["dma_submissions"] == t[9]["xfer_launches"] + t[9]["dma_submissions"] == 2, t


# ---- sharing ----
def test_bow_key_frames_shared_between_matcher_contexts_and_threads(oracle):
    import orb_slam3_amd as osa
    sc = Scene(960, 600, 8, 4)
    A = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(A, 700).load(sc.F)
    D.compute_bow(sc.voc, 2, download=False)
    fv_f = sc.featvec(oracle, sc.d, 2)
    host = [_kf(oracle, A, sc, 2, n=int(sc.rng.integers(150, 400)), bow=False) for _ in range(6)]
    valid = [q.valid for q in host]
    want_f = [oracle.search_by_bow_frame(q.d, q.ang, q.v1, q.fv, sc.d, sc.k["angle"], fv_f, 0.75, True) for q in host]
    want_k = [oracle.search_by_bow_keyframes(host[0].d, host[0].ang, host[0].v1, host[0].fv, q.d, q.ang, q.v1, q.fv, 0.75, True) for q in host]
    errors, iters = [], 2 if EMULATOR else 30

    def loop_closing(kfs):
        try:
            B = osa.ORBmatcher(0.75, True)
            for it in range(iters):
                nm, m12 = B.SearchByBoWKeyFramesResident(kfs[0], kfs, valid[0], valid)
                for k, (on, om) in enumerate(want_k):
                    assert nm[k] == on and np.array_equal(m12[k], om), ("B", it, k)
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    # A attaches the BoW state (the attaching call is ordered before the hand-over, as the header demands) and hands the key frames over
    # WITHOUT synchronising: B's first search waits for the events
    kfs = []
    for j, q in enumerate(host):
        if j % 2:
            E = osa.DeviceFrame(A, 500).load(q.view)
            E.compute_bow(sc.voc, 2, download=False)
            kfs.append(osa.DeviceKeyFrame.from_frame(A, E, ISG).bow_from_frame(A, E))
        else:
            q.dev.compute_bow(A, sc.voc, 2, download=False)
            kfs.append(q.dev)
    if EMULATOR:   # the SIMT emulator is single-threaded: the same calls, one thread
        loop_closing(kfs)
    else:
        t = threading.Thread(target=loop_closing, args=(kfs,), daemon=True)
        t.start()
    for it in range(iters):          # meanwhile A (Tracking) searches the same key frames from its frame handle
        nm, match = A.SearchByBoWResident(D, kfs, valid)
        for k, (on, om) in enumerate(want_f):
            assert nm[k] == on and np.array_equal(match[k], om), ("A", it, k)
    if not EMULATOR:
        t.join(timeout=300)
        assert not t.is_alive(), "the LoopClosing thread did not finish"
    assert not errors, errors
    assert min(on for on, _ in want_f) > 10


# ---- refusals: each returns before anything is enqueued, and the matcher's next call still works ----
def test_refusals(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    vp = C.c_void_p
    sc = Scene(970, 400, 8, 4)
    m, m2 = osa.ORBmatcher(0.75, True), osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 400).load(sc.F)
    a, b = _kf(oracle, m, sc, 2, n=200), _kf(oracle, m, sc, 2, n=220)
    bare = _kf(oracle, m, sc, 2, n=100, bow=False)
    lv3 = KF(oracle, m, sc, 3, a.k, a.d)                                   # another levelsup
    N = len(sc.d)
    match, nm = np.zeros((4, N), np.int32), np.zeros(4, np.int32)
    one = lambda *q: (vp * len(q))(*[x.dev._h.value for x in q])          # noqa: E731
    none = (vp * 4)()

    def frame_call(frame, hs, n=1, mt=match, mm=m):
        return L.orbx_frame_search_by_bow_resident(mm._h, frame._h, n, hs, None, 0.75, 1, None if mt is None else mt.ctypes.data, N, nm.ctypes.data)

    def kf_call(k1, hs, n=1, mt=match):
        return L.orbx_keyframe_search_by_bow(m._h, None if k1 is None else k1.dev._h, None, n, hs, None, 0.75, 1, None if mt is None else mt.ctypes.data, N,
                                             nm.ctypes.data)

    assert frame_call(D, one(a)) == BAD                                   # the frame has no compute_bow yet
    D.compute_bow(sc.voc, 2, download=False)
    assert frame_call(D, one(a)) == 0
    want = nm[0]
    assert want > 10
    assert frame_call(D, one(a, bare), 2) == BAD                          # a key frame without BoW
    assert frame_call(D, one(a, lv3), 2) == BAD                           # another levelsup
    assert frame_call(D, none) == BAD                                     # a NULL key frame
    assert frame_call(D, one(a), mt=None) == BAD                          # a NULL row
    assert frame_call(D, one(a), mm=m2) == BAD                            # a handle of another matcher
    assert frame_call(D, None) == BAD
    big = (vp * (_lib.MAX_BOW_KEYFRAMES + 1))(*[a.dev._h.value] * (_lib.MAX_BOW_KEYFRAMES + 1))
    assert frame_call(D, big, _lib.MAX_BOW_KEYFRAMES + 1) == TOO_LARGE
    Fe = osa.DeviceFrame(m, 600)                                          # a fisheye-stereo handle
    nl, nr = 200, 150
    left = osa.FrameView(sc.k[:nl], sc.d[:nl + nr], 0.0, float(W), 0.0, float(H), SF)
    Fe.load_fisheye(left, sc.k[nl:nl + nr], np.full(nl, -1, np.int32), np.full(nr, -1, np.int32))
    Fe.compute_bow_fisheye(sc.voc, 2, download=False)
    assert frame_call(Fe, one(a)) == BAD
    fkf = osa.DeviceKeyFrame.from_host(m, a.view, ISG)
    assert L.orbx_keyframe_bow_from_frame(m._h, fkf._h, Fe._h) == BAD
    assert kf_call(bare, one(a)) == BAD and kf_call(a, one(bare)) == BAD and kf_call(a, one(b, lv3), 2) == BAD and kf_call(lv3, one(b)) == BAD
    assert kf_call(None, one(a)) == BAD and kf_call(a, none) == BAD and kf_call(a, one(b), mt=None) == BAD
    assert kf_call(a, big, _lib.MAX_BOW_KEYFRAMES + 1) == TOO_LARGE
    assert kf_call(a, None, 0) == 0
    g = _lib.KeyFrameGate((C.c_float * 9)(), 0.0, 0.0, 0, 0, len(SG), SG.ctypes.data)
    out = np.zeros(300, np.int32)
    tri = lambda k1, k2, gate=g, o=out: L.orbx_keyframe_search_for_triangulation(m._h, k1.dev._h, k2.dev._h, None, None, 1,   # noqa: E731
                                                                                 None if gate is None else C.byref(gate), None if o is None else o.ctypes.data)
    assert tri(a, bare) == BAD and tri(bare, a) == BAD and tri(a, lv3) == BAD and tri(a, b, None) == BAD and tri(a, b, g, None) == BAD
    g7 = _lib.KeyFrameGate((C.c_float * 9)(), 0.0, 0.0, 0, 0, 7, SG.ctypes.data)
    assert tri(a, b, g7) == BAD                                           # a level table of another length than the key frame's
    gn = _lib.KeyFrameGate((C.c_float * 9)(), 0.0, 0.0, 0, 0, len(SG), None)
    assert tri(a, b, gn) == BAD
    assert L.orbx_keyframe_compute_bow(m._h, None, sc.voc._h, 2, None, None) == BAD
    assert L.orbx_keyframe_compute_bow(m._h, bare.dev._h, None, 2, None, None) == BAD
    import torch
    if torch.cuda.device_count() > 1 and not EMULATOR:
        m1 = osa.ORBmatcher(0.75, True, device=1)
        assert L.orbx_keyframe_compute_bow(m1._h, bare.dev._h, sc.voc._h, 2, None, None) == BAD      # a context of another device
        D1 = osa.DeviceFrame(m1, 400).load(sc.F)
        v1 = osa.ORBVocabulary(sc.L, sc.cp, sc.ci, sc.nd, sc.wi, device=1).set_word_weights(sc.weights)
        D1.compute_bow(v1, 2, download=False)
        assert frame_call(D1, one(a), mm=m1) == BAD                       # key frames of another device
    assert frame_call(D, one(a)) == 0 and nm[0] == want                   # the matcher still works
    assert tri(a, b) >= 0
