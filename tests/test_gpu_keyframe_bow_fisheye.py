"""BoW on device-resident FISHEYE-STEREO key frames: KeyFrame::ComputeBoW over both cameras' rows (orbx_keyframe_compute_bow_fisheye), the
FeatureVector copied from the fisheye frame handle (orbx_keyframe_bow_from_frame_fisheye) and the three BoW-guided matchers with both sides resident
(orbx_frame_search_by_bow_resident_fisheye, orbx_keyframe_search_by_bow_fisheye, orbx_keyframe_search_for_triangulation_fisheye).

Features [0, N_left) are the left camera's, [N_left, N) the right one's, on every side and in every result.  Expectations come from the CPU oracle
(bow_transform, search_by_bow_frame_fisheye, search_by_bow_keyframes with the right camera's features masked, search_for_triangulation_kb8) on the host
arrays, with the FeatureVectors built here from the oracle's transform (stopped words dropped); every resident result is also compared with the
host-pointer entry point for the same arrays.  Every comparison is equality of integers, no row excluded; the non-emptiness floors are asserted on the
ORACLE's counts (about half of what it returns for the seed, the measured value in a comment)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from test_gpu_frame_bow import _noisy
from test_gpu_frame_bow_fisheye import RigScene
from test_gpu_frame_fisheye import SF, H, W, _extract_pairs, _kps
from test_gpu_matcher import _random_vocabulary

pytestmark = pytest.mark.gpu

f32 = np.float32
BAD, TOO_LARGE, STALE = -2, -7, -9
SG = (SF * SF).astype(f32)            # mvLevelSigma2
ISG = (f32(1.0) / SG).astype(f32)     # mvInvLevelSigma2
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))
BOUNDS = (0.0, float(W), 0.0, float(H))


def _pad(b):
    return (b + 255) // 256 * 256   # the arena's unit


class RigKF:
    """A rig key frame on the host (what the host-pointer entry points and the oracle take) and the same key frame resident, made from the host
    arrays (how="host") or from a host-loaded fisheye handle (how="frame"), with BoW computed on the key frame (bow="compute"), copied from that
    handle (bow="frame") or not attached (bow=None).  sc: anything with voc / featvec (a RigScene, a TriScene)."""

    def __init__(self, oracle, m, sc, levelsup, kl, kr, desc, valid=None, how="host", bow="compute", bounds=BOUNDS, sf=SF):
        import orb_slam3_amd as osa
        self.kl, self.kr, self.d, self.valid = kl, kr, np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), valid
        self.nl, self.n = len(kl), len(kl) + len(kr)
        assert len(self.d) == self.n
        self.k = np.concatenate([kl, kr])
        self.ang = np.ascontiguousarray(self.k["angle"], f32)
        self.fv = sc.featvec(oracle, self.d, levelsup)
        self.view = osa.FrameView(kl, self.d, *bounds, sf)
        isg = (f32(1.0) / (sf * sf)).astype(f32)
        self.handle = None
        if how == "host":
            self.dev = osa.DeviceKeyFrame.from_host_fisheye(m, self.view, kr, isg)
        else:
            self.handle = osa.DeviceFrame(m, self.n + 37).load_fisheye(self.view, kr, np.full(self.nl, -1, np.int32), np.full(self.n - self.nl, -1, np.int32))
            self.dev = osa.DeviceKeyFrame.from_frame_fisheye(m, self.handle, isg)
        if bow == "frame":
            self.handle.compute_bow_fisheye(sc.voc, levelsup, download=False)
            self.dev.bow_from_frame_fisheye(m, self.handle)
        elif bow:
            self.dev.compute_bow_fisheye(m, sc.voc, levelsup, download=False)

    @property
    def v1(self):
        return np.ones(self.n, np.uint8) if self.valid is None else self.valid

    @property
    def left(self):
        """valid with every right-camera feature marked as having no map point (ORBmatcher.cc:800-802, :820-822 skip them)."""
        v = self.v1.copy()
        v[self.nl:] = 0
        return v

    @property
    def host(self):
        return self.d, self.ang, self.valid, self.fv


class PairedRigScene(RigScene):
    """A RigScene whose right-camera features are near copies of left-camera ones (the rig's lapping area): a key-frame feature that finds its left
    match within TH_LOW usually has a right candidate within TH_LOW too (ORBmatcher.cc:318-377 looks at the right camera only then)."""

    def __init__(self, seed, nl, nr, *a, **kw):
        super().__init__(seed, nl, nr, *a, **kw)
        self.d[nl:] = _noisy(self.rng, self.d[self.rng.permutation(nl)[:nr]], 0.03)


def _rig_kf_from(oracle, m, sc, levelsup, base, n, valid="random", **kw):
    """A key frame that sees what key frame `base` sees: noisy copies of n of its features in random order, rotated by about 25 degrees."""
    rng = sc.rng
    src = rng.integers(0, base.n, n)
    k = _kps(rng, n)
    k["angle"] = np.mod(base.ang[src] + 25.0 + rng.normal(0, 3, n), 360).astype(f32)
    nl = (n * 11) // 20
    v = (rng.random(n) < 0.8).astype(np.uint8) if valid == "random" else None
    return RigKF(oracle, m, sc, levelsup, k[:nl], k[nl:], _noisy(rng, base.d[src], 0.04), v, **kw)


def _rig_kf(oracle, m, sc, levelsup, related=True, n=None, valid="random", **kw):
    """A key frame of sc.keyframe()'s features, the first ~55 % of them the left camera's."""
    d, ang, v, _ = sc.keyframe(oracle, levelsup, related=related, n=n)
    k = _kps(sc.rng, len(d))
    k["angle"] = ang
    nl = (len(d) * 11) // 20
    v = {"random": v, "none": None}[valid]
    return RigKF(oracle, m, sc, levelsup, k[:nl], k[nl:], d, v, **kw)


# ---- (1) attaching BoW ----
@pytest.mark.parametrize("how", ["host", "frame"])
@pytest.mark.parametrize("vocab", [(8, 4), (12, 3)])
def test_attach_ids_equal_the_oracle(oracle, vocab, how):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    k, Lv = vocab
    sc = RigScene(1100 + k, 300, 200, k, Lv, ragged=(k == 8))
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m)
    other = RigScene(5, 10, 10).voc
    for levelsup in (0, 2, Lv):
        q = _rig_kf(oracle, m, sc, levelsup, n=500, how=how, bow=None)
        assert (q.nl, q.n) == (275, 500)
        w, node = q.dev.compute_bow_fisheye(m, sc.voc, levelsup)
        ow, onode = sc.transform(oracle, q.d, levelsup)
        assert len(w) == q.n and np.array_equal(w, ow) and np.array_equal(node, onode)
        assert (sc.weights[ow] <= 0).any() and (sc.weights[ow] > 0).sum() > q.n // 2          # some features are stopped, most are not
        w2, node2 = q.dev.compute_bow_fisheye(m, sc.voc, levelsup)                            # not computed again: the ids that were kept
        assert np.array_equal(w2, w) and np.array_equal(node2, node)
        assert L.orbx_keyframe_compute_bow_fisheye(m._h, q.dev._h, sc.voc._h, levelsup + 1, None, None) == BAD   # another levelsup
        assert L.orbx_keyframe_compute_bow_fisheye(m._h, q.dev._h, other._h, levelsup, None, None) == BAD        # another vocabulary
        assert L.orbx_keyframe_compute_bow_fisheye(m._h, q.dev._h, sc.voc._h, levelsup, None, None) == 0
        if how == "frame":   # the copy from the handle: the same ids and the same search results
            c = RigKF(oracle, m, sc, levelsup, q.kl, q.kr, q.d, q.valid, how="frame", bow="frame")
            w3, node3 = c.dev.compute_bow_fisheye(m, sc.voc, levelsup)
            assert np.array_equal(w3, w) and np.array_equal(node3, node)
            D.compute_bow_fisheye(sc.voc, levelsup, download=False)
            n1, r1 = m.SearchByBoWResidentFisheye(D, [q.dev, c.dev], [q.valid, q.valid])
            on, om = oracle.search_by_bow_frame_fisheye(q.d, q.ang, q.v1, q.fv, sc.d, sc.angle, sc.nl, sc.featvec(oracle, sc.d, levelsup), 0.75, True)
            assert list(n1) == [on, on] and np.array_equal(r1[0], om) and np.array_equal(r1[1], om)
            n2, r2 = m.SearchByBoWKeyFramesResidentFisheye(c.dev, [q.dev, c.dev], q.valid, [q.valid, q.valid])
            n3, r3 = m.SearchByBoWKeyFramesResidentFisheye(q.dev, [q.dev, c.dev], q.valid, [q.valid, q.valid])
            assert np.array_equal(n2, n3) and np.array_equal(r2, r3)
            if levelsup == 2:
                assert on > 42          # oracle: 84 (8, 4), 103 (12, 3)


def test_bow_from_frame_preconditions_and_stale(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    sc = RigScene(1120, 300, 200)
    m = osa.ORBmatcher(0.75, True)
    q = _rig_kf(oracle, m, sc, 2, n=300, how="frame", bow=None)
    cur = sc.handle(m)
    cur.compute_bow_fisheye(sc.voc, 2, download=False)
    call = lambda kf, frame: L.orbx_keyframe_bow_from_frame_fisheye(m._h, kf._h, frame._h)   # noqa: E731
    assert call(q.dev, q.handle) == BAD                     # no compute_bow_fisheye since the load
    q.handle.compute_bow_fisheye(sc.voc, 2, download=False)
    assert call(q.dev, cur) == BAD                          # not the handle the key frame was made from
    late = osa.DeviceKeyFrame.from_frame_fisheye(m, q.handle, ISG)
    assert call(q.dev, q.handle) == 0
    assert call(q.dev, q.handle) == BAD                     # set once
    q.handle.load_fisheye(q.view, q.kr, np.full(q.nl, -1, np.int32), np.full(q.n - q.nl, -1, np.int32))   # reloaded: another frame by now
    q.handle.compute_bow_fisheye(sc.voc, 2, download=False)
    assert call(late, q.handle) == STALE


# ---- (2) frame against K resident rig key frames ----
def _frame_list(oracle, m, sc, levelsup, K):
    """K key frames: related ones, from K = 3 on an unrelated one and one without flags, at K = 9 the same key frame twice; made both ways."""
    kfs = [_rig_kf(oracle, m, sc, levelsup, how=("frame" if j % 2 else "host"), bow=("frame" if j % 4 == 1 else "compute")) for j in range(K)]
    if K >= 3:
        kfs[1] = _rig_kf(oracle, m, sc, levelsup, related=False)
        kfs[2] = _rig_kf(oracle, m, sc, levelsup, valid="none")
    if K >= 9:
        kfs[7] = kfs[4]
    return kfs


@pytest.mark.parametrize("K", [1, 3, 9])
def test_frame_against_resident_rig_key_frames(oracle, K):
    import orb_slam3_amd as osa
    sc = PairedRigScene(1200 + K, 520, 480)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m, 1100)
    for levelsup in (2, 4):   # 4 = L: every feature in node 0, a node of 1000 frame features (the big-node path)
        D.compute_bow_fisheye(sc.voc, levelsup, download=False)
        fv_f = sc.featvec(oracle, sc.d, levelsup)
        if levelsup == 4:
            assert len(fv_f.node_id) == 1 and fv_f.node_ptr[-1] > 64
        kfs = _frame_list(oracle, m, sc, levelsup, K)
        for ratio, ori in ((0.75, True), (0.9, False)):
            m.mfNNratio, m.mbCheckOrientation = ratio, ori
            nm, match = m.SearchByBoWResidentFisheye(D, [q.dev for q in kfs], [q.valid for q in kfs])
            assert nm.shape == (K,) and match.shape == (K, len(sc.d))
            hn, hmatch = m.SearchByBoWDeviceFisheye(D, [q.host for q in kfs])     # today's call with the key frames as host arrays
            assert np.array_equal(nm, hn) and np.array_equal(match, hmatch)
            for k, q in enumerate(kfs):
                on, om = oracle.search_by_bow_frame_fisheye(q.d, q.ang, q.v1, q.fv, sc.d, sc.angle, sc.nl, fv_f, ratio, ori)
                assert nm[k] == on and np.array_equal(match[k], om), (k, levelsup, ratio, ori, nm[k], on)
                if k != 1:   # oracle, related key frames: 73 .. 414 matches, 47 .. 223 on the frame's left camera, 26 .. 191 on its right one,
                    #              30 .. 150 naming a right-camera feature of the key frame
                    assert on > 36 and (om[:sc.nl] >= 0).sum() > 23 and (om[sc.nl:] >= 0).sum() > 13 and (om >= q.nl).sum() > 15, (k, levelsup, on)
                else:
                    assert on == 0
            if K >= 9:
                assert nm[7] == nm[4] and np.array_equal(match[7], match[4])
    nm, match = m.SearchByBoWResidentFisheye(D, [])
    assert nm.shape == (0,) and match.shape == (0, 1000)


# ---- (3) key frame against K key frames ----
@pytest.mark.parametrize("K", [1, 4])
def test_rig_keyframe_against_rig_key_frames(oracle, K):
    import orb_slam3_amd as osa
    sc = RigScene(1300 + K, 520, 480)
    m = osa.ORBmatcher(0.75, True)
    for levelsup in (2, 4):
        kf1 = _rig_kf(oracle, m, sc, levelsup, n=500, how="frame", bow="frame")
        kfs = [kf1] + [_rig_kf_from(oracle, m, sc, levelsup, kf1, int(sc.rng.integers(200, 420)), valid=("none" if j == 2 else "random"))
                       for j in range(1, K)]
        for ratio, ori in ((0.75, True), (0.9, False)):
            m.mfNNratio, m.mbCheckOrientation = ratio, ori
            nm, m12 = m.SearchByBoWKeyFramesResidentFisheye(kf1.dev, [q.dev for q in kfs], kf1.valid, [q.valid for q in kfs])
            assert m12.shape == (K, 500)
            for k, q in enumerate(kfs):
                on, om = oracle.search_by_bow_keyframes(kf1.d, kf1.ang, kf1.left, kf1.fv, q.d, q.ang, q.left, q.fv, ratio, ori)
                assert nm[k] == on and np.array_equal(m12[k], om), (k, levelsup, ratio, ori, nm[k], on)
                hn, hm = m.SearchByBoWKeyFrames(kf1.d, kf1.ang, kf1.left, kf1.fv, q.d, q.ang, q.left, q.fv)   # today's call, with masks
                assert hn == on and np.array_equal(hm, om)
                assert (m12[k][kf1.nl:] == -1).all() and (m12[k] < q.nl).all()
                assert on > (89 if k == 0 else 8), (k, levelsup, on)   # oracle: 178 .. 205 against itself, 16 .. 41 against the others
        nm0, m0 = m.SearchByBoWKeyFramesResidentFisheye(kf1.dev, [q.dev for q in kfs])            # no flags at all: the right rows are still off
        for k, q in enumerate(kfs):
            v1, v2 = np.ones(kf1.n, np.uint8), np.ones(q.n, np.uint8)
            v1[kf1.nl:] = 0
            v2[q.nl:] = 0
            on, om = oracle.search_by_bow_keyframes(kf1.d, kf1.ang, v1, kf1.fv, q.d, q.ang, v2, q.fv, 0.9, False)
            assert nm0[k] == on and np.array_equal(m0[k], om)


# ---- (4) triangulation ----
class TriScene:
    """Two key frames of a fisheye rig looking at common points (synth.make_fisheye_keyframes) and a vocabulary whose node descriptors are sampled
    from the two key frames' descriptors; one_proto: all descriptors noisy copies of ONE prototype (every pair of a node passes the distance test)."""

    transform = RigScene.transform
    featvec = RigScene.featvec

    def __init__(self, seed, n_pts, k=8, L=4, one_proto=False):
        import orb_slam3_amd as osa
        from orb_slam3_amd import synth
        self.rng = rng = np.random.default_rng(seed)
        self.k1, self.nl1, d1, self.id1, self.k2, self.nl2, d2, self.id2, self.R12, self.t12, self.cams = synth.make_fisheye_keyframes(rng, n_pts)
        if one_proto:
            proto = rng.integers(0, 256, (1, 32), dtype=np.uint8)
            d1, d2 = _noisy(rng, np.repeat(proto, len(d1), 0), 0.03), _noisy(rng, np.repeat(proto, len(d2), 0), 0.03)
        self.d1, self.d2 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32), np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        self.cp, self.ci, nd, self.wi = _random_vocabulary(rng, k, L, True)
        pool = np.concatenate([self.d1, self.d2])
        self.nd = _noisy(rng, pool[rng.integers(0, len(pool), len(nd))], 0.05)
        self.L = L
        nw = int(self.wi.max()) + 1
        self.weights = rng.uniform(0.2, 3.0, nw)
        self.weights[rng.random(nw) < 0.05] = 0.0
        self.voc = osa.ORBVocabulary(L, self.cp, self.ci, self.nd, self.wi).set_word_weights(self.weights)
        self.skip1 = (rng.random(len(self.k1)) < 0.2).astype(np.uint8)
        self.skip2 = (rng.random(len(self.k2)) < 0.2).astype(np.uint8)

    def pair(self, oracle, m, levelsup, **kw):
        a = RigKF(oracle, m, self, levelsup, self.k1[:self.nl1], self.k1[self.nl1:], self.d1, **kw)
        b = RigKF(oracle, m, self, levelsup, self.k2[:self.nl2], self.k2[self.nl2:], self.d2)
        return a, b

    def expected(self, oracle, a, b, s1, s2, coarse, ori):
        return oracle.search_for_triangulation_kb8(a.k, a.nl, a.d, s1, a.fv, b.k, b.nl, b.d, s2, b.fv, SG, SG, self.cams, self.cams, self.R12, self.t12,
                                                   coarse, ori)

    def resident(self, m, a, b, s1, s2, coarse):
        return m.SearchForTriangulationResidentKB8(a.dev, b.dev, s1, s2, SG, SG, self.cams, self.cams, self.R12, self.t12, coarse)

    def host(self, m, a, b, s1, s2, coarse):
        return m.SearchForTriangulationKB8(a.k, a.nl, a.d, s1, a.fv, b.k, b.nl, b.d, s2, b.fv, SG, SG, self.cams, self.cams, self.R12, self.t12, coarse)


@pytest.fixture(scope="module")
def tri_scene():
    return TriScene(701, 420)


@pytest.mark.parametrize("levelsup", [2, 4])
def test_triangulation_between_resident_rig_key_frames(oracle, tri_scene, levelsup):
    import orb_slam3_amd as osa
    sc = tri_scene
    m = osa.ORBmatcher(0.6, True)
    a, b = sc.pair(oracle, m, levelsup, how="frame", bow="frame")
    if levelsup == 4:
        assert len(a.fv.node_id) == 1 and a.fv.node_ptr[-1] > 400      # one node of about 580 features
    else:
        assert len(a.fv.node_id) > 20 and np.diff(a.fv.node_ptr).max() <= 64
    for ori, coarse in ((True, False), (False, False), (True, True)):
        m.mbCheckOrientation = ori
        on, om = sc.expected(oracle, a, b, sc.skip1, sc.skip2, coarse, ori)
        hn, hm = sc.host(m, a, b, sc.skip1, sc.skip2, coarse)
        t_host = m.last_transfers()
        n, m12 = sc.resident(m, a, b, sc.skip1, sc.skip2, coarse)
        t_res = m.last_transfers()
        assert n == on == hn and np.array_equal(m12, om) and np.array_equal(hm, om), (levelsup, ori, coarse, n, on, hn)
        assert t_res["uploads"] == 1 and t_res["downloads"] == 1
        # two flag rows, two level tables, one Kb8Gate (336 B), the problem's three records (512 B), each array padded to the arena's unit once
        bound = _pad(a.n) + _pad(b.n) + 2 * _pad(4 * len(SG)) + _pad(336) + 512 + 3 * 256
        assert t_res["upload_bytes"] <= bound < t_host["upload_bytes"] // 8, (t_res, t_host)
        hit = om >= 0
        if coarse:
            assert on > (31 if levelsup == 2 else 52)                  # oracle: 63 (levelsup 2), 105 (L)
        else:   # oracle, gated: 57 / 152 matches with / without the rotation check at levelsup 2, 95 / 317 at L
            assert on > (28 if levelsup == 2 else 47)
            r1, r2 = np.nonzero(hit)[0] >= a.nl, om[hit] >= b.nl
            # accepted pairs in all four camera pairs: oracle at least 12 (levelsup 2), 17 (L) in each of ll, lr, rl, rr
            assert all(((r1 == x) & (r2 == y)).sum() > 5 for x in (False, True) for y in (False, True))
    m.mbCheckOrientation = True
    n0, m0 = sc.resident(m, a, b, None, None, False)                                    # no flags at all
    z1, z2 = np.zeros(a.n, np.uint8), np.zeros(b.n, np.uint8)
    on, om = sc.expected(oracle, a, b, z1, z2, False, True)
    assert n0 == on and np.array_equal(m0, om)


def test_triangulation_list_flush(oracle):
    """170 points, all descriptors noisy copies of one prototype, levelsup L: one node of about 237 x 233 pairs, every one within TH_LOW -- the
    2048-entry pair list of k_tri_kb8_resident flushes repeatedly and the gate alone decides (equal distances: the later candidate, :1017)."""
    import orb_slam3_amd as osa
    sc = TriScene(811, 170, one_proto=True)
    m = osa.ORBmatcher(0.6, True)
    a, b = sc.pair(oracle, m, 4)
    assert len(a.fv.node_id) == 1 and len(b.fv.node_id) == 1 and a.fv.node_ptr[-1] * b.fv.node_ptr[-1] > 20 * 2048   # 225 x 216 pairs
    for ori in (True, False):
        m.mbCheckOrientation = ori
        on, om = sc.expected(oracle, a, b, sc.skip1, sc.skip2, False, ori)
        n, m12 = sc.resident(m, a, b, sc.skip1, sc.skip2, False)
        hn, hm = sc.host(m, a, b, sc.skip1, sc.skip2, False)
        assert n == on == hn and np.array_equal(m12, om) and np.array_equal(hm, om), (ori, n, on, hn)
        assert on > (27 if ori else 85)   # oracle: 54 with the rotation check, 171 without


# ---- the batch-loaded handle: counts pending, a gap behind the left rows ----
def test_key_frames_of_a_batch_loaded_handle_with_a_row_gap(oracle):
    """Rig key frames made from a batch-loaded handle (320 x 240, capacity above N): the right rows start at the handle's left capacity, the counts are
    on the device only.  Made three ways -- BoW copied from the handle with the counts pending, computed on the key frame with the counts pending,
    copied after the handle's counts came home (then the key frame's right rows start at N_left: the copy moves and renumbers them) -- they give the
    ids and the results of all three searches that a key frame rebuilt from the downloaded host arrays gives, and end with the same counts."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    w, h, nb, nf = 320, 240, 2, 400
    left, right = _extract_pairs(w, h, nb, nf)
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    exl.extract_batch_device(left.data_ptr(), nb, w, h, w, w * h, (0, 0))
    exr.extract_batch_device(right.data_ptr(), nb, w, h, w, w * h, (0, 0))
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    capl, capr = exl.batch_view().cap, exr.batch_view().cap
    sf = exl.GetScaleFactors().astype(f32)
    sg = (sf * sf).astype(f32)
    isg = (f32(1.0) / sg).astype(f32)
    bounds = (0.0, float(w), 0.0, float(h))
    outs = [(exl.download(t), exr.download(t)) for t in range(nb)]
    (_, kl, dl), (_, kr, dr) = outs[0]
    nl, nr = len(kl), len(kr)
    assert capl > nl and nr > 0     # a gap between N_left and the right rows
    rng = np.random.default_rng(6)

    class Voc:
        transform = RigScene.transform
        featvec = RigScene.featvec
    sc = Voc()
    sc.cp, sc.ci, nd, sc.wi = _random_vocabulary(rng, 8, 4)
    pool = np.concatenate([o[2] for pair in outs for o in pair])
    sc.nd = _noisy(rng, pool[rng.integers(0, len(pool), len(nd))], 0.03)
    sc.L = 4
    sc.weights = rng.uniform(0.1, 1.0, int(sc.wi.max()) + 1)
    sc.weights[rng.random(len(sc.weights)) < 0.05] = 0.0
    sc.voc = osa.ORBVocabulary(4, sc.cp, sc.ci, sc.nd, sc.wi).set_word_weights(sc.weights)
    m = osa.ORBmatcher(0.75, True)
    cap = capl + capr

    def load(t):
        return osa.DeviceFrame(m, cap).load_stereo_fisheye_batch(exl, exr, t, bounds=bounds, scale_factors=sf)   # the counts stay on the device

    def copied():      # BoW copied from the handle, everything pending
        D = load(0)
        D.compute_bow_fisheye(sc.voc, 2, download=False)
        return osa.DeviceKeyFrame.from_frame_fisheye(m, D, isg).bow_from_frame_fisheye(m, D)

    def computed():    # BoW computed on the key frame's own rows, counts pending
        q = osa.DeviceKeyFrame.from_frame_fisheye(m, load(0), isg)
        q.compute_bow_fisheye(m, sc.voc, 2, download=False)
        return q

    def counted():     # the handle's counts at home before the copy: the key frame's right rows start at N_left, the handle's at its left capacity
        D = load(0)
        D.compute_bow_fisheye(sc.voc, 2, download=False)
        assert D.counts() == (nl, nr)
        return osa.DeviceKeyFrame.from_frame_fisheye(m, D, isg).bow_from_frame_fisheye(m, D)

    ways = (copied, computed, counted)
    desc = np.concatenate([dl, dr]).reshape(-1, 32)
    want = RigKF(oracle, m, sc, 2, kl, kr, desc, bounds=bounds, sf=sf)                   # rebuilt from the downloaded host arrays
    N = nl + nr
    valid = (rng.random(N) < 0.8).astype(np.uint8)
    ow, onode = sc.transform(oracle, desc, 2)
    # the ids, with the counts pending
    for make in ways:
        q = make()
        w_, node_ = q.compute_bow_fisheye(m, sc.voc, 2, cap=cap)
        assert np.array_equal(w_, ow) and np.array_equal(node_, onode), make.__name__
        assert q.counts() == (nl, nr)
    # the frame form: the handle of the other pair against the key frames, no count read before the search
    (_, fl, fdl), (_, fr, fdr) = outs[1]
    fdesc = np.concatenate([fdl, fdr]).reshape(-1, 32)
    fang = np.concatenate([fl["angle"], fr["angle"]]).astype(f32)
    F = load(1)
    F.compute_bow_fisheye(sc.voc, 2, download=False)
    kfs = [make() for make in ways]
    nm, match = m.SearchByBoWResidentFisheye(F, kfs + [want.dev])
    on, om = oracle.search_by_bow_frame_fisheye(desc, want.ang, np.ones(N, np.uint8), want.fv, fdesc, fang, len(fl), sc.featvec(oracle, fdesc, 2), 0.75, True)
    assert match.shape == (4, len(fdesc)) and list(nm) == [on] * 4 and all(np.array_equal(match[k], om) for k in range(4))
    assert on > 158 and (om[len(fl):] >= 0).sum() > 61 and (om >= nl).sum() > 33        # oracle: 317 matches, 122 on the right camera, 67 right values
    assert [q.counts() for q in kfs] == [(nl, nr)] * 3 and F.counts() == (len(fl), len(fr))
    nm2, match2 = m.SearchByBoWResidentFisheye(F, kfs + [want.dev], [valid] * 4)         # again with the counts at home, the gap still there, and flags
    on, om = oracle.search_by_bow_frame_fisheye(desc, want.ang, valid, want.fv, fdesc, fang, len(fl), sc.featvec(oracle, fdesc, 2), 0.75, True)
    assert list(nm2) == [on] * 4 and all(np.array_equal(match2[k], om) for k in range(4))
    # key frame against key frames, pending on both sides (match_stride = the capacity)
    other = RigKF(oracle, m, sc, 2, fl, fr, fdesc, bounds=bounds, sf=sf)
    left_of = lambda n_, nl_: np.concatenate([np.ones(nl_, np.uint8), np.zeros(n_ - nl_, np.uint8)])   # noqa: E731
    on, om = oracle.search_by_bow_keyframes(desc, want.ang, left_of(N, nl), want.fv, fdesc, other.ang, left_of(other.n, other.nl), other.fv, 0.75, True)
    sn, sm = oracle.search_by_bow_keyframes(desc, want.ang, left_of(N, nl), want.fv, desc, want.ang, left_of(N, nl), want.fv, 0.75, True)
    assert on > 75 and sn > 197      # oracle: 150 against the other pair, 395 against itself
    from orb_slam3_amd import _lib
    L = _lib.lib()
    for make in ways:
        q1, q2 = make(), make()
        rows, cnt = np.full((2, cap), -7, np.int32), np.zeros(2, np.int32)
        hs = (C.c_void_p * 2)(other.dev._h.value, q2._h.value)
        assert L.orbx_keyframe_search_by_bow_fisheye(m._h, q1._h, None, 2, hs, None, 0.75, 1, rows.ctypes.data, cap, cnt.ctypes.data) == 0
        assert list(cnt) == [on, sn] and np.array_equal(rows[0, :N], om) and np.array_equal(rows[1, :N], sm), make.__name__
        assert (rows[:, N:] == -7).all()                                                 # untouched beyond N
        assert q1.counts() == (nl, nr) and q2.counts() == (nl, nr)
    # triangulation, coarse and gated (the poses of an arbitrary rig: the oracle decides), the batch-made key frame as kf1 and, its counts pending and
    # without flags of its own, as kf2
    _, _, _, _, _, _, _, _, R12, t12, cams = synth.make_fisheye_keyframes(np.random.default_rng(3), 50)
    s1, s2 = (rng.random(N) < 0.2).astype(np.uint8), (rng.random(other.n) < 0.2).astype(np.uint8)
    z1 = np.zeros(N, np.uint8)
    m6 = osa.ORBmatcher(0.6, True)
    for coarse in (True, False):
        on, om = oracle.search_for_triangulation_kb8(want.k, nl, desc, s1, want.fv, other.k, other.nl, fdesc, s2, other.fv, sg, sg, cams, cams, R12, t12,
                                                     coarse, True)
        on2, om2 = oracle.search_for_triangulation_kb8(other.k, other.nl, fdesc, s2, other.fv, want.k, nl, desc, z1, want.fv, sg, sg, cams, cams, R12, t12,
                                                       coarse, True)
        assert on > (188 if coarse else 124) and on2 > (198 if coarse else 104)          # oracle: 377 and 396 coarse, 249 and 209 gated
        for make in ways + (lambda: want.dev,):
            n_, m12 = m6.SearchForTriangulationResidentKB8(make(), other.dev, s1, s2, sg, sg, cams, cams, R12, t12, coarse)
            assert n_ == on and np.array_equal(m12, om), (make.__name__, coarse, n_, on)
            q2 = make()
            n_, m12 = m6.SearchForTriangulationResidentKB8(other.dev, q2, s2, None, sg, sg, cams, cams, R12, t12, coarse)
            assert n_ == on2 and np.array_equal(m12, om2), (make.__name__, coarse, n_, on2)
            assert q2.counts() == (nl, nr)


# ---- (5) transfers ----
def test_transfers_are_flags_and_records_only(oracle):
    import orb_slam3_amd as osa
    sc = RigScene(1400, 520, 480)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m)
    D.compute_bow_fisheye(sc.voc, 2, download=False)
    kfs = [_rig_kf(oracle, m, sc, 2, n=int(sc.rng.integers(300, 420))) for _ in range(9)]
    # per problem: its BowProblem (336 B), its pairing record (80 B) and its renumbering record (88 B) -- 504 B; each of the three arrays is padded to
    # the arena's unit at most once per call
    record, arrays = 512, 3 * 256
    t_f, t_k, t_h = {}, {}, {}
    for K in (1, 9):
        sub = kfs[:K]
        m.SearchByBoWResidentFisheye(D, [q.dev for q in sub], [q.valid for q in sub])
        t_f[K] = m.last_transfers()
        m.SearchByBoWDeviceFisheye(D, [q.host for q in sub])
        t_h[K] = m.last_transfers()
        m.SearchByBoWKeyFramesResidentFisheye(kfs[0].dev, [q.dev for q in sub], kfs[0].valid, [q.valid for q in sub])
        t_k[K] = m.last_transfers()
        flags = sum(_pad(q.n) for q in sub)
        assert t_f[K]["upload_bytes"] <= flags + K * record + arrays, (K, t_f[K])                              # nothing that grows with 32 x N
        assert t_k[K]["upload_bytes"] <= flags + K * _pad(kfs[0].n) + K * record + arrays, (K, t_k[K])
        assert t_f[K]["upload_bytes"] < t_h[K]["upload_bytes"] // 8, (t_f[K], t_h[K])
    for t in (t_f, t_k):
        assert t[1]["uploads"] == t[9]["uploads"] == 1 and t[1]["downloads"] == t[9]["downloads"] == 1, t
        assert t[1]["xfer_launches"] + t[1]["dma_submissions"] == t[9]["xfer_launches"] + t[9]["dma_submissions"] == 2, t


# ---- (6) sharing and refusals ----
def test_rig_key_frames_shared_between_matcher_contexts_and_threads(oracle):
    import orb_slam3_amd as osa
    sc = PairedRigScene(1500, 320, 280)
    A = osa.ORBmatcher(0.75, True)
    D = sc.handle(A)
    D.compute_bow_fisheye(sc.voc, 2, download=False)
    fv_f = sc.featvec(oracle, sc.d, 2)
    host = [_rig_kf(oracle, A, sc, 2, how="host", bow=None)]
    host += [_rig_kf_from(oracle, A, sc, 2, host[0], 300, how=("frame" if j % 2 else "host"), bow=None) for j in range(1, 4)]
    valid = [q.valid for q in host]
    want_f = [oracle.search_by_bow_frame_fisheye(q.d, q.ang, q.v1, q.fv, sc.d, sc.angle, sc.nl, fv_f, 0.75, True) for q in host]
    want_k = [oracle.search_by_bow_keyframes(host[0].d, host[0].ang, host[0].left, host[0].fv, q.d, q.ang, q.left, q.fv, 0.75, True) for q in host]
    errors, iters = [], 2 if EMULATOR else 20

    def loop_closing(kfs):
        try:
            B = osa.ORBmatcher(0.75, True)
            for it in range(iters):
                nm, m12 = B.SearchByBoWKeyFramesResidentFisheye(kfs[0], kfs, valid[0], valid)
                for k, (on, om) in enumerate(want_k):
                    assert nm[k] == on and np.array_equal(m12[k], om), ("B", it, k)
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    # A attaches the BoW state and hands the key frames over WITHOUT synchronising: B's first search waits for the events
    for j, q in enumerate(host):
        if j % 2:
            q.handle.compute_bow_fisheye(sc.voc, 2, download=False)
            q.dev.bow_from_frame_fisheye(A, q.handle)
        else:
            q.dev.compute_bow_fisheye(A, sc.voc, 2, download=False)
    kfs = [q.dev for q in host]
    if EMULATOR:   # the SIMT emulator is single-threaded: the same calls, one thread
        loop_closing(kfs)
    else:
        t = threading.Thread(target=loop_closing, args=(kfs,), daemon=True)
        t.start()
    for it in range(iters):          # meanwhile A (Tracking) searches the same key frames from its frame handle
        nm, match = A.SearchByBoWResidentFisheye(D, kfs, valid)
        for k, (on, om) in enumerate(want_f):
            assert nm[k] == on and np.array_equal(match[k], om), ("A", it, k)
    if not EMULATOR:
        t.join(timeout=300)
        assert not t.is_alive(), "the LoopClosing thread did not finish"
    assert not errors, errors
    assert min(on for on, _ in want_f) > 25 and min(on for on, _ in want_k) > 7   # oracle: 50 .. 88 and 15 .. 114


def test_refusals_leave_the_transfer_counters_alone(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    from test_gpu_frame_bow import Scene
    L = _lib.lib()
    vp = C.c_void_p
    sc = RigScene(1600, 220, 180)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m)
    D.compute_bow_fisheye(sc.voc, 2, download=False)
    a, b = _rig_kf(oracle, m, sc, 2, n=200), _rig_kf(oracle, m, sc, 2, n=220)
    bare = _rig_kf(oracle, m, sc, 2, n=100, bow=None)
    lv3 = RigKF(oracle, m, sc, 3, a.kl, a.kr, a.d)                         # another levelsup
    sc2 = RigScene(1601, 220, 180)
    foreign = _rig_kf(oracle, m, sc2, 2, n=150)                            # another vocabulary
    # a monocular key frame with BoW, and a monocular handle
    ms = Scene(1602, 300, 8, 4)
    mono_view = osa.FrameView(ms.k, ms.d, 0.0, float(W), 0.0, float(H), SF)
    mono = osa.DeviceKeyFrame.from_host(m, mono_view, ISG)
    mono.compute_bow(m, ms.voc, 2, download=False)
    Dm = osa.DeviceFrame(m, 300).load(mono_view)
    Dm.compute_bow(ms.voc, 2, download=False)
    N = len(sc.d)
    match, nm, out = np.zeros((4, N), np.int32), np.zeros(4, np.int32), np.zeros(400, np.int32)
    hs = lambda *q: (vp * len(q))(*[(x.dev if isinstance(x, RigKF) else x)._h.value for x in q])   # noqa: E731
    g = _lib.KeyFrameKb8Gate(SG.ctypes.data, SG.ctypes.data, len(SG), (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 36)(), (C.c_float * 12)(), 0)
    h_ = lambda x: (x.dev if isinstance(x, RigKF) else x)._h   # noqa: E731

    def frame_call(frame, lst, n):
        return L.orbx_frame_search_by_bow_resident_fisheye(m._h, frame._h, n, lst, None, 0.75, 1, match.ctypes.data, N, nm.ctypes.data)

    def kf_call(k1, lst, n):
        return L.orbx_keyframe_search_by_bow_fisheye(m._h, h_(k1), None, n, lst, None, 0.75, 1, match.ctypes.data, N, nm.ctypes.data)

    def tri(k1, k2, gate=g):
        return L.orbx_keyframe_search_for_triangulation_fisheye(m._h, h_(k1), h_(k2), None, None, 1, C.byref(gate), out.ctypes.data)

    rng = np.random.default_rng(1)
    kb = _kps(rng, 18000)                                                  # 9000 + 9000 features: a row extent above 16384
    big = osa.DeviceKeyFrame.from_host_fisheye(m, osa.FrameView(kb[:9000], rng.integers(0, 256, (18000, 32), dtype=np.uint8), *BOUNDS, SF), kb[9000:], ISG)
    assert frame_call(D, hs(a, b), 2) == 0 and nm[0] > 0
    before = m.last_transfers()
    refused = [
        # a monocular key frame: all five calls
        L.orbx_keyframe_compute_bow_fisheye(m._h, mono._h, ms.voc._h, 2, None, None),
        L.orbx_keyframe_bow_from_frame_fisheye(m._h, mono._h, Dm._h),
        frame_call(D, hs(a, mono), 2), kf_call(mono, hs(a), 1), kf_call(a, hs(mono), 1), tri(mono, a), tri(a, mono),
        frame_call(Dm, hs(a), 1),                                          # a monocular handle
        # a rig key frame without BoW
        frame_call(D, hs(a, bare), 2), kf_call(bare, hs(a), 1), kf_call(a, hs(bare), 1), tri(a, bare), tri(bare, a),
        # mixed vocabularies or levelsup values
        frame_call(D, hs(a, lv3), 2), frame_call(D, hs(foreign), 1), kf_call(a, hs(b, lv3), 2), kf_call(lv3, hs(b), 1), kf_call(a, hs(foreign), 1),
        tri(a, lv3), tri(a, foreign),
        # a level table of another length than the key frames', a missing one
        tri(a, b, _lib.KeyFrameKb8Gate(SG.ctypes.data, SG.ctypes.data, 7, (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 36)(), (C.c_float * 12)(), 0)),
        tri(a, b, _lib.KeyFrameKb8Gate(None, SG.ctypes.data, len(SG), (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 36)(), (C.c_float * 12)(), 0)),
        frame_call(D, (vp * 2)(), 2),                                      # NULL key frames
    ]
    assert refused == [BAD] * len(refused), refused
    # the calls of the monocular kind keep refusing a rig key frame
    assert L.orbx_keyframe_compute_bow(m._h, bare.dev._h, sc.voc._h, 2, None, None) == BAD
    assert L.orbx_keyframe_search_by_bow(m._h, a.dev._h, None, 1, hs(b), None, 0.75, 1, match.ctypes.data, N, nm.ctypes.data) == BAD
    assert L.orbx_frame_search_by_bow_resident(m._h, Dm._h, 1, hs(a), None, 0.75, 1, match.ctypes.data, N, nm.ctypes.data) == BAD
    # a row extent above 16384
    assert L.orbx_keyframe_compute_bow_fisheye(m._h, big._h, sc.voc._h, 2, None, None) == TOO_LARGE
    lots = (vp * (_lib.MAX_BOW_KEYFRAMES + 1))(*[a.dev._h.value] * (_lib.MAX_BOW_KEYFRAMES + 1))
    assert frame_call(D, lots, _lib.MAX_BOW_KEYFRAMES + 1) == TOO_LARGE and kf_call(a, lots, _lib.MAX_BOW_KEYFRAMES + 1) == TOO_LARGE
    assert m.last_transfers() == before                                    # nothing was enqueued by any refusal
    assert frame_call(D, hs(a), 1) == 0 and kf_call(a, hs(b), 1) == 0 and tri(a, b) >= 0   # the matcher still works
