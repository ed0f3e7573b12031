"""Frame::ComputeBoW, SearchByBoW(KeyFrame*, Frame&) and Relocalization's window search on a fisheye-stereo frame handle (orbx_frame_compute_bow_fisheye,
orbx_frame_search_by_bow_fisheye, orbx_frame_search_by_projection_window_fisheye).  Features [0, N_left) are the left camera's, [N_left, N) the right
one's.  Every result is compared bit for bit with the host-pointer forms (orbx_search_by_bow_frame_fisheye; orbx_search_by_projection_window over the
left camera) and the CPU oracle: the frame's FeatureVector is built here from the oracle's transform over all N rows with the stopped words dropped."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_frame_bow import _noisy
from test_gpu_frame_fisheye import SF, H, W, _extract_pairs, _kps, _left_view
from test_gpu_matcher import _random_vocabulary

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BAD = -2   # ORBX_E_BAD_ARG


class RigScene:
    """A rig frame (N_left + N_right features whose descriptors cluster around shared prototypes), a vocabulary whose node descriptors are sampled
    from them, word weights with stop words, and key frames related to the frame (noisy copies of features of both cameras) or not."""

    def __init__(self, seed, nl, nr, k=8, L=4, stop=0.1, ragged=True):
        import orb_slam3_amd as osa
        self.rng = rng = np.random.default_rng(seed)
        self.nl, self.nr, n = nl, nr, nl + nr
        self.kl, self.kr = _kps(rng, nl), _kps(rng, nr)
        protos = rng.integers(0, 256, (max(n // 3, 8), 32), dtype=np.uint8)
        self.d = _noisy(rng, protos[rng.integers(0, len(protos), n)], 0.12) if n else np.zeros((0, 32), np.uint8)
        self.angle = np.concatenate([self.kl["angle"], self.kr["angle"]]).astype(np.float32)
        self.cp, self.ci, nd, self.wi = _random_vocabulary(rng, k, L, ragged)
        src = np.concatenate([self.d, protos]) if n else protos
        self.nd = _noisy(rng, src[rng.integers(0, len(src), len(nd))], 0.05)
        self.L = L
        nw = int(self.wi.max()) + 1
        self.weights = rng.uniform(0.2, 3.0, nw)
        self.weights[rng.random(nw) < stop] = 0.0
        self.weights[rng.random(nw) < stop / 4] = -1.0
        self.voc = osa.ORBVocabulary(L, self.cp, self.ci, self.nd, self.wi).set_word_weights(self.weights)

    def handle(self, m, cap=None):
        import orb_slam3_amd as osa
        l2r, r2l = np.full(self.nl, -1, np.int32), np.full(self.nr, -1, np.int32)
        return osa.DeviceFrame(m, cap or max(1, self.nl + self.nr)).load_fisheye(_left_view(self.kl, self.d), self.kr, l2r, r2l)

    def transform(self, oracle, desc, levelsup):
        return oracle.bow_transform(self.cp, self.ci, self.nd, self.wi, self.L, levelsup, desc)

    def featvec(self, oracle, desc, levelsup):
        import orb_slam3_amd as osa
        w, node = self.transform(oracle, desc, levelsup)
        kept = np.nonzero(self.weights[w] > 0)[0] if len(w) else np.zeros(0, np.int64)
        nodes = np.unique(node[kept])
        return osa.FeatureVector(nodes, [kept[node[kept] == nd_] for nd_ in nodes])

    def keyframe(self, oracle, levelsup, related=True, n=None, valid_p=0.8):
        """related: copies of features of both cameras; the key frame's angles are what the adapter passes (mvKeysUn, or mvKeys / mvKeysRight of a
        fisheye key frame: a key frame of two halves, left copies then right copies)."""
        rng = self.rng
        n = int(rng.integers(150, 400)) if n is None else n
        N = len(self.d)
        if related and N:
            src = np.sort(rng.integers(0, N, n)) if rng.random() < 0.5 else rng.integers(0, N, n)
            d = _noisy(rng, self.d[src], 0.04)
            ang = np.mod(self.angle[src] + 25.0 + rng.normal(0, 3, n), 360).astype(np.float32)
            wild = rng.random(n) < 0.1
            ang[wild] = rng.uniform(0, 360, wild.sum()).astype(np.float32)
        else:
            d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            ang = rng.uniform(0, 360, n).astype(np.float32)
        valid = (rng.random(n) < valid_p).astype(np.uint8)
        return d, ang, valid, self.featvec(oracle, d, levelsup)


def _expected(oracle, sc, fv_f, kfs, ratio, ori):
    return [oracle.search_by_bow_frame_fisheye(d, a, v if v is not None else np.ones(len(d), np.uint8), fv, sc.d, sc.angle, sc.nl, fv_f, ratio, ori)
            for d, a, v, fv in kfs]


def _check_rows(oracle, m, sc, D, fv_f, kfs, ratio, ori, single=True):
    nm, match = m.SearchByBoWDeviceFisheye(D, kfs)
    assert nm.shape == (len(kfs),) and match.shape == (len(kfs), len(sc.d))
    for k, ((on, om), kf) in enumerate(zip(_expected(oracle, sc, fv_f, kfs, ratio, ori), kfs)):
        assert nm[k] == on and np.array_equal(match[k], om), (k, ratio, ori, nm[k], on)
        if single:
            d, a, v, fv = kf
            n1, fm1 = m.SearchByBoWFrameFisheye(d, a, v, fv, sc.d, sc.angle, sc.nl, fv_f)
            assert n1 == on and np.array_equal(fm1, om), (k, n1, on)
    return nm, match


@pytest.mark.parametrize("levelsup", [4, 2, 0])
@pytest.mark.parametrize("vocab", [(8, 4, True), (6, 5, True), (12, 3, False)])
def test_compute_bow_fisheye_equals_oracle_transform(oracle, levelsup, vocab):
    import orb_slam3_amd as osa
    k, L, ragged = vocab
    sc = RigScene(100 + 10 * k + levelsup, 500, 450, k, L, ragged=ragged)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m, 1200)
    w, node = D.compute_bow_fisheye(sc.voc, levelsup)
    ow, onode = sc.transform(oracle, sc.d, levelsup)
    assert np.array_equal(w, ow) and np.array_equal(node, onode)
    assert (sc.weights[w] <= 0).any() and (sc.weights[w] > 0).sum() > 500   # some features are stopped, most are not
    fv_f = sc.featvec(oracle, sc.d, levelsup)
    kf = sc.keyframe(oracle, levelsup)
    for ratio, ori in ((0.75, True), (0.9, True), (0.75, False)):
        m.mfNNratio, m.mbCheckOrientation = ratio, ori
        nm, match = _check_rows(oracle, m, sc, D, fv_f, [kf], ratio, ori)
        assert nm[0] > (5 if levelsup == 0 else 20), (ratio, ori, nm)   # (levelsup 0: leaf nodes, few candidates each)


@pytest.mark.parametrize("n_kf", [1, 7, 40])
def test_batches_of_candidates_equal_the_single_calls(oracle, n_kf):
    import orb_slam3_amd as osa
    sc = RigScene(200 + n_kf, 520, 480, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m)
    for levelsup in (2, 4):   # 4 = L: every feature in node 0, a node of 1000 frame features (the big-node path)
        D.compute_bow_fisheye(sc.voc, levelsup, download=False)
        fv_f = sc.featvec(oracle, sc.d, levelsup)
        if levelsup == 4:
            assert len(fv_f.node_id) == 1 and fv_f.node_ptr[-1] > 64
        kfs = [sc.keyframe(oracle, levelsup, related=(j % 3 != 1)) for j in range(n_kf)]
        if n_kf >= 7:
            d, a, v, fv = sc.keyframe(oracle, levelsup)
            kfs[2] = (d, a, v, osa.FeatureVector(fv.node_id + np.uint32(1 << 30), [fv.index[fv.node_ptr[i]:fv.node_ptr[i + 1]]
                                                                                    for i in range(len(fv.node_id))]))   # no common node
            d, a, v, _ = sc.keyframe(oracle, levelsup)
            kfs[3] = (d, a, v, osa.FeatureVector([], []))                          # an empty FeatureVector
            d, a, v, fv = sc.keyframe(oracle, levelsup)
            kfs[5] = (d, a, None, fv)                                              # valid = NULL: all
        for ratio, ori in ((0.75, True), (0.7, False)):
            m.mfNNratio, m.mbCheckOrientation = ratio, ori
            nm, match = _check_rows(oracle, m, sc, D, fv_f, kfs, ratio, ori, single=(n_kf < 40))
            related = [k for k in range(n_kf) if k % 3 != 1 and not (n_kf >= 7 and k in (2, 3))]
            assert min(nm[related]) > 20, nm
            assert (match[related][:, :sc.nl] >= 0).any() and (match[related][:, sc.nl:] >= 0).any()   # matches on both cameras
            if n_kf >= 7:
                assert nm[2] == nm[3] == 0
    nm, match = m.SearchByBoWDeviceFisheye(D, [])
    assert nm.shape == (0,) and match.shape == (0, 1000)


@pytest.mark.parametrize("nl,nr", [(600, 0), (0, 600), (0, 0)])
def test_one_camera_or_empty(oracle, nl, nr):
    import orb_slam3_amd as osa
    sc = RigScene(300 + nl, nl, nr, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m, 700)
    w, node = D.compute_bow_fisheye(sc.voc, 2)
    ow, onode = sc.transform(oracle, sc.d, 2)
    assert np.array_equal(w, ow) and np.array_equal(node, onode)
    fv_f = sc.featvec(oracle, sc.d, 2)
    other = RigScene(399, 300, 0)
    kfs = [sc.keyframe(oracle, 2) if nl + nr else other.keyframe(oracle, 2), sc.keyframe(oracle, 2, related=False)]
    nm, match = _check_rows(oracle, m, sc, D, fv_f, kfs, 0.75, True)
    assert match.shape == (2, nl + nr)
    if nl:
        assert nm[0] > 20
    else:   # no left feature: the right camera is looked at only inside the left camera's bestDist1 <= TH_LOW branch (ORBmatcher.cc:318-377)
        assert list(nm) == [0, 0]


def test_stop_words_empty_whole_nodes(oracle):
    import orb_slam3_amd as osa
    sc = RigScene(410, 500, 500, 6, 4, stop=0.6)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m)
    w, node = D.compute_bow_fisheye(sc.voc, 2)
    ow, onode = sc.transform(oracle, sc.d, 2)
    assert np.array_equal(w, ow) and np.array_equal(node, onode)
    kept = sc.weights[w] > 0
    gone = set(node.tolist()) - set(node[kept].tolist())
    assert gone and kept.sum() > 100, (len(gone), kept.sum())   # whole nodes vanish from the FeatureVector
    fv_f = sc.featvec(oracle, sc.d, 2)
    kfs = [sc.keyframe(oracle, 2, n=600) for _ in range(5)]
    nm, _ = _check_rows(oracle, m, sc, D, fv_f, kfs, 0.75, True)
    assert nm.min() > 5


def _window_queries(rng, kl, desc, n_q, th):
    src = rng.integers(0, len(kl), n_q)
    lvl = kl["octave"][src]
    return dict(x=kl["x"][src] + rng.normal(0, 2.0, n_q).astype(np.float32), y=kl["y"][src] - 1.0,
                angle=np.mod(kl["angle"][src] + 30.0, 360).astype(np.float32), desc=_noisy(rng, desc[src], 0.08),
                r=(th * SF[lvl]).astype(np.float32), min_level=lvl - 1, max_level=lvl + 1)


def test_window_search_covers_the_left_camera_only(oracle):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(9)
    sc = RigScene(420, 900, 800)
    nl, N = sc.nl, len(sc.d)
    m = osa.ORBmatcher(0.75, True)
    D = sc.handle(m, 2000)
    F = osa.FrameView(sc.kl, sc.d[:nl], 0.0, float(W), 0.0, float(H), SF)   # the left view: N = N_left, mvKeys
    grid = oracle.OracleGrid(sc.kl, 0.0, float(W), 0.0, float(H))
    occ = (rng.random(N) < 0.1).astype(np.uint8)
    for th, orbdist in ((10.0, 100.0), (3.0, 64.0)):   # Tracking.cc:3726,3740
        q = _window_queries(rng, sc.kl, sc.d, 600, th)
        on, om = oracle.search_by_projection_window(grid, sc.d[:nl], q, orbdist, True, False, occ[:nl])
        n1, m1 = m.SearchByProjectionWindow(F, q, orbdist, True, occ[:nl], raw=True)
        n2, m2 = m.SearchByProjectionWindowFisheye(D, q, orbdist, True, occ, raw=True)
        assert m2.shape == (N,) and (m2[nl:] == -1).all()
        assert n1 == n2 == on and np.array_equal(m1, m2[:nl]) and np.array_equal(np.maximum(m2[:nl], -1), om), (th, n1, n2, on)
        assert on > 100
        n3, m3 = m.SearchByProjectionWindowFisheye(D, q, orbdist, True, None, raw=True)   # no mask
        n4, m4 = m.SearchByProjectionWindow(F, q, orbdist, True, None, raw=True)
        assert n3 == n4 and np.array_equal(m3[:nl], m4) and (m3[nl:] == -1).all()


def test_batch_loaded_frame_equals_the_host_loaded_handle(oracle):
    """load_stereo_fisheye_batch -> compute_bow_fisheye(download=False) -> SearchByBoWDeviceFisheye: the counts are never read before the search, the
    right rows sit at the left extractor's capacity (a gap behind N_left).  Equal to the host-loaded handle of the same frame and to the oracle."""
    import orb_slam3_amd as osa
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    w = h = 512
    nb, nf = 4, 1000
    left, right = _extract_pairs(w, h, nb, nf)
    fs = w * h
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    exl.extract_batch_device(left.data_ptr(), nb, w, h, w, fs, (0, 0))
    exr.extract_batch_device(right.data_ptr(), nb, w, h, w, fs, (0, 0))
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    capl, capr = exl.batch_view().cap, exr.batch_view().cap
    sf = exl.GetScaleFactors().astype(np.float32)
    bounds = (0.0, float(w), 0.0, float(h))
    outs_l = [exl.download(t) for t in range(nb)]
    outs_r = [exr.download(t) for t in range(nb)]
    _, _, l2r, r2l, _, _ = exl.stereo_fisheye_download(3)
    rng = np.random.default_rng(5)
    cp, ci, nd, wi = _random_vocabulary(rng, 10, 4)
    pool = np.concatenate([o[2] for o in outs_l + outs_r])
    nd = _noisy(rng, pool[rng.integers(0, len(pool), len(nd))], 0.03)
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.05] = 0.0
    voc = osa.ORBVocabulary(4, cp, ci, nd, wi).set_word_weights(weights)

    def fv(desc, levelsup=2):
        wd, node = oracle.bow_transform(cp, ci, nd, wi, 4, levelsup, desc)
        kept = np.nonzero(weights[wd] > 0)[0]
        nodes = np.unique(node[kept])
        return osa.FeatureVector(nodes, [kept[node[kept] == x] for x in nodes])

    _, kl, dl = outs_l[3]
    _, kr, dr = outs_r[3]
    nl = len(kl)
    assert capl > nl and len(kr) > 0   # a gap between N_left and the right rows
    desc = np.concatenate([dl, dr]).reshape(-1, 32)
    angle = np.concatenate([kl["angle"], kr["angle"]]).astype(np.float32)
    kfs = []
    for t in range(3):   # fisheye key frames: both cameras' rows, angles from mvKeys / mvKeysRight
        kd = np.concatenate([outs_l[t][2], outs_r[t][2]]).reshape(-1, 32)
        ka = np.concatenate([outs_l[t][1]["angle"], outs_r[t][1]["angle"]]).astype(np.float32)
        kfs.append((kd, ka, (rng.random(len(kd)) < 0.8).astype(np.uint8), fv(kd)))
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, 3, bounds=bounds, scale_factors=sf)
    assert D.compute_bow_fisheye(voc, 2, download=False) is None
    nm, match = m.SearchByBoWDeviceFisheye(D, kfs)
    assert D.counts() == (nl, len(kr))
    fv_c = fv(desc)
    for k, (d, a, v, f) in enumerate(kfs):
        on, om = oracle.search_by_bow_frame_fisheye(d, a, v, f, desc, angle, nl, fv_c, 0.75, True)
        assert nm[k] == on and np.array_equal(match[k], om), (k, nm[k], on)
        assert on > 50 and (om[nl:] >= 0).any()
    # the same frame loaded from the host: same ids, same rows
    Hh = osa.DeviceFrame(m, capl + capr).load_fisheye(osa.FrameView(kl, desc, 0.0, float(w), 0.0, float(h), sf), kr, l2r, r2l)
    wd, node = Hh.compute_bow_fisheye(voc, 2)
    assert np.array_equal(node, oracle.bow_transform(cp, ci, nd, wi, 4, 2, desc)[1])
    nm2, match2 = m.SearchByBoWDeviceFisheye(Hh, kfs)
    assert np.array_equal(nm, nm2) and np.array_equal(match, match2)
    # downloads while the counts are still on the device: a fresh load, ids straight after it
    D2 = osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, 3, bounds=bounds, scale_factors=sf)
    wd2, node2 = D2.compute_bow_fisheye(voc, 2)
    assert np.array_equal(wd2, wd) and np.array_equal(node2, node)
    # the window search on a fresh batch load (N_left read on the device) equals the host-loaded handle's
    D3 = osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, 3, bounds=bounds, scale_factors=sf)
    q = _window_queries(rng, kl, desc, 500, 10.0)
    n3, m3 = m.SearchByProjectionWindowFisheye(D3, q, 100.0, True, None, raw=True)
    n4, m4 = m.SearchByProjectionWindowFisheye(Hh, q, 100.0, True, None, raw=True)
    assert D3.counts() == (nl, len(kr))
    assert n3 == n4 and np.array_equal(m3, m4) and n3 > 50 and (m3[nl:] == -1).all()


def test_refusals(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    sc = RigScene(430, 300, 250)
    m, m2 = osa.ORBmatcher(0.75, True), osa.ORBmatcher(0.75, True)
    D = sc.handle(m)
    Mo = osa.DeviceFrame(m, 600).load(osa.FrameView(sc.kl, sc.d[:300], 0.0, float(W), 0.0, float(H), SF))
    kf = sc.keyframe(oracle, 2)
    q = _window_queries(np.random.default_rng(1), sc.kl, sc.d, 50, 10.0)
    with pytest.raises(_lib.OrbxError):
        m.SearchByBoWDeviceFisheye(D, [kf])                   # no compute_bow_fisheye yet
    with pytest.raises(_lib.OrbxError):
        Mo.compute_bow_fisheye(sc.voc, 2)                      # a monocular handle
    Mo.compute_bow(sc.voc, 2, download=False)
    for call in (lambda: m.SearchByBoWDeviceFisheye(Mo, [kf]), lambda: m.SearchByProjectionWindowFisheye(Mo, q, 100.0, True),
                 lambda: m2.SearchByProjectionWindowFisheye(D, q, 100.0, True)):
        with pytest.raises(_lib.OrbxError):
            call()
    assert L.orbx_frame_compute_bow_fisheye(m2._h, D._h, sc.voc._h, 2, None, None) == BAD   # a handle of another matcher
    assert L.orbx_frame_compute_bow_fisheye(m._h, D._h, None, 2, None, None) == BAD
    D.compute_bow_fisheye(sc.voc, 2, download=False)
    nm, _ = m.SearchByBoWDeviceFisheye(D, [kf])
    assert nm[0] > 20
    with pytest.raises(_lib.OrbxError):
        m2.SearchByBoWDeviceFisheye(D, [kf])                  # foreign handle
    with pytest.raises(_lib.OrbxError):
        m.SearchByBoWDevice(D, [kf])                          # the monocular form still refuses a fisheye handle
    with pytest.raises(_lib.OrbxError):
        m.SearchByBoWDeviceFisheye(D, [kf] * (_lib.MAX_BOW_KEYFRAMES + 1))
    D.load_fisheye(_left_view(sc.kl, sc.d), sc.kr, np.full(300, -1, np.int32), np.full(250, -1, np.int32))   # a reload clears the BoW state
    with pytest.raises(_lib.OrbxError):
        m.SearchByBoWDeviceFisheye(D, [kf])
    assert L.orbx_frame_search_by_bow_fisheye(m._h, D._h, 0, None, 0.75, 1, None, 600, None) == BAD   # before n_kf == 0
    D.compute_bow_fisheye(sc.voc, 2, download=False)
    nm2, _ = m.SearchByBoWDeviceFisheye(D, [kf])              # the matcher and the handle are still usable
    assert nm2[0] == nm[0]


@pytest.mark.skipif(bool(os.environ.get("ORBX_TEST_EMULATOR")), reason="runs a separately built program")
def test_cpp_device_frame_bow_fisheye_equals_python(oracle, tmp_path):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    exe = tmp_path / "frame_bow_fisheye_demo"
    r = subprocess.run(["g++", "-std=c++17", "-O1", str(ROOT / "tests/cpp/frame_bow_fisheye_demo.cpp"), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    sc = RigScene(500, 450, 400)
    kfs = [sc.keyframe(oracle, 2) for _ in range(3)]
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([sc.L, len(sc.wi), len(sc.ci), len(sc.weights), sc.nl, sc.nr, len(kfs)], np.int32).tobytes())
        f.write(sc.cp.tobytes() + sc.ci.tobytes() + sc.nd.tobytes() + sc.wi.tobytes() + sc.weights.astype(np.float64).tobytes())
        f.write(sc.kl.tobytes() + sc.kr.tobytes() + sc.d.tobytes())
        for d, a, v, fv in kfs:
            f.write(np.array([len(d), len(fv.node_id)], np.int32).tobytes())
            f.write(d.tobytes() + a.astype(np.float32).tobytes() + v.tobytes() + fv.node_id.tobytes() + fv.node_ptr.tobytes() + fv.index.tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = str(Path(torch.__file__).parent / "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(out, np.int32)
    n = len(sc.d)
    assert len(raw) == 2 * n + len(kfs) * (1 + n)
    ow, onode = sc.transform(oracle, sc.d, 2)
    assert np.array_equal(raw[:n], ow) and np.array_equal(raw[n:2 * n], onode)
    fv_f = sc.featvec(oracle, sc.d, 2)
    o = 2 * n
    for k, (on, om) in enumerate(_expected(oracle, sc, fv_f, kfs, 0.75, True)):
        assert raw[o] == on and np.array_equal(raw[o + 1:o + 1 + n], om), k
        assert on > 20
        o += 1 + n
