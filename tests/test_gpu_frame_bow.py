"""Frame::ComputeBoW and SearchByBoW(KeyFrame*, Frame&) on the device-resident frame (orbx_frame_compute_bow / orbx_frame_search_by_bow), and the
window matcher's handle form.  Every result is compared bit for bit with the host-pointer entry points and the CPU oracle: the frame's FeatureVector
is built here from the oracle's transform with the stopped features dropped, row k of a batch against orbx_search_by_bow_frame for key frame k."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_matcher import _random_vocabulary

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = 752, 480
SF = np.array([1.2 ** i for i in range(8)], np.float32)
BAD = -2


def _noisy(rng, d, p):
    return d ^ np.packbits(rng.random((len(d), 256)) < p, axis=1, bitorder="little")


def _keypoints(rng, n):
    import orb_slam3_amd as osa
    k = np.zeros(n, osa.KP_DTYPE)
    k["octave"] = rng.integers(0, 8, n)
    sc = (1.2 ** k["octave"]).astype(np.float32)
    k["x"] = (rng.uniform(20, W - 20, n) / sc).round().astype(np.float32) * sc
    k["y"] = (rng.uniform(20, H - 20, n) / sc).round().astype(np.float32) * sc
    k["size"] = 31.0 * sc
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.integers(7, 200, n).astype(np.float32)
    k["class_id"] = -1
    return k


class Scene:
    """A current frame, a vocabulary whose node descriptors are sampled from the frame's descriptors (true correspondences share nodes), word
    weights with some stop words, and key frames that are related to the frame (noisy copies of a subset, rotated by ~25 degrees) or not."""

    def __init__(self, seed, n, k=8, L=4, stop=0.1, ragged=True):
        import orb_slam3_amd as osa
        self.rng = rng = np.random.default_rng(seed)
        self.k = _keypoints(rng, n)
        protos = rng.integers(0, 256, (max(n // 3, 8), 32), dtype=np.uint8)
        self.d = _noisy(rng, protos[rng.integers(0, len(protos), n)], 0.12) if n else np.zeros((0, 32), np.uint8)
        self.cp, self.ci, nd, self.wi = _random_vocabulary(rng, k, L, ragged)
        src = np.concatenate([self.d, protos]) if n else protos
        self.nd = _noisy(rng, src[rng.integers(0, len(src), len(nd))], 0.05)
        self.L = L
        nw = int(self.wi.max()) + 1
        self.weights = rng.uniform(0.2, 3.0, nw)
        self.weights[rng.random(nw) < stop] = 0.0
        self.weights[rng.random(nw) < stop / 4] = -1.0
        self.voc = osa.ORBVocabulary(L, self.cp, self.ci, self.nd, self.wi).set_word_weights(self.weights)
        self.F = osa.FrameView(self.k, self.d, 0.0, float(W), 0.0, float(H), SF)

    def transform(self, oracle, desc, levelsup):
        return oracle.bow_transform(self.cp, self.ci, self.nd, self.wi, self.L, levelsup, desc)

    def featvec(self, oracle, desc, levelsup):
        import orb_slam3_amd as osa
        w, node = self.transform(oracle, desc, levelsup)
        kept = np.nonzero(self.weights[w] > 0)[0] if len(w) else np.zeros(0, np.int64)
        nodes = np.unique(node[kept])
        return osa.FeatureVector(nodes, [kept[node[kept] == nd_] for nd_ in nodes])

    def keyframe(self, oracle, levelsup, related=True, n=None, valid_p=0.8):
        rng = self.rng
        n = int(rng.integers(150, 400)) if n is None else n
        if related and len(self.d):
            src = rng.integers(0, len(self.d), n)
            d = _noisy(rng, self.d[src], 0.04)
            ang = np.mod(self.k["angle"][src] + 25.0 + rng.normal(0, 3, n), 360).astype(np.float32)
            wild = rng.random(n) < 0.1
            ang[wild] = rng.uniform(0, 360, wild.sum()).astype(np.float32)
        else:
            d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            ang = rng.uniform(0, 360, n).astype(np.float32)
        valid = (rng.random(n) < valid_p).astype(np.uint8)
        return d, ang, valid, self.featvec(oracle, d, levelsup)


def _expected(oracle, sc, fv_f, kfs, ratio, ori):
    return [oracle.search_by_bow_frame(d, a, v if v is not None else np.ones(len(d), np.uint8), fv, sc.d, sc.k["angle"], fv_f, ratio, ori)
            for d, a, v, fv in kfs]


def _check_rows(oracle, m, sc, D, fv_f, kfs, ratio, ori, single=True):
    nm, match = m.SearchByBoWDevice(D, kfs)
    assert nm.shape == (len(kfs),) and match.shape == (len(kfs), len(sc.d))
    for k, ((on, om), kf) in enumerate(zip(_expected(oracle, sc, fv_f, kfs, ratio, ori), kfs)):
        assert nm[k] == on and np.array_equal(match[k], om), (k, ratio, ori, nm[k], on)
        if single:
            d, a, v, fv = kf
            n1, fm1 = m.SearchByBoWFrame(d, a, v, fv, sc.d, sc.k["angle"], fv_f)
            assert n1 == on and np.array_equal(fm1, om), (k, n1, on)
    return nm


@pytest.mark.parametrize("levelsup", [4, 2, 0])
@pytest.mark.parametrize("vocab", [(8, 4, True), (6, 5, True), (12, 3, False)])
def test_compute_bow_and_single_keyframe_equal_host_forms_and_oracle(oracle, levelsup, vocab):
    import orb_slam3_amd as osa
    k, L, ragged = vocab
    sc = Scene(100 + 10 * k + levelsup, 900, k, L, ragged=ragged)
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 1200).load(sc.F)
    w, node = D.compute_bow(sc.voc, levelsup)
    ow, onode = sc.transform(oracle, sc.d, levelsup)
    assert np.array_equal(w, ow) and np.array_equal(node, onode)
    assert (sc.weights[w] <= 0).any() and (sc.weights[w] > 0).sum() > 500   # some features are stopped, most are not
    fv_f = sc.featvec(oracle, sc.d, levelsup)
    kf = sc.keyframe(oracle, levelsup)
    for ratio, ori in ((0.7, True), (0.75, True), (0.9, True), (0.75, False)):
        m.mfNNratio, m.mbCheckOrientation = ratio, ori
        nm = _check_rows(oracle, m, sc, D, fv_f, [kf], ratio, ori)
        assert nm[0] > 20, (ratio, ori, nm)


@pytest.mark.parametrize("n_kf", [1, 7, 40])
def test_batches_of_candidates_equal_the_single_calls(oracle, n_kf):
    import orb_slam3_amd as osa
    sc = Scene(200 + n_kf, 1000, 8, 4)
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 1000).load(sc.F)
    for levelsup in (2, 4):   # 4 = L: every feature in node 0, a node of 1000 frame features (the big-node path)
        D.compute_bow(sc.voc, levelsup, download=False)
        fv_f = sc.featvec(oracle, sc.d, levelsup)
        if levelsup == 4:
            assert len(fv_f.node_id) == 1 and fv_f.node_ptr[-1] > 64
        kfs = []
        for j in range(n_kf):
            kfs.append(sc.keyframe(oracle, levelsup, related=(j % 3 != 1)))
        if n_kf >= 7:
            d, a, v, fv = sc.keyframe(oracle, levelsup)
            kfs[2] = (d, a, v, osa.FeatureVector(fv.node_id + np.uint32(1 << 30), [fv.index[fv.node_ptr[i]:fv.node_ptr[i + 1]]
                                                                                    for i in range(len(fv.node_id))]))   # no common node
            d, a, v, _ = sc.keyframe(oracle, levelsup)
            kfs[3] = (d, a, v, osa.FeatureVector([], []))                          # an empty FeatureVector
            d, a, v, fv = sc.keyframe(oracle, levelsup)
            kfs[4] = (d, a, np.zeros(len(d), np.uint8), fv)                        # no valid map point
            d, a, v, fv = sc.keyframe(oracle, levelsup)
            kfs[5] = (d, a, None, fv)                                              # valid = NULL: all
        for ratio, ori in ((0.75, True), (0.7, False)):
            m.mfNNratio, m.mbCheckOrientation = ratio, ori
            nm = _check_rows(oracle, m, sc, D, fv_f, kfs, ratio, ori, single=(n_kf < 40))
            related = [k for k in range(n_kf) if k % 3 != 1 and not (n_kf >= 7 and 2 <= k <= 4)]
            assert min(nm[related]) > 20, nm
            if n_kf >= 7:
                assert nm[2] == nm[3] == nm[4] == 0
    nm, match = m.SearchByBoWDevice(D, [])
    assert nm.shape == (0,) and match.shape == (0, 1000)


def test_empty_and_full_frames(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    m = osa.ORBmatcher(0.75, True)
    sc = Scene(300, 0)
    D = osa.DeviceFrame(m, 100).load(sc.F)
    w, node = D.compute_bow(sc.voc, 2)
    assert len(w) == len(node) == 0
    kf = Scene(301, 300).keyframe(oracle, 2, related=False)
    nm, match = m.SearchByBoWDevice(D, [kf, kf])
    assert list(nm) == [0, 0] and match.shape == (2, 0)
    cap = 16000
    sc = Scene(302, cap, 10, 4)
    D = osa.DeviceFrame(m, cap).load(sc.F)
    w, node = D.compute_bow(sc.voc, 2)
    ow, onode = sc.transform(oracle, sc.d, 2)
    assert np.array_equal(w, ow) and np.array_equal(node, onode)
    fv_f = sc.featvec(oracle, sc.d, 2)
    nm = _check_rows(oracle, m, sc, D, fv_f, [sc.keyframe(oracle, 2, n=2000), sc.keyframe(oracle, 2, related=False)], 0.75, True, single=False)
    assert nm[0] > 100


def _batch(canvas, nfr=4):
    import torch
    from orb_slam3_amd import synth
    frames = np.stack([synth.frame_from_canvas(canvas, t, W, H, 1000 + t) for t in range(nfr)])
    return torch.from_numpy(frames).cuda()


def test_chain_from_a_batch_without_host_synchronisation(oracle, canvas1):
    """load_batch -> compute_bow(download=False) -> SearchByBoWDevice: N is never counted before the search, nothing of the frame is uploaded."""
    import orb_slam3_amd as osa
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    d_frames = _batch(canvas1)
    ex.extract_batch_device(d_frames.data_ptr(), 4, W, H, W, W * H, (0, 1000))
    outs = [ex.download(t) for t in range(4)]
    cap = ex.batch_view().cap
    rng = np.random.default_rng(5)
    cp, ci, nd, wi = _random_vocabulary(rng, 10, 4)
    pool = np.concatenate([o[2] for o in outs])
    nd = _noisy(rng, pool[rng.integers(0, len(pool), len(nd))], 0.03)
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.05] = 0.0
    voc = osa.ORBVocabulary(4, cp, ci, nd, wi).set_word_weights(weights)

    def fv(desc, levelsup=2):
        w, node = oracle.bow_transform(cp, ci, nd, wi, 4, levelsup, desc)
        kept = np.nonzero(weights[w] > 0)[0]
        nodes = np.unique(node[kept])
        return osa.FeatureVector(nodes, [kept[node[kept] == x] for x in nodes])

    _, kc, dc = outs[3]
    kfs = [(outs[t][2], outs[t][1]["angle"], (rng.random(len(outs[t][1])) < 0.8).astype(np.uint8), fv(outs[t][2])) for t in range(3)]
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, cap).load_batch(ex, 3)
    assert D.compute_bow(voc, 2, download=False) is None
    nm, match = m.SearchByBoWDevice(D, kfs)
    t_batch = m.last_transfers()
    assert D.count() == len(kc)
    fv_c = fv(dc)
    for k, (d, a, v, f) in enumerate(kfs):
        on, om = oracle.search_by_bow_frame(d, a, v, f, dc, kc["angle"], fv_c, 0.75, True)
        assert nm[k] == on and np.array_equal(match[k], om), (k, nm[k], on)
        assert on > 50
    # the same frame loaded from the host: same results, and the same uploads (the key frames only)
    H_ = osa.DeviceFrame(m, cap).load(osa.FrameView(kc, dc, 0.0, float(W), 0.0, float(H), ex.GetScaleFactors()))
    w, node = H_.compute_bow(voc, 2)
    assert np.array_equal(node, oracle.bow_transform(cp, ci, nd, wi, 4, 2, dc)[1])
    nm2, match2 = m.SearchByBoWDevice(H_, kfs)
    assert np.array_equal(nm, nm2) and np.array_equal(match, match2)
    t_host = m.last_transfers()
    kf_bytes = sum(33 * len(d) + 4 * len(d) for d, _, _, _ in kfs)
    assert t_batch["upload_bytes"] == t_host["upload_bytes"] and t_batch["upload_bytes"] < kf_bytes + 32 * 1024, (t_batch, kf_bytes)
    assert t_batch["uploads"] == 1 and t_batch["downloads"] <= 2, t_batch


def test_window_handle_form_equals_host_form_and_oracle(oracle):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(9)
    n = 1200
    k = _keypoints(rng, n)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    F = osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), SF)
    grid = oracle.OracleGrid(k, 0.0, float(W), 0.0, float(H))
    m = osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 2000).load(F)
    src = rng.integers(0, n, 700)
    lvl = k["octave"][src]
    occ = (rng.random(n) < 0.1).astype(np.uint8)
    base = dict(x=k["x"][src] + rng.normal(0, 2.0, len(src)).astype(np.float32), y=k["y"][src] - 1.0,
                angle=np.mod(k["angle"][src] + 30.0, 360).astype(np.float32), desc=_noisy(rng, d[src], 0.08))
    for th, orbdist in ((10.0, 100.0), (3.0, 64.0)):   # Tracking.cc:3726,3740
        q = dict(base, r=(th * SF[lvl]).astype(np.float32), min_level=lvl - 1, max_level=lvl + 1)
        on, om = oracle.search_by_projection_window(grid, d, q, orbdist, True, False, occ)
        n1, m1 = m.SearchByProjectionWindow(F, q, orbdist, True, occ, raw=True)
        n2, m2 = m.SearchByProjectionWindow(D, q, orbdist, True, occ, raw=True)
        assert n1 == n2 == on and np.array_equal(m1, m2) and np.array_equal(np.maximum(m2, -1), om), (th, n1, n2, on)
        assert on > 100
        t = m.last_transfers()
        assert t["upload_bytes"] < 32 * n + 64 * len(src), t


def test_errors_before_anything_is_enqueued(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    sc = Scene(400, 500)
    m, m2 = osa.ORBmatcher(0.75, True), osa.ORBmatcher(0.75, True)
    D = osa.DeviceFrame(m, 500).load(sc.F)
    kf = sc.keyframe(oracle, 2)
    with pytest.raises(RuntimeError):
        m.SearchByBoWDevice(D, [kf])                          # no compute_bow yet
    assert L.orbx_frame_compute_bow(m2._h, D._h, sc.voc._h, 2, None, None) == BAD   # a handle of another matcher
    assert L.orbx_frame_compute_bow(m._h, D._h, None, 2, None, None) == BAD
    D.compute_bow(sc.voc, 2, download=False)
    nm, _ = m.SearchByBoWDevice(D, [kf])
    assert nm[0] > 20
    with pytest.raises(RuntimeError):
        m2.SearchByBoWDevice(D, [kf])                         # foreign handle
    D.load(sc.F)                                              # a reload clears the BoW state
    with pytest.raises(RuntimeError):
        m.SearchByBoWDevice(D, [kf])
    D.compute_bow(sc.voc, 2, download=False)
    big = [kf] * (_lib.MAX_BOW_KEYFRAMES + 1)
    with pytest.raises(RuntimeError):
        m.SearchByBoWDevice(D, big)                           # n_kf above ORBX_MAX_BOW_KEYFRAMES
    d, a, v, fv = kf
    bad_fv = osa.FeatureVector.__new__(osa.FeatureVector)
    bad_fv.node_id, bad_fv.node_ptr, bad_fv.index = fv.node_id, fv.node_ptr, fv.index.copy()
    bad_fv.index[0] = len(d)                                  # an index past the key frame's features
    with pytest.raises(RuntimeError):
        m.SearchByBoWDevice(D, [kf, (d, a, v, bad_fv)])
    with pytest.raises(RuntimeError):
        sc.voc.set_word_weights(sc.weights[:-1])              # a word id without a weight
    nm2, _ = m.SearchByBoWDevice(D, [kf])                     # the handle is still usable
    assert nm2[0] == nm[0]
    import torch
    if torch.cuda.device_count() > 1 and not os.environ.get("ORBX_TEST_EMULATOR"):
        v1 = osa.ORBVocabulary(sc.L, sc.cp, sc.ci, sc.nd, sc.wi, device=1)
        assert L.orbx_frame_compute_bow(m._h, D._h, v1._h, 2, None, None) == BAD   # a vocabulary on another device


@pytest.mark.skipif(bool(os.environ.get("ORBX_TEST_EMULATOR")), reason="runs a separately built program")
def test_cpp_device_frame_bow_equals_python(oracle, tmp_path):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    exe = tmp_path / "frame_bow_demo"
    r = subprocess.run(["g++", "-std=c++17", "-O1", str(ROOT / "tests/cpp/frame_bow_demo.cpp"), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    sc = Scene(500, 800)
    kfs = [sc.keyframe(oracle, 2) for _ in range(3)]
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([sc.L, len(sc.wi), len(sc.ci), len(sc.weights), len(sc.d), len(kfs)], np.int32).tobytes())
        f.write(sc.cp.tobytes() + sc.ci.tobytes() + sc.nd.tobytes() + sc.wi.tobytes() + sc.weights.astype(np.float64).tobytes())
        f.write(sc.k.tobytes() + sc.d.tobytes())
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
