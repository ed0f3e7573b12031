"""The device-resident frame handle (orbx_frame / DeviceFrame): load a frame once, search it many times.  Every result is compared bit for bit
with the host-pointer forms and the CPU oracle.  The host-pointer forms take the grid-less k_window_brute path for small problems while the
handle always searches through its resident grid, so the small scenes here compare the two paths directly."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 752, 480
SF = np.array([1.2 ** i for i in range(8)], np.float32)
EUROC4 = (458.654, 457.296, 367.215, 248.375)


def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _noisy(rng, d, p):
    return d ^ np.packbits(rng.random((len(d), 256)) < p, axis=1, bitorder="little")


def _frame(rng, n, w=W, h=H, packed=False):
    import orb_slam3_amd as osa
    k = np.zeros(n, osa.KP_DTYPE)
    k["octave"] = rng.integers(0, 3 if packed else 8, n)
    sc = (1.2 ** k["octave"]).astype(np.float32)
    if packed:   # a few hundred features in a small region: long contention chains
        k["x"] = rng.uniform(300, 380, n).astype(np.float32)
        k["y"] = rng.uniform(200, 260, n).astype(np.float32)
    else:
        k["x"] = (rng.uniform(20, w - 20, n) / sc).round().astype(np.float32) * sc
        k["y"] = (rng.uniform(20, h - 20, n) / sc).round().astype(np.float32) * sc
    k["size"] = 31.0 * sc
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.integers(7, 200, n).astype(np.float32)
    k["class_id"] = -1
    if packed:
        protos = _rand_desc(rng, 6)
        return k, _noisy(rng, protos[rng.integers(0, 6, n)], 0.08)
    return k, _rand_desc(rng, n)


def _u_right(rng, k):
    ur = (k["x"] - rng.uniform(2, 40, len(k))).astype(np.float32)
    ur[rng.random(len(k)) < 0.3] = -1.0
    return ur


def _mp(rng, k, d, n_mp, noise, ur=None):
    src = rng.integers(0, len(k), n_mp)
    px = k["x"][src] + rng.normal(0, noise, n_mp).astype(np.float32)
    pxr = (px - (k["x"][src] - ur[src]) + rng.normal(0, 1.0, n_mp).astype(np.float32)) if ur is not None else np.zeros(n_mp, np.float32)
    level = k["octave"][src].copy()
    level[rng.random(n_mp) < 0.02] = 9            # out of the frame's levels: skipped
    return dict(proj_x=px, proj_y=k["y"][src] + rng.normal(0, noise, n_mp).astype(np.float32), proj_xr=pxr.astype(np.float32), level=level,
                view_cos=rng.choice(np.array([0.9, 0.998, np.nextafter(np.float32(0.998), np.float32(1)), 0.9995, 1.0], np.float32), n_mp),
                desc=_noisy(rng, d[src], 0.05), in_view=(rng.random(n_mp) < 0.95).astype(np.uint8),
                has_obs=(rng.random(n_mp) < 0.9).astype(np.uint8)), src


def _queries(rng, k, d, src, ur=None):
    n = len(src)
    u = k["x"][src] + 1.0
    return dict(u=u, v=k["y"][src] - 1.0, ur=(u - (k["x"][src] - ur[src])) if ur is not None else np.zeros(n, np.float32),
                octave=k["octave"][src], angle=k["angle"][src], desc=_noisy(rng, d[src], 0.05), has_obs=(rng.random(n) < 0.85).astype(np.uint8))


# (frame size, map points / queries, packed) -- small problems (host form: k_window_brute), the contention scenes and a grid-sized one
SCENES = [(150, 60, False), (1000, 700, False), (400, 2500, True), (500, 2500, True), (1500, 10000, False)]


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("scene", range(len(SCENES)))
def test_host_load_m1_m2_equal_host_pointer_forms_and_oracle(oracle, scene, stereo):
    import orb_slam3_amd as osa
    N, nq, packed = SCENES[scene]
    rng = np.random.default_rng(1000 + 10 * scene + stereo)
    k, d = _frame(rng, N, packed=packed)
    ur = _u_right(rng, k) if stereo else None
    F = osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), SF, ur)
    grid = oracle.OracleGrid(k, 0.0, float(W), 0.0, float(H))
    m = osa.ORBmatcher(0.9, True)
    D = osa.DeviceFrame(m, N).load(F)
    assert D.count() == N
    occ = (rng.random(N) < 0.05).astype(np.uint8)
    mp, src = _mp(rng, k, d, nq, 3.0 if packed else 2.0, ur)
    for th in (1.0, 3.0, 8.0):
        on, ofm = oracle.search_by_projection_mappoints(grid, d, SF, mp, th, 0.9, ur, occ)
        n1, fm1 = m.SearchByProjection(F, mp, th, occ)
        n2, fm2 = m.SearchByProjection(D, mp, th, occ)
        assert n1 == n2 == on and np.array_equal(fm1, ofm) and np.array_equal(fm2, ofm), (th, n1, n2, on)
    assert on > 0
    q = _queries(rng, k, d, src, ur)
    for mode, th, ori in ((0, 15.0, True), (1, 7.0, True), (2, 15.0, False), (0, 3.0, True)):
        m.mbCheckOrientation = ori
        on, ocm = oracle.search_by_projection_frame(grid, d, SF, q, th, mode, ori, ur, occ)
        n1, cm1 = m.SearchByProjectionFrame(F, q, th, mode, occ, raw=True)
        n2, cm2 = m.SearchByProjectionFrame(D, q, th, mode, occ, raw=True)
        assert n1 == n2 == on and np.array_equal(np.maximum(cm1, -1), ocm) and np.array_equal(cm1, cm2), (mode, th, n1, n2, on)
    assert on > 0


def test_reuse_uploads_no_frame_rows(oracle):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(7)
    N, n_mp = 1000, 300
    k, d = _frame(rng, N)
    F = osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), SF)
    grid = oracle.OracleGrid(k, 0.0, float(W), 0.0, float(H))
    m = osa.ORBmatcher(0.8, True)
    D = osa.DeviceFrame(m, 2000).load(F)
    mp, _ = _mp(rng, k, d, n_mp, 2.0)
    for call, th in enumerate((1.0, 3.0, 5.0, 3.0, 10.0)):
        occ = (rng.random(N) < 0.1 * call).astype(np.uint8)
        on, ofm = oracle.search_by_projection_mappoints(grid, d, SF, mp, th, 0.8, None, occ)
        n, fm = m.SearchByProjection(D, mp, th, occ)
        assert n == on and np.array_equal(fm, ofm), (call, n, on)
        t = m.last_transfers()
        assert t["upload_bytes"] < 32 * N, t         # the queries and the mask only: no keypoint or descriptor row travels
    m.SearchByProjection(F, mp, 3.0, None)
    assert m.last_transfers()["upload_bytes"] >= 60 * N


def _batch(canvas, t0, nfr=8, nf=1000):
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    frames = np.stack([synth.frame_from_canvas(canvas, t0 + t, W, H, 1000 + t0 + t) for t in range(nfr)])
    return torch.from_numpy(frames).cuda()


def _m2_consecutive(oracle, prev, cur, sf):
    _, k0, d0 = prev
    _, k1, d1 = cur
    q = dict(u=k0["x"] - 2.0, v=k0["y"] - 1.0, ur=np.zeros(len(k0), np.float32), octave=k0["octave"], angle=k0["angle"], desc=d0,
             has_obs=np.ones(len(k0), np.uint8))
    grid = oracle.OracleGrid(k1, 0.0, float(W), 0.0, float(H))
    return q, oracle.search_by_projection_frame(grid, d1, sf, q, 15.0, 0, True, None, None)


def test_batch_load_equals_oracle_and_match_consecutive(oracle, canvas1):
    import torch
    import orb_slam3_amd as osa
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    nfr = 8
    d_frames = _batch(canvas1, 0, nfr)
    ex.extract_batch_device(d_frames.data_ptr(), nfr, W, H, W, W * H, (0, 1000))
    m = osa.ORBmatcher(0.9, True)
    cap = ex.batch_view().cap
    handles = [osa.DeviceFrame(m, cap).load_batch(ex, f) for f in range(nfr)]   # no host synchronisation in between
    d_match = torch.full((nfr, cap), -7, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(nfr, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ex.match_consecutive_device(d_match.data_ptr(), d_nm.data_ptr(), th=15.0, du=-2.0, dv=-1.0, check_orientation=True)
    ex.sync()
    match, nm = d_match.cpu().numpy(), d_nm.cpu().numpy()
    sf = ex.GetScaleFactors()
    outs = [ex.download(t) for t in range(nfr)]
    for f in range(1, nfr):
        q, (on, ocm) = _m2_consecutive(oracle, outs[f - 1], outs[f], sf)
        n, cm = m.SearchByProjectionFrame(handles[f], q, 15.0, 0, None)
        assert handles[f].count() == len(outs[f][1])
        assert n == on == nm[f] and np.array_equal(cm, ocm) and np.array_equal(match[f, :len(cm)], cm), (f, n, on, nm[f])
        assert on > 300


def test_batch_load_holds_a_copy(oracle, canvas1):
    import orb_slam3_amd as osa
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    m = osa.ORBmatcher(0.9, True)
    a = _batch(canvas1, 0)
    ex.extract_batch_device(a.data_ptr(), 8, W, H, W, W * H, (0, 1000))
    sf = ex.GetScaleFactors()
    prev, cur = ex.download(2), ex.download(3)
    q, (on, ocm) = _m2_consecutive(oracle, prev, cur, sf)
    D = osa.DeviceFrame(m, ex.batch_view().cap).load_batch(ex, 3)
    b = _batch(canvas1, 40)   # different images into the same extractor, enqueued right behind the copy
    ex.extract_batch_device(b.data_ptr(), 8, W, H, W, W * H, (0, 1000))
    n, cm = m.SearchByProjectionFrame(D, q, 15.0, 0, None)
    assert n == on and np.array_equal(cm, ocm), (n, on)
    ex.sync()
    assert ex.download(3)[1].tobytes() != cur[1].tobytes()   # the extractor's own outputs did change
    n2, cm2 = m.SearchByProjectionFrame(D, q, 15.0, 0, None)
    assert n2 == on and np.array_equal(cm2, ocm)


def _local_map(rng, k, n_mp, stereo):
    """map points back-projected from the frame's features (pose near identity) plus points anywhere: in and out of view, behind the camera"""
    fx, fy, cx, cy = EUROC4
    src = rng.integers(0, len(k), n_mp)
    z = rng.uniform(1.0, 30.0, len(k))[src] * rng.uniform(0.99, 1.01, n_mp)
    pos = np.stack([(k["x"][src] - cx) / fx * z, (k["y"][src] - cy) / fy * z, z], axis=1)
    far = rng.random(n_mp) < 0.25
    pos[far] = rng.uniform(-20, 20, (far.sum(), 3))
    pos = pos.astype(np.float32)
    normal = pos / np.linalg.norm(pos, axis=1, keepdims=True) + rng.normal(0, 0.3, pos.shape)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    dist = np.linalg.norm(pos, axis=1)
    max_d = (dist * 1.2 ** k["octave"][src] * rng.uniform(0.9, 1.1, n_mp)).astype(np.float32)
    min_d = (max_d / 1.2 ** 7).astype(np.float32)
    return src, pos, normal, min_d, max_d


@pytest.mark.parametrize("stereo", [False, True])
def test_search_local_points_equals_oracle_chain(oracle, stereo):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(31 + stereo)
    N, n_mp = 1500, 10000
    k, d = _frame(rng, N)
    bf = 47.9 if stereo else 0.0
    src, pos, normal, min_d, max_d = _local_map(rng, k, n_mp, stereo)
    ur = None
    if stereo:   # mvuRight of the features the points came from: u - bf / z (some features without a right match)
        zf = np.full(N, 10.0, np.float32)
        zf[src] = pos[:, 2]
        ur = (k["x"] - np.float32(bf) / np.maximum(zf, 0.5)).astype(np.float32)
        ur[rng.random(N) < 0.3] = -1.0
    desc = _noisy(rng, d[src], 0.05)
    eligible = (rng.random(n_mp) < 0.9).astype(np.uint8)
    has_obs = (rng.random(n_mp) < 0.95).astype(np.uint8)
    a = 0.01
    Rcw = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    tcw = np.array([0.02, -0.01, 0.03], np.float32)
    Ow = (-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(np.float32)
    bounds = np.array([0.0, float(W), 0.0, float(H)], np.float32)
    lsf = np.float32(np.log(np.float32(1.2)))
    F = osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), SF, ur)
    grid = oracle.OracleGrid(k, 0.0, float(W), 0.0, float(H))
    m = osa.ORBmatcher(0.8, True)
    D = osa.DeviceFrame(m, 2000).load(F)
    cam10 = EUROC4 + (0, 0, 0, 0, 0, bf)
    want = oracle.is_in_frustum(Rcw, tcw, Ow, EUROC4 + (bf,), bounds, lsf, 8, 0.5, pos, normal, min_d, max_d)
    assert 2000 < want["in_view"].sum() < n_mp
    occ = (rng.random(N) < 0.05).astype(np.uint8)
    for far_points, th_far, th in ((False, 0.0, 1.0), (True, 12.0, 3.0), (True, 20.0, 1.0)):
        n, fm, iv = m.SearchLocalPoints(D, cam10, (Rcw, tcw, Ow), lsf, 0.5, pos, normal, min_d, max_d, desc, eligible, has_obs, th, far_points,
                                        th_far, occ)
        assert np.array_equal(iv, want["in_view"] & eligible)
        searched = iv.astype(bool) & ~(far_points & (want["depth"] > np.float32(th_far)))
        mp = dict(proj_x=want["proj_x"], proj_y=want["proj_y"], proj_xr=want["proj_xr"], level=want["level"], view_cos=want["view_cos"], desc=desc,
                  in_view=searched.astype(np.uint8), has_obs=has_obs)
        on, ofm = oracle.search_by_projection_mappoints(grid, d, SF, mp, th, 0.8, ur, occ)
        assert n == on and np.array_equal(fm, ofm), (far_points, th, n, on)
        assert on > 100
        n1, fm1 = m.SearchByProjection(F, mp, th, occ)   # today's host-pointer call on the same records
        assert n1 == on and np.array_equal(fm1, ofm)
    # a FrameView is loaded into a handle for the call
    n3, fm3, iv3 = m.SearchLocalPoints(F, cam10, (Rcw, tcw, Ow), lsf, 0.5, pos, normal, min_d, max_d, desc, eligible, has_obs, th, far_points, th_far, occ)
    assert n3 == n and np.array_equal(fm3, fm) and np.array_equal(iv3, iv)


def test_errors_before_anything_is_enqueued(canvas1):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    BAD, TOO_LARGE = -2, -7
    m, m2 = osa.ORBmatcher(0.9, True), osa.ORBmatcher(0.9, True)
    h = C.c_void_p()
    assert L.orbx_frame_create(None, 100, C.byref(h)) == BAD
    assert L.orbx_frame_create(m._h, 100, None) == BAD
    assert L.orbx_frame_create(m._h, 16001, C.byref(h)) == TOO_LARGE
    with pytest.raises(osa.OrbxError):
        osa.DeviceFrame(m, 16001)
    D = osa.DeviceFrame(m, 200)
    assert L.orbx_frame_load_host(None, None) == BAD and L.orbx_frame_load_host(D._h, None) == BAD
    assert L.orbx_frame_count(D._h, None) == BAD and L.orbx_frame_count(None, None) == BAD
    rng = np.random.default_rng(3)
    k, d = _frame(rng, 201)
    with pytest.raises(osa.OrbxError):   # more rows than the handle holds
        D.load(osa.FrameView(k, d, 0.0, float(W), 0.0, float(H), SF))
    D.load(osa.FrameView(k[:150], d[:150], 0.0, float(W), 0.0, float(H), SF))
    mp, src = _mp(rng, k[:150], d[:150], 50, 2.0)
    out = np.zeros(150, np.int32)
    assert L.orbx_frame_search_by_projection_mappoints(m2._h, D._h, None, 50, *[None] * 8, 3.0, 0.8, out.ctypes.data) == BAD   # not its owner
    with pytest.raises(osa.OrbxError):
        m2.SearchByProjection(D, mp, 3.0)
    with pytest.raises(osa.OrbxError):
        m2.SearchByProjectionFrame(D, _queries(rng, k, d, src), 15.0)
    assert L.orbx_frame_search_local_points(m._h, None, None, None, None, 0.0, 0.5, 0, *[None] * 7, 1.0, 0.8, 0, 0.0, None, None) == BAD
    assert L.orbx_frame_load_batch(D._h, None, 0, None, None, 0) == BAD
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    b = _batch(canvas1, 0, 4)
    ex.extract_batch_device(b.data_ptr(), 4, W, H, W, W * H, (0, 1000))
    cap = ex.batch_view().cap
    big = osa.DeviceFrame(m, cap)
    for f in (4, -1):   # not a frame of the batch
        assert L.orbx_frame_load_batch(big._h, ex._h, f, None, None, 0) == BAD
    assert L.orbx_frame_load_batch(D._h, ex._h, 0, None, None, 0) == BAD   # the batch's per-frame capacity exceeds the handle's
    ex.sync()
    big.load_batch(ex, 3)
    assert big.count() == len(ex.download(3)[1])


def _whole(a):
    """The array a wrapper handed to the library, of which the returned `a` is the leading N entries of every row."""
    return a if a.base is None else a.base


# entry points that can be the first to touch a batch-loaded handle, and the value their wrappers fill the result arrays with
PENDING = {"mappoints": -1, "frame": -1, "window": -1, "local_points": -1, "compute_bow": 0, "search_by_bow": -1, "search_by_bow_resident": -1}


@pytest.mark.parametrize("entry", sorted(PENDING))
def test_count_pending_equals_counted_first(canvas1, entry):
    """Two handles loaded from the same batch frame with a capacity above N: A is counted first, B meets the call with its count still on the
    device.  The same return value, the same entries [0, N), nothing written beyond N (the wrappers' arrays have the handle's capacity and keep
    their fill there), and B knows A's count afterwards."""
    import orb_slam3_amd as osa
    from test_gpu_matcher import _random_vocabulary
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    d_frames = _batch(canvas1, 0)
    ex.extract_batch_device(d_frames.data_ptr(), 8, W, H, W, W * H, (0, 1000))
    sf = ex.GetScaleFactors().astype(np.float32)
    (_, k2, d2), (_, k, d) = ex.download(2), ex.download(3)
    N, cap = len(k), ex.batch_view().cap + 37
    assert 0 < N < cap
    rng = np.random.default_rng(17)
    m = osa.ORBmatcher(0.8, True)
    mp, src = _mp(rng, k, d, 700, 2.0)
    q = _queries(rng, k, d, src)
    if entry == "mappoints":
        def call(D):
            n, fm = m.SearchByProjection(D, mp, 3.0)
            return [n], [fm]
    elif entry == "frame":
        def call(D):
            n, cm = m.SearchByProjectionFrame(D, q, 15.0, 0, raw=True)
            return [n], [cm]
    elif entry == "window":
        o = q["octave"]
        qw = dict(x=q["u"], y=q["v"], r=(7.0 * sf[o]).astype(np.float32), min_level=o - 1, max_level=o + 1, angle=q["angle"], desc=q["desc"],
                  has_obs=q["has_obs"])

        def call(D):
            n, match = m.SearchByProjectionWindow(D, qw, 64.0, True, raw=True)
            return [n], [match]
    elif entry == "local_points":
        src, pos, normal, min_d, max_d = _local_map(rng, k, 3000, False)
        desc = _noisy(rng, d[src], 0.05)
        pose = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32))

        def call(D):
            n, fm, iv = m.SearchLocalPoints(D, EUROC4 + (0, 0, 0, 0, 0, 0.0), pose, np.float32(np.log(np.float32(1.2))), 0.5, pos, normal, min_d,
                                            max_d, desc, th=3.0)
            return [n, iv], [fm]
    else:
        cp, ci, nd, wi = _random_vocabulary(rng, 4, 2, ragged=False)
        voc = osa.ORBVocabulary(2, cp, ci, _noisy(rng, d[rng.integers(0, N, len(nd))], 0.03), wi)
        if entry == "compute_bow":
            def call(D):
                return [], list(D.compute_bow(voc, 1))
        elif entry == "search_by_bow":
            kfs = []
            for kk, dd in ((k2, d2), (k, d)):
                _, node = m.BowTransform(voc, dd, 1)
                nodes = np.unique(node)
                kfs.append((dd, kk["angle"], None, osa.FeatureVector(nodes, [np.nonzero(node == x)[0] for x in nodes])))

            def call(D):
                D.compute_bow(voc, 1, download=False)
                nm, match = m.SearchByBoWDevice(D, kfs)
                return [nm], [match]
        else:
            kf = osa.DeviceKeyFrame.from_host(m, osa.FrameView(k2, d2, 0.0, float(W), 0.0, float(H), sf))
            kf.compute_bow(m, voc, 1, download=False)

            def call(D):
                D.compute_bow(voc, 1, download=False)
                nm, match = m.SearchByBoWResident(D, [kf])
                return [nm], [match]
    A, B = osa.DeviceFrame(m, cap).load_batch(ex, 3), osa.DeviceFrame(m, cap).load_batch(ex, 3)
    assert A.count() == N
    (ra, a), (rb, b) = call(A), call(B)
    assert len(ra) == len(rb) and all(np.array_equal(x, y) for x, y in zip(ra, rb)), (ra, rb)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.shape[-1] == N and np.array_equal(x, y)
        for whole in (_whole(x), _whole(y)):
            assert whole.shape[-1] == cap and (whole[..., N:] == PENDING[entry]).all()
    if entry != "compute_bow":
        assert (a[0] >= 0).sum() > 50   # the call did match
    assert B.count() == N
