"""LoopClosing's Sim3 projection searches on resident key frames: orbx_keyframe_search_by_projection_sim3 (both SearchByProjection(KeyFrame*, Sim3f&,
...) overloads, ORBmatcher.cc:427-646) and orbx_keyframe_fuse_map_points_sim3 (SearchAndFuse's Fuse, :1339-1455).

The reference is COMPOSED in tests/sim3_scene.py from the oracle and float32 numpy, independent of the code under test.  Every comparison is equality
of integers or of float bit patterns; no pair is left out, except that proj_u / proj_v are compared only where projected == 1.  The tests that use
only host arrays also run on the CPU emulator (ORBX_TEST_EMULATOR=1)."""
import ctypes as C

import numpy as np
import pytest

import sim3_scene as S
import test_gpu_keyframe as T

pytestmark = pytest.mark.gpu

f32 = np.float32
TH_LOW = S.TH_LOW
BAD, TOO_LARGE = -2, -7


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes(oracle):
    out = {}
    for seed, K in S.SEEDS.items():
        sc = S.make_scene(seed, K)
        S.check_conditions(oracle, sc, range(K))
        out[seed] = sc
    return out


def _flags(sc, K):
    """skip: every 11th pair; occupied: every 7th feature on even k, no row on odd k."""
    n = len(sc["map_points"]["pos"])
    skip = (np.arange(K * n).reshape(K, n) % 11 == 0).astype(np.uint8)
    occ = [(np.arange(len(sc["key_frames"][k]["kps"])) % 7 == 0).astype(np.uint8) if k % 2 == 0 else None for k in range(K)]
    return skip, occ


def _key_frames(osa, m, sc, ks, isg=True, u_right=False):
    return [osa.DeviceKeyFrame.from_host(m, T._view(osa, sc, k, u_right), sc["inv_level_sigma2"] if isg else None) for k in ks]


def _search(m, kfs, sc, ks, th, ratio, form, skip, occ, **kw):
    return m.SearchByProjectionSim3KeyFrames(kfs, [sc["cams"][k] for k in ks], [sc["poses"][k] for k in ks], sc["map_points"], th, ratio,
                                             sc["log_scale_factor"], form, skip, occ, want_uv=True, **kw)


def _assert_search_equal(got, ref):
    nm, match, pr, (pu, pv) = got
    assert np.array_equal(pr, ref["projected"]), np.nonzero(pr != ref["projected"])
    on = ref["projected"] == 1
    assert np.array_equal(_bits(pu)[on], _bits(ref["u"])[on]) and np.array_equal(_bits(pv)[on], _bits(ref["v"])[on])
    for k, (a, b) in enumerate(zip(match, ref["match"])):
        assert np.array_equal(a, b), (k, np.nonzero(a != b))
    assert np.array_equal(nm, ref["nm"])


# ---- 1. the search form against the composed reference ----
@pytest.mark.parametrize("th,ratio", [(8.0, 1.5), (5.0, 1.0)])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("seed", sorted(S.SEEDS))
def test_search_form_equals_the_composed_reference(oracle, scenes, seed, form, th, ratio):
    import orb_slam3_amd as osa
    sc, K = scenes[seed], S.SEEDS[seed]
    skip, occ = _flags(sc, K)
    ref = S.search_reference(oracle, sc, range(K), th, ratio, form, skip, occ)
    assert ref["nm"].sum() >= 0.1 * ref["projected"].size     # (with a ninth of the pairs skipped and a seventh of the features taken)
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    _assert_search_equal(_search(m, kfs, sc, range(K), th, ratio, form, skip, occ), ref)
    # no flags at all, and the optional outputs left out
    ref0 = S.search_reference(oracle, sc, range(K), th, ratio, form)
    nm, match, pr, uv = m.SearchByProjectionSim3KeyFrames(kfs, sc["cams"][:K], sc["poses"][:K], sc["map_points"], th, ratio, sc["log_scale_factor"], form,
                                                          want_projected=False)
    assert pr is None and uv is None and np.array_equal(nm, ref0["nm"]) and all(np.array_equal(a, b) for a, b in zip(match, ref0["match"]))


# ---- 2. the rows of one call are independent problems, each today's window search on that key frame ----
@pytest.mark.parametrize("form", [0, 1])
def test_rows_are_independent_and_equal_the_host_pointer_window_search(oracle, scenes, form):
    import orb_slam3_amd as osa
    sc, K, th, ratio = scenes[5], 3, 8.0, 1.5
    skip, occ = _flags(sc, K)
    ref = S.search_reference(oracle, sc, range(K), th, ratio, form, skip, occ)
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    nm3, match3, pr3, (pu3, pv3) = _search(m, kfs, sc, range(K), th, ratio, form, skip, occ)
    for k in range(K):
        nm1, match1, pr1, (pu1, pv1) = _search(m, [kfs[k]], sc, [k], th, ratio, form, skip[k:k + 1], [occ[k]])
        assert nm1[0] == nm3[k] and np.array_equal(match1[0], match3[k]) and np.array_equal(pr1[0], pr3[k])
        assert np.array_equal(_bits(pu1[0]), _bits(pu3[k])) and np.array_equal(_bits(pv1[0]), _bits(pv3[k]))
        sel, q = ref["recs"][k]
        n, mm = m.SearchByProjectionWindow(T._view(osa, sc, k, u_right=False), q, float(f32(TH_LOW) * f32(ratio)), False, occ[k])
        assert n == nm3[k] and np.array_equal(np.where(mm >= 0, sel[np.maximum(mm, 0)], -1), match3[k]), k
        assert n > 40


# ---- 3. the Fuse form ----
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("seed", sorted(S.SEEDS))
def test_fuse_form_equals_the_composed_reference(oracle, scenes, seed, with_skip):
    import orb_slam3_amd as osa
    sc, K = scenes[seed], S.SEEDS[seed]
    skip = _flags(sc, K)[0] if with_skip else None
    bi, bd, pr, recs = S.fuse_reference(oracle, sc, range(K), T.TH, skip)
    assert pr.mean() >= 0.5 and (bd <= TH_LOW).mean() >= 0.2
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(K))
    gi, gd, gp = m.FuseMapPointsSim3(kfs, sc["cams"][:K], sc["poses"][:K], sc["map_points"], T.TH, sc["log_scale_factor"], skip)
    assert np.array_equal(gp, pr), np.nonzero(gp != pr)
    assert np.array_equal(gi, bi) and np.array_equal(gd, bd)
    # == the gate-less search on resident key frames fed the reference's queries
    rows = m.FuseSearchKeyFrames(kfs, [q for _, q in recs], use_chi2=False)
    for k, ((sel, _), (ri, rd)) in enumerate(zip(recs, rows)):
        assert np.array_equal(ri, gi[k, sel]) and np.array_equal(rd, gd[k, sel]), k
    # key frames made WITHOUT inv_level_sigma2, and key frames that carry mvuRight: the same rows
    for isg, u_right in ((False, False), (True, True)):
        other = _key_frames(osa, m, sc, range(K), isg, u_right)
        oi, od, op = m.FuseMapPointsSim3(other, sc["cams"][:K], sc["poses"][:K], sc["map_points"], T.TH, sc["log_scale_factor"], skip)
        assert np.array_equal(oi, bi) and np.array_equal(od, bd) and np.array_equal(op, pr), (isg, u_right)
    si, sd, sp = m.FuseMapPointsSim3(kfs, sc["cams"][:K], sc["poses"][:K], sc["map_points"], T.TH, sc["log_scale_factor"], skip, want_projected=False)
    assert sp is None and np.array_equal(si, bi) and np.array_equal(sd, bd)


def test_fuse_form_takes_key_frames_with_different_bounds_in_one_call(oracle):
    import orb_slam3_amd as osa
    bounds = [(0.0, 752.0, 0.0, 480.0), (-18.5, 770.25, -12.0, 495.5)]
    sc = S.make_scene(31, 2, special=False, bounds=bounds)
    bi, bd, pr, _ = S.fuse_reference(oracle, sc, range(2), T.TH)
    m = osa.ORBmatcher(0.6, True)
    kfs = _key_frames(osa, m, sc, range(2), isg=False)
    gi, gd, gp = m.FuseMapPointsSim3(kfs, sc["cams"], sc["poses"], sc["map_points"], T.TH, sc["log_scale_factor"])
    assert np.array_equal(gp, pr) and np.array_equal(gi, bi) and np.array_equal(gd, bd)
    assert (bd[0] <= TH_LOW).sum() > 40 and (bd[1] <= TH_LOW).sum() > 40
    with pytest.raises(osa.OrbxError):   # the search form takes one set of grid parameters per launch
        m.SearchByProjectionSim3KeyFrames(kfs, sc["cams"], sc["poses"], sc["map_points"], 8.0, 1.5, sc["log_scale_factor"])


# ---- 4. key frames made from a host-loaded handle ----
def test_key_frames_from_a_handle_give_the_rows_of_host_made_ones(oracle, scenes):
    import orb_slam3_amd as osa
    sc, K, th, ratio = scenes[6], 3, 8.0, 1.5
    skip, occ = _flags(sc, K)
    m = osa.ORBmatcher(0.6, True)
    D = osa.DeviceFrame(m, max(len(kf["kps"]) for kf in sc["key_frames"]) + 50)
    kfs = []
    for k in range(K):
        D.load(T._view(osa, sc, k, u_right=bool(k % 2)))
        kfs.append(osa.DeviceKeyFrame.from_frame(m, D, None if k == 1 else sc["inv_level_sigma2"]))
    D.load(T._view(osa, sc, 0))                                # the handle holds another frame before anything is searched
    assert [kf.count() for kf in kfs] == [len(kf["kps"]) for kf in sc["key_frames"]]
    for form in (0, 1):
        _assert_search_equal(_search(m, kfs, sc, range(K), th, ratio, form, skip, occ), S.search_reference(oracle, sc, range(K), th, ratio, form, skip, occ))
    bi, bd, pr, _ = S.fuse_reference(oracle, sc, range(K), T.TH, skip)
    gi, gd, gp = m.FuseMapPointsSim3(kfs, sc["cams"], sc["poses"], sc["map_points"], T.TH, sc["log_scale_factor"], skip)
    assert np.array_equal(gp, pr) and np.array_equal(gi, bi) and np.array_equal(gd, bd)


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
    m.FuseMapPointsSim3(kfs[:1], sc["cams"][:1], sc["poses"][:1], mp, T.TH, sc["log_scale_factor"])   # the last call that enqueues anything
    before = m.last_transfers()
    assert before["uploads"] == 1 and before["downloads"] == 1
    kps, desc = sc["key_frames"][0]["kps"], sc["key_frames"][0]["desc"]
    left = osa.FrameView(kps[:100], desc[:160], 0.0, float(T.W), 0.0, float(T.H), sc["scale_factors"])
    rig = osa.DeviceKeyFrame.from_host_fisheye(m, left, kps[100:160], sc["inv_level_sigma2"])
    odd = osa.DeviceKeyFrame.from_host(m, T._view(osa, sc, 1, False, bounds=(0.0, 752.0, 0.0, 480.5)), None)   # other image bounds
    made = m.last_transfers()
    vp = C.c_void_p
    hs = lambda *k: (vp * len(k))(*[None if x is None else x._h.value if isinstance(x._h, vp) else x._h for x in k])   # noqa: E731
    cams = (_lib.Camera * 3)(*[_lib.Camera(*[float(x) for x in c]) for c in sc["cams"][:3]])
    poses = (_lib.FramePose * 3)(*[_lib.FramePose.make(*p) for p in sc["poses"][:3]])
    pts = [mp["pos"].ctypes.data, mp["normal"].ctypes.data, mp["min_dist"].ctypes.data, mp["max_dist"].ctypes.data, mp["desc"].ctypes.data]
    rows_np = [np.full(400, 7, np.int32) for _ in range(3)]
    rows = (vp * 3)(*[r.ctypes.data for r in rows_np])
    nm = np.full(3, 7, np.int32)
    bi, bd = np.zeros(3 * n, np.int32), np.zeros(3 * n, np.int32)
    uv = np.zeros(3 * n, f32)

    def search(K, h, form=0, r=rows, n_mp=n, nmp=nm.ctypes.data, pu=None, pv=None, points=pts):
        return L.orbx_keyframe_search_by_projection_sim3(m._h, K, h, cams, poses, 8.0, 1.5, 0.18, form, n_mp, *points, None, None, r, nmp, None, pu, pv)

    def fuse(K, h, n_mp=n, out=bi.ctypes.data, points=pts):
        return L.orbx_keyframe_fuse_map_points_sim3(m._h, K, h, cams, poses, 3.0, 0.18, n_mp, *points, None, out, bd.ctypes.data, None)

    assert search(2, hs(kfs[0], rig)) == BAD and fuse(2, hs(kfs[0], rig)) == BAD                     # a fisheye key frame
    assert search(2, hs(kfs[0], None)) == BAD and fuse(2, hs(kfs[0], None)) == BAD                   # a NULL key frame
    assert search(2, hs(*kfs[:2]), r=(vp * 3)(rows_np[0].ctypes.data, None, None)) == BAD           # a NULL match row
    assert search(1, hs(kfs[0]), form=2) == BAD and search(1, hs(kfs[0]), form=-1) == BAD           # projection_form not 0 / 1
    assert search(2, hs(kfs[0], odd)) == BAD                                                        # unequal bounds in the search form
    assert search(1, hs(kfs[0]), pu=uv.ctypes.data) == BAD                                          # proj_u without proj_v
    assert search(1, hs(kfs[0]), nmp=None) == BAD and fuse(1, hs(kfs[0]), out=None) == BAD
    assert search(1, hs(kfs[0]), points=[None] + pts[1:]) == BAD and fuse(1, hs(kfs[0]), points=[None] + pts[1:]) == BAD
    nmax = _lib.MAX_FUSE_KEYFRAMES
    many = (vp * (nmax + 1))(*[kfs[0]._h.value if isinstance(kfs[0]._h, vp) else kfs[0]._h] * (nmax + 1))
    assert L.orbx_keyframe_fuse_map_points_sim3(m._h, nmax + 1, many, None, None, 3.0, 0.18, 0, *pts, None, None, None, None) == BAD
    big = ((_lib.Camera * (nmax + 1))(), (_lib.FramePose * (nmax + 1))())
    assert L.orbx_keyframe_fuse_map_points_sim3(m._h, nmax + 1, many, *big, 3.0, 0.18, n, *pts, None, bi.ctypes.data, bd.ctypes.data, None) == TOO_LARGE
    if _lib_device_count() > 1:                                                                     # a key frame of another device
        m1 = osa.ORBmatcher(0.6, True, device=1)
        far = osa.DeviceKeyFrame.from_host(m1, T._view(osa, sc, 0, False), None)
        assert search(1, hs(far)) == BAD and fuse(1, hs(far)) == BAD
    assert all(np.all(r == 7) for r in rows_np) and np.all(nm == 7)                                 # a refused call writes nothing
    # n_kf = 0 and n_mp = 0 are fine: rows all -1, nmatches 0
    assert search(0, None, r=None, nmp=None) == 0 and fuse(0, None, out=None) == 0
    assert search(2, hs(*kfs[:2]), n_mp=0) == 0 and fuse(2, hs(*kfs[:2]), n_mp=0) == 0
    for k in range(2):
        N = len(sc["key_frames"][k]["kps"])
        assert np.all(rows_np[k][:N] == -1) and np.all(rows_np[k][N:] == 7) and nm[k] == 0
    assert m.last_transfers() == made, (m.last_transfers(), made)


def _lib_device_count():
    import os
    if os.environ.get("ORBX_TEST_EMULATOR"):
        return 1
    import torch
    return torch.cuda.device_count()


# ---- 6. the cost does not grow with K ----
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
        m.FuseMapPointsSim3(kfs[:K], sc["cams"][:K], sc["poses"][:K], sc["map_points"], T.TH, sc["log_scale_factor"], skip[:K])
        tf[K] = m.last_transfers()
    for t in (ts, tf):
        assert t[1]["uploads"] == t[3]["uploads"] == 1 and t[1]["downloads"] == t[3]["downloads"] == 1, t
        assert t[1]["xfer_launches"] + t[1]["dma_submissions"] == t[3]["xfer_launches"] + t[3]["dma_submissions"] == 2, t
    n = len(sc["map_points"]["pos"])
    assert ts[1]["upload_bytes"] >= 60 * n and tf[1]["upload_bytes"] >= 60 * n            # the map points do go up (once)
    assert ts[3]["upload_bytes"] - ts[1]["upload_bytes"] < 60 * n                           # ... and not once per key frame
    assert tf[3]["upload_bytes"] - tf[1]["upload_bytes"] < 60 * n
