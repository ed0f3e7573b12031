"""Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166) whole on the device: k_knn2 over the lapping-area tails, then k_tri_kb8_stereo (Lowe's ratio,
KannalaBrandt8::TriangulateMatches of the rig's two cameras, the four output vectors) -- single call, batched on two resident extractions, and the C++
overload.  Every output byte for byte against the oracle's Frame::ComputeStereoFishEyeMatches with a triangulation callback built from the oracle's
KannalaBrandt8 functions: the value is orbo_kb8_triangulate_matches', p3D is recomputed here in float32 from orbo_kb8_unproject and
orbo_eigen_jacobi_svd4_V in the order that function uses."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle_binding as ob

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
SIGMA2 = (np.array([1.2 ** i for i in range(8)], np.float32) ** 2).astype(np.float32)


def _x3d(cam1, cam2, xy1, xy2, R12, t12):
    """x3D of KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:305-368, Triangulate :387-400), operation for operation as orbo_kb8_triangulate_matches"""
    r1 = ob.kb8_unproject(cam1, np.array([xy1], f32))[0]
    r2 = ob.kb8_unproject(cam2, np.array([xy2], f32))[0]
    R = np.asarray(R12, f32).reshape(3, 3)
    t = np.asarray(t12, f32).ravel()
    R21 = R.T.copy()
    T1 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
    T2 = np.zeros((3, 4), f32)
    for i in range(3):
        T2[i, :3] = R21[i]
        T2[i, 3] = ((f32(0) + (-R21[i, 0]) * t[0]) + (-R21[i, 1]) * t[1]) + (-R21[i, 2]) * t[2]
    A = np.zeros((4, 4), f32)
    for j in range(4):
        A[0, j] = r1[0] * T1[2, j] - T1[0, j]
        A[1, j] = r1[1] * T1[2, j] - T1[1, j]
        A[2, j] = r2[0] * T2[2, j] - T2[0, j]
        A[3, j] = r2[1] * T2[2, j] - T2[1, j]
    V = np.zeros(16, f32)
    L = ob.lib()
    L.orbo_eigen_jacobi_svd4_V.restype = None
    L.orbo_eigen_jacobi_svd4_V(A.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p), None)
    return (V[3] / V[15], V[7] / V[15], V[11] / V[15])


def oracle_triangulate(kl, kr, rig, seen=None):
    """KannalaBrandt8::TriangulateMatches(mpCamera2, mvKeys[iL], mvKeysRight[iR], mRlr, mtlr, sigma1, sigma2, p3D) as a callback"""
    cl, cr, R, t = (np.asarray(rig[k], f32) for k in ("cam_left", "cam_right", "R_lr", "t_lr"))

    def tri(il, ir, s1, s2):
        xy1 = (kl["x"][il], kl["y"][il])
        xy2 = (kr["x"][ir], kr["y"][ir])
        _, val = ob.kb8_epipolar_constrain(cl, cr, np.array([xy1], f32), np.array([xy2], f32), R, t, np.array([s1], f32), np.array([s2], f32))
        v = f32(val[0])
        if seen is not None:
            seen.append(float(v))
        p = _x3d(cl, cr, xy1, xy2, R, t) if v > 0 else (0.0, 0.0, 0.0)   # the reference sets p3D on success only
        return float(v), p
    return tri


def _same(got, want, what=""):
    (n, nd, *a), (on, ond, *o) = got, want
    assert (n, nd) == (on, ond), (what, n, nd, on, ond)
    for name, x, y in zip(("l2r", "r2l", "depth", "u_right", "p3d"), a, o):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name, int((x != y).sum()))


SHAPES = [(600, 580, 350, 330), (300, 40, 0, 39), (50, 60, 50, 10), (64, 64, 10, 64), (200, 220, 199, 0), (2500, 2400, 700, 650)]


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_single_call_equals_oracle(case):
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    n_left, n_right, mono_left, mono_right = SHAPES[case]
    rng = np.random.default_rng(900 + case)
    kl, dl, kr, dr, ml, mr, rig, _, _ = synth.make_fisheye_stereo_frame(rng, int(1.7 * max(n_left, n_right)) + 100, n_left, n_right, mono_left, mono_right)
    want = ob.stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, SIGMA2, oracle_triangulate(kl, kr, rig))
    m = osa.ORBmatcher()
    _same(m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, rig), want, case)
    _same(m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, osa.FisheyeRig(**rig)), want, case)   # the dataclass form
    if case in (0, 5):
        assert want[0] > 50, want[:2]
    if case in (2, 3):
        assert want[0] == 0 and want[1] == 0


def test_every_lapping_query_reaches_the_gate():
    """Equal descriptors for true correspondents, distinct random ones otherwise, every left tail point in the right tail: every query passes the
    ratio test, so every one is triangulated -- thousands of values, accepted and rejected, in the outputs."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    rng = np.random.default_rng(31)
    kl, dl, kr, dr, ml, mr, rig, idl, idr = synth.make_fisheye_stereo_frame(rng, 4200, 2200, 2400, 150, 100, flip=0.0)
    assert np.isin(idl[ml:], idr[mr:]).all()
    seen = []
    want = ob.stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, SIGMA2, oracle_triangulate(kl, kr, rig, seen))
    got = osa.ORBmatcher().ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, rig)
    _same(got, want)
    assert want[1] == len(kl) - ml and len(seen) == want[1]   # every lapping query passed the ratio test
    vals = np.array(seen, np.float32)
    assert want[0] > 1000 and (vals <= 0.0001).sum() > 50, (want[0], np.unique(vals[vals < 0], return_counts=True))
    assert len(set(vals[vals < 0].tolist()) & {-1.0, -4.0, -5.0}) >= 2


def test_right_to_left_conflicts_keep_the_largest_accepted_query():
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    rng = np.random.default_rng(47)
    kl, dl, kr, dr, ml, mr, rig, _, _ = synth.make_fisheye_stereo_frame(rng, 1400, 700, 700, 100, 100, flip=0.0)
    m = osa.ORBmatcher()
    base = m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, rig)
    acc = np.nonzero(base[2] >= 0)[0]
    assert len(acc) > 40
    # several left features become copies (keypoint and descriptor) of accepted ones: they reach the same right feature and triangulate alike
    src = rng.choice(acc, 12, replace=False)
    for s in src:
        for d in rng.choice(np.arange(ml, len(kl)), 3, replace=False):
            if d not in src:
                kl[d], dl[d] = kl[s], dl[s]
    want = ob.stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, SIGMA2, oracle_triangulate(kl, kr, rig))
    got = m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, rig)
    _same(got, want)
    l2r, r2l = got[2], got[3]
    conflicts = 0
    for ir in np.unique(l2r[l2r >= 0]):
        who = np.nonzero(l2r == ir)[0]
        assert r2l[ir] == who.max()
        conflicts += len(who) > 1
    assert conflicts >= 5, conflicts


def test_accepted_depths_equal_the_reference_text():
    from oracle import ref_binding as rb
    if not (ROOT / "oracle" / "_ref" / "libfrustum_ref.so").exists():
        pytest.skip("oracle/_ref/libfrustum_ref.so not built (needs the reference source tree at build time)")
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    rng = np.random.default_rng(5)
    kl, dl, kr, dr, ml, mr, rig, _, _ = synth.make_fisheye_stereo_frame(rng, 2000, 1200, 1200, 300, 300)
    n, _, l2r, _, depth, _, _ = osa.ORBmatcher().ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, rig)
    a = np.nonzero(l2r >= 0)[0]
    b = l2r[a]
    assert n == len(a) > 50
    _, val, _ = rb.ref_kb8_triangulate_matches(rig["cam_left"], rig["cam_right"], np.stack([kl["x"][a], kl["y"][a]], 1), np.stack([kr["x"][b], kr["y"][b]], 1),
                                               rig["R_lr"], rig["t_lr"], SIGMA2[kl["octave"][a]], SIGMA2[kr["octave"][b]])
    assert val.tobytes() == depth[a].tobytes()


def _rig_for_shifted_images():
    from orb_slam3_amd import synth
    cam = np.array(synth.TUMVI_L, np.float32)
    return dict(cam_left=cam, cam_right=cam.copy(), R_lr=np.eye(3, dtype=np.float32), t_lr=np.array([0.1, 0.0, 0.0], np.float32))


def test_batch_on_two_resident_extractions():
    """orbx_stereo_fisheye_batch_device on 8 stereo pairs of 512 x 512: per-frame download == download_all == the single call on the frame's
    downloaded features == the oracle, with lapping areas that make the mono index 0 and not 0.  Then ordering: the stage, the NEXT pair of batches
    extracted right behind it, and only then the download -- still the first batch's results.  A pinhole rig's stereo stage in the same process keeps
    its results."""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    w = h = 512
    nb, nf = 8, 1000
    canvas = synth.make_canvas(11, size=2048)
    pairs = [synth.make_stereo_pair(11, t, w, h, canvas) for t in range(2 * nb)]
    left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    fs = w * h
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    pl, pr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)   # a pinhole rig beside it
    rig = _rig_for_shifted_images()
    sg = exl.GetScaleSigmaSquares().astype(np.float32)
    m = osa.ORBmatcher()

    pl.extract_batch_device(left.data_ptr(), nb, w, h, w, fs, (0, 0))
    pr.extract_batch_device(right.data_ptr(), nb, w, h, w, fs, (0, 0))
    pl.stereo_batch_device(pr, 40.0, 0.1)
    pin_ref = [pl.stereo_download(t) for t in range(nb)]

    def extract(first, lap):
        exl.extract_batch_device(left.data_ptr() + first * fs, nb, w, h, w, fs, lap)
        exr.extract_batch_device(right.data_ptr() + first * fs, nb, w, h, w, fs, lap)

    results = {}
    for lap in ((0, 511), (200, 511)):
        extract(0, lap)
        exl.stereo_fisheye_batch_device(exr, rig)
        pl.stereo_batch_device(pr, 40.0, 0.1)   # the pinhole stage on the other rig, interleaved
        al = exl.stereo_fisheye_download_all()
        monos, total = [], 0
        for t in range(nb):
            one = exl.stereo_fisheye_download(t)
            ml, kl, dl = exl.download(t)
            mr, kr, dr = exr.download(t)
            monos.append(ml)
            nl, nr = len(kl), len(kr)
            assert one[0] == al[0][t] and one[1] == al[1][t]
            for x, y in zip(one[2:], (al[2][t, :nl], al[3][t, :nr], al[4][t, :nl], al[5][t, :nl])):
                assert x.tobytes() == y.tobytes(), (lap, t)
            single = m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, sg, rig)
            want = ob.stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, sg, oracle_triangulate(kl, kr, rig))
            _same(single, want, (lap, t))
            n, nd, l2r, r2l, depth, ur, p3d = single
            _same((one[0], one[1], one[2], one[3], one[4], ur, one[5]), want, (lap, t))
            total += n
        assert total > 0, lap
        if lap[0] > 0:
            assert min(monos) > 0, monos
        else:
            assert max(monos) == 0, monos
        results[lap] = [exl.stereo_fisheye_download(t) for t in range(nb)]
    # ordering: the stage, then the next pair of batches, then the download
    extract(0, (200, 511))
    exl.stereo_fisheye_batch_device(exr, rig)
    extract(nb, (200, 511))
    for t in range(nb):
        got = exl.stereo_fisheye_download(t)
        for x, y in zip(got, results[(200, 511)][t]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), t
    for t in range(nb):
        nm, ur, depth = pl.stereo_download(t)
        assert nm == pin_ref[t][0] and ur.tobytes() == pin_ref[t][1].tobytes() and depth.tobytes() == pin_ref[t][2].tobytes(), t


@pytest.mark.skipif(bool(os.environ.get("ORBX_TEST_EMULATOR")), reason="runs a separately built program")
def test_cpp_rig_overload_equals_python(tmp_path):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib, synth
    exe = tmp_path / "stereo_fisheye_demo"
    r = subprocess.run(["g++", "-std=c++17", "-O1", str(ROOT / "tests/cpp/stereo_fisheye_demo.cpp"), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(77)
    kl, dl, kr, dr, ml, mr, rig, _, _ = synth.make_fisheye_stereo_frame(rng, 2000, 1100, 1000, 250, 200)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(kl), len(kr), ml, mr, len(SIGMA2)], np.int32).tobytes())
        f.write(np.concatenate([np.asarray(rig[k], np.float32).ravel() for k in ("cam_left", "cam_right", "R_lr", "t_lr")]).tobytes())
        f.write(SIGMA2.tobytes() + kl.tobytes() + dl.tobytes() + kr.tobytes() + dr.tobytes())
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = str(Path(torch.__file__).parent / "lib") + ":" + env.get("LD_LIBRARY_PATH", "")   # the HIP runtime the tests use
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(out, np.uint8)
    nl, nr = len(kl), len(kr)
    c = raw[:8].view(np.int32)
    o = 8
    parts = []
    for cnt, dt in ((nl, np.int32), (nr, np.int32), (nl, np.float32), (nl, np.float32), (3 * nl, np.float32)):
        parts.append(raw[o:o + 4 * cnt].view(dt))
        o += 4 * cnt
    assert o == len(raw)
    want = osa.ORBmatcher().ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, SIGMA2, rig)
    assert (int(c[0]), int(c[1])) == want[:2] and want[0] > 50
    for x, y in zip(parts, want[2:]):
        assert x.tobytes() == np.asarray(y).tobytes()
