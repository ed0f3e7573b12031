"""References and inputs for the rectified-stereo / RGB-D depth path of resident frames (tests/test_gpu_stereo_resident.py).  Everything here is float32
numpy arithmetic on host arrays: Frame::ComputeStereoFromRGBD and Frame::UnprojectStereo restated, the depth images of the RGB-D tests, and
check_conditions, which is evaluated on the references alone -- nothing here calls the code under test."""
import numpy as np

f32 = np.float32

# the RGB-D batch: 3 frames of 320 x 240, a distorting camera (fx, fy, cx, cy, k1, k2, p1, p2, k3, bf)
W, H, FRAMES = 320, 240, 3
PITCH = 4 * (W + 7)                       # bytes per row: above 4 * W, the padding holds garbage
CAMERA = (265.0, 262.0, 161.5, 118.25, -0.28, 0.07, 1.5e-4, -2.0e-4, 0.0, 40.0)
BF = f32(40.0)
# columns [x0, x1) of every frame hold this value instead of the ramp: no depth (0, negative, NaN) or a depth that overflows nothing (1e-30 > 0)
HOLES = ((40, 70, 0.0), (100, 130, -1.0), (160, 190, float("nan")), (220, 250, 1e-30))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def depth_images(seed=3):
    """[FRAMES] images of H rows of PITCH bytes: d(x, y) = 0.5 + 0.01 x + 0.003 y + frame -- a wrong pixel, a rounded coordinate or a wrong frame
    changes the value -- with the HOLES, and random positive garbage in the padding behind every row."""
    rng = np.random.default_rng(seed)
    buf = rng.uniform(100.0, 200.0, (FRAMES, H, PITCH // 4)).astype(f32)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for f in range(FRAMES):
        buf[f, :, :W] = (0.5 + 0.01 * x + 0.003 * y + f).astype(f32)
        for x0, x1, v in HOLES:
            buf[f, :, x0:x1] = f32(v)
    return buf


def reference_rgbd(img, kps, kps_un, bf):
    """Frame::ComputeStereoFromRGBD: img [rows][>= width] float32 (one frame), kps = mvKeys, kps_un = mvKeysUn.  Returns (mvuRight, mvDepth, n with depth)."""
    ui, vi = np.trunc(kps["x"]).astype(np.int64), np.trunc(kps["y"]).astype(np.int64)   # (int)v, (int)u: truncation
    d = img[vi, ui].astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        has = d > 0                                                                      # a NaN fails it
        ur = np.where(has, kps_un["x"].astype(f32) - f32(bf) / d, f32(-1)).astype(f32)   # one division, one subtraction, each rounded to float32
    return ur, np.where(has, d, f32(-1)).astype(f32), int(has.sum())


def reference_unproject(xy, depth, view):
    """Frame::UnprojectStereo per feature: xy [n][2] = the key points the member reads, view = dict(R=Rcw [3, 3], Ow [3], p=(fx, fy, cx, cy)).
    Returns (pos [n, 3] float32 -- rows without depth hold NaN --, has [n])."""
    R, Ow = np.asarray(view["R"], f32), np.asarray(view["Ow"], f32)
    fx, fy, cx, cy = [f32(v) for v in view["p"]]
    invfx, invfy = f32(1) / fx, f32(1) / fy
    z = np.asarray(depth, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        has = z > 0
        x = ((xy[:, 0].astype(f32) - cx) * z) * invfx                                    # a subtraction and two products, each rounded on its own
        y = ((xy[:, 1].astype(f32) - cy) * z) * invfy
        pos = np.full((len(z), 3), np.nan, f32)
        for r in range(3):                                                               # row r of Rwc = column r of Rcw; dot3: ((0 + a0 b0) + a1 b1) + a2 b2
            s = ((f32(0) + R[0, r] * x) + R[1, r] * y) + R[2, r] * z
            pos[:, r] = np.where(has, s + Ow[r], f32(np.nan))
    return pos, has


def view_of(seed, p):
    """A key frame pose that is no identity: Rcw from a small rotation vector, tcw random; Ow = -Rwc tcw."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.2, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    t = rng.normal(0, 0.5, 3)
    return dict(R=R.astype(f32), t=t.astype(f32), Ow=(-R.T @ t).astype(f32), p=np.asarray(p, f32))


def check_conditions_rgbd(frames):
    """frames: [(kps, kps_un)] per frame, as the extractor gave them.  The properties the RGB-D test relies on, from the inputs and the reference alone."""
    imgs = depth_images()
    for f, (k, ku) in enumerate(frames):
        assert (k["x"] >= 0).all() and (k["x"] < W).all() and (k["y"] >= 0).all() and (k["y"] < H).all()
        trunc_differs = (np.trunc(k["x"]) != np.rint(k["x"])) | (np.trunc(k["y"]) != np.rint(k["y"]))
        assert trunc_differs.sum() >= 50, (f, int(trunc_differs.sum()))                  # a rounded coordinate reads another pixel
        assert (k["x"] != ku["x"]).sum() >= 50, f                                        # mvKeysUn, not mvKeys, enters mvuRight
        ui = np.trunc(k["x"]).astype(np.int64)
        in_hole = np.zeros(len(k), bool)
        for x0, x1, _ in HOLES:
            in_hole |= (ui >= x0) & (ui < x1)
        assert in_hole.sum() >= 10, (f, int(in_hole.sum()))
        ur, d, n = reference_rgbd(imgs[f], k, ku, BF)
        assert 0 < n < len(k) and ((d == -1) == (ur == -1)).all()


# ---------------------------------------------------------------------------------------------------------
# The stereo branches of LocalMapping::CreateNewMapPoints on two Pinhole key frames that hold mvuRight, mvDepth and raw key points.
# The scene starts from new_points_scene's monocular one (its pairs stay, as class (g) and more) and designs stereo pairs on the features that scene
# left free; reference_stereo hands every pair without a stereo observation to new_points_scene.reference_new_points and restates the member's stereo
# text (include/orbx.h) for the others.  PARITY UNPINNED, as there.
# ---------------------------------------------------------------------------------------------------------
import ctypes as C

import new_points_scene as N

UNPROJECT_FAILED = 12
STATUS = N.STATUS + ("UNPROJECT_FAILED",)
MB = f32(0.11)
MBF = f32(MB * f32(N.MONO_CAM[0]))
PAIR_COUNTS = N.PAIR_COUNTS
CLASSES = ("a_between", "a_reproj_r", "a_plain", "b", "c", "d", "e_turned", "f", "h_reproj_2", "h_behind", "h_scale")
PER_CLASS = 8
_libm = C.CDLL("libm.so.6")
_libm.atan2f.restype = C.c_float
_libm.atan2f.argtypes = [C.c_float, C.c_float]


def _cosf(x):
    from oracle import oracle_binding as ob
    return f32(ob.lib().orbo_cosf(float(x)))


def _cos_parallax_stereo(mb, depth):
    """cos(2 * atan2(mb / 2, depth)) in the float overloads: a float halving, atan2f, an exact doubling, cosf."""
    return _cosf(f32(f32(2) * f32(_libm.atan2f(float(f32(mb / f32(2))), float(depth)))))


def _unproject_kf(kf, view, i):
    """KeyFrame::UnprojectStereo(i): the RAW key point.  None when mvDepth[i] <= 0 (or NaN)."""
    z = kf["depth"][i]
    if not z > 0:
        return None
    pos, _ = reference_unproject(kf["keys_xy"][i:i + 1], np.array([z], f32), view)
    return [pos[0, 0], pos[0, 1], pos[0, 2]]


def reference_stereo(scene, variant, idx1, idx2):
    """(status [n], pos [n, 3], info) of the `_stereo` forms: info["path"] 0 = no stereo observation (new_points_scene's reference), 1 = triangulated,
    2 / 3 = unprojected from key frame 1 / 2, -1 = left to the host; info["three"] = the three-term error over sigma2 in key frame 1 where it was
    evaluated, info["two"] = its first two terms over sigma2, info["cosr"] = cosParallaxRays of the stereo pairs."""
    L = N._oracle()
    V = scene["variants"][variant]
    kf1, kf2 = scene["key_frames"]
    n = len(idx1)
    status, pos = N.reference_new_points(scene, variant, idx1, idx2)      # every pair without a stereo observation: final
    status, pos = status.copy(), pos.copy()
    info = dict(path=np.zeros(n, np.int8), three=np.full(n, np.nan), two=np.full(n, np.nan), cosr=np.full(n, np.nan, f32))
    ratioFactor, one = f32(V["ratio_factor"]), f32(1)
    with np.errstate(all="ignore"):
        for q in range(n):
            if status[q] != N.STEREO_LEFT_TO_HOST:
                continue
            i1, i2 = int(idx1[q]), int(idx2[q])
            st1, st2 = bool(kf1["u_right"][i1] >= 0), bool(kf2["u_right"][i2] >= 0)
            if (st1 and kf1.get("depth") is None) or (st2 and kf2.get("depth") is None):
                info["path"][q] = -1
                continue
            x1, y1, o1, _ = N.feature(kf1, i1)
            x2, y2, o2, _ = N.feature(kf2, i2)
            v1, v2 = V["views"][0][0], V["views"][1][0]
            R1, t1, R2, t2 = v1["R"], v1["t"], v2["R"], v2["t"]
            a, b = N._unproject(L, v1["p"], x1, y1)
            c, d = N._unproject(L, v2["p"], x2, y2)
            ray1 = [N._dot3(R1[0, r], R1[1, r], R1[2, r], a, b, one) for r in range(3)]
            ray2 = [N._dot3(R2[0, r], R2[1, r], R2[2, r], c, d, one) for r in range(3)]
            n1, n2 = f32(np.sqrt(N._dot3(*ray1, *ray1))), f32(np.sqrt(N._dot3(*ray2, *ray2)))
            cosr = f32(N._dot3(*ray1, *ray2) / f32(n1 * n2))
            info["cosr"][q] = cosr
            cs1 = cs2 = f32(cosr + one)
            if st1:
                cs1 = _cos_parallax_stereo(V["mb"][0], kf1["depth"][i1])
            else:
                cs2 = _cos_parallax_stereo(V["mb"][1], kf2["depth"][i2])
            cs = cs2 if cs2 < cs1 else cs1                                   # std::min(a, b)
            if cosr < cs and cosr > 0:                                       # (bStereo1 || bStereo2 holds)
                A = np.zeros((4, 4), f32)
                for j in range(4):
                    T1 = (R1[0, j], R1[1, j], R1[2, j]) if j < 3 else (t1[0], t1[1], t1[2])
                    T2 = (R2[0, j], R2[1, j], R2[2, j]) if j < 3 else (t2[0], t2[1], t2[2])
                    A[0, j] = f32(f32(a * T1[2]) - T1[0]); A[1, j] = f32(f32(b * T1[2]) - T1[1])
                    A[2, j] = f32(f32(c * T2[2]) - T2[0]); A[3, j] = f32(f32(d * T2[2]) - T2[1])
                Vm = np.zeros(16, f32)
                L.orbo_eigen_jacobi_svd4_V(A.ctypes.data, Vm.ctypes.data, None)
                if Vm[15] == 0:
                    status[q] = N.TRIANGULATE_FAILED
                    continue
                X = [f32(Vm[3] / Vm[15]), f32(Vm[7] / Vm[15]), f32(Vm[11] / Vm[15])]
                info["path"][q] = 1
            elif st1 and cs1 < cs2:
                X = _unproject_kf(kf1, v1, i1)
                info["path"][q] = 2
            elif st2 and cs2 < cs1:
                X = _unproject_kf(kf2, v2, i2)
                info["path"][q] = 3
            else:
                status[q] = N.LOW_PARALLAX
                continue
            if X is None:
                status[q] = UNPROJECT_FAILED
                continue
            z1 = f32(N._dot3(R1[2, 0], R1[2, 1], R1[2, 2], *X) + t1[2])
            if z1 <= 0:
                status[q] = N.BEHIND_1
                continue
            z2 = f32(N._dot3(R2[2, 0], R2[2, 1], R2[2, 2], *X) + t2[2])
            if z2 <= 0:
                status[q] = N.BEHIND_2
                continue
            rejected = False
            for k, (R, t, v, z, x, y, o, st, kf, i) in enumerate(((R1, t1, v1, z1, x1, y1, o1, st1, kf1, i1), (R2, t2, v2, z2, x2, y2, o2, st2, kf2, i2))):
                px = f32(N._dot3(R[0, 0], R[0, 1], R[0, 2], *X) + t[0]); py = f32(N._dot3(R[1, 0], R[1, 1], R[1, 2], *X) + t[1])
                sigma2 = float(kf["sigma2"][o])
                if st:
                    invz = f32(one / z)
                    u = f32(f32(f32(v["p"][0] * px) * invz) + v["p"][2])
                    u_r = f32(u - f32(V["mbf"][k] * invz))
                    vv = f32(f32(f32(v["p"][1] * py) * invz) + v["p"][3])
                    ex, ey, er = f32(u - x), f32(vv - y), f32(u_r - kf["u_right"][i])
                    two = f32(f32(ex * ex) + f32(ey * ey))
                    three = f32(two + f32(er * er))
                    if k == 0:
                        info["three"][q], info["two"][q] = float(three) / sigma2, float(two) / sigma2
                    bad = float(three) > 7.8 * sigma2
                else:
                    u, vv = N._project(L, v["p"], px, py, z)
                    ex, ey = f32(u - x), f32(vv - y)
                    bad = float(f32(f32(ex * ex) + f32(ey * ey))) > 5.991 * sigma2
                if bad:
                    status[q] = N.REPROJ_1 + k
                    rejected = True
                    break
            if rejected:
                continue
            d1 = [f32(X[k] - v1["Ow"][k]) for k in range(3)]
            d2 = [f32(X[k] - v2["Ow"][k]) for k in range(3)]
            dist1, dist2 = f32(np.sqrt(N._dot3(*d1, *d1))), f32(np.sqrt(N._dot3(*d2, *d2)))
            if dist1 == 0 or dist2 == 0:
                status[q] = N.ZERO_DIST
                continue
            th = f32(V["th_far_points"])
            if V["far_points"] and (dist1 >= th or dist2 >= th):
                status[q] = N.FAR
                continue
            ratioDist, ratioOctave = f32(dist2 / dist1), f32(kf1["scale"][o1] / kf2["scale"][o2])
            if f32(ratioDist * ratioFactor) < ratioOctave or ratioDist > f32(ratioOctave * ratioFactor):
                status[q] = N.SCALE_RATIO
                continue
            status[q] = N.OK
            pos[q] = X
    return status, pos, info


def _make_stereo(seed):
    L = N._oracle()
    base = N.make_scene(seed, False)
    rng = np.random.default_rng(1000 + seed)
    kfs = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kf.items()} for kf in base["key_frames"]]   # the shared scene stays as it is
    views = base["variants"]["base"]["views"]
    W, H = base["W"], base["H"]
    fx = f32(N.MONO_CAM[0])
    for kf in kfs:
        n = len(kf["x"])
        disp = kf["x"] - kf["u_right"]
        kf["depth"] = np.where(kf["u_right"] >= 0, MBF / np.where(disp > 0, disp, 1).astype(f32), f32(-1)).astype(f32)   # the base scene's stereo pairs
        off = np.where(rng.random((n, 1)) < 0.5, rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(0.3, 1.5, (n, 2)), 0.0)
        kf["keys_xy"] = (np.stack([kf["x"], kf["y"]], axis=1) + off).astype(f32)                                      # raw != undistorted on about half
    free = [sorted(set(range(len(kf["x"]))) - set(ix.tolist())) for kf, ix in zip(kfs, (base["idx1"], base["idx2"][base["idx2"] >= 0]))]
    for fr in free:
        rng.shuffle(fr)
    O = [views[k][0]["Ow"].astype(np.float64) for k in range(2)]
    axis = (O[1] - O[0]) / np.linalg.norm(O[1] - O[0])
    # the `turned` variant: key frame 2 looks sideways (about the y axis), so that rays of the two key frames can be perpendicular
    Rt = N._rot(0.0, 1.5, 0.0) @ views[1][0]["R"].astype(np.float64)
    turned = [list(views[0]), [N._view(Rt, O[1], N.MONO_CAM)]]

    def inside(u, v):
        return 8 < u < W - 8 and 8 < v < H - 8

    def set_feature(k, i, u, v, level, depth=None, ur_noise=0.0):
        kf = kfs[k]
        kf["x"][i], kf["y"][i], kf["octave"][i] = f32(u), f32(v), level
        d = rng.uniform(-1.2, 1.2, 2) if rng.random() < 0.5 else np.zeros(2)
        kf["keys_xy"][i] = (f32(u) + f32(d[0]), f32(v) + f32(d[1]))
        if depth is None:
            kf["u_right"][i], kf["depth"][i] = -1, -1
        else:
            kf["depth"][i] = f32(depth)
            kf["u_right"][i] = f32(f32(u) - (MBF / f32(depth) if depth > 0 else f32(10)) + f32(ur_noise))

    pairs, kinds = [], []
    want = {c: PER_CLASS for c in CLASSES}
    guard = 0
    while any(want.values()) and guard < 4000:
        guard += 1
        kind = [c for c in CLASSES if want[c]][0]
        i1, i2 = free[0][-1], free[1][-1]
        lv = [int(rng.integers(0, 3)), int(rng.integers(0, 3))]
        noise = rng.normal(0, 0.1, (2, 2))
        depth_noise = 1.0 + rng.normal(0, 0.002)
        if kind.startswith("a"):                              # an ordinary point of the cloud: ample ray parallax
            z = rng.uniform(3.0, 7.0)
            P = 0.5 * (O[0] + O[1]) + np.array([rng.uniform(-0.45, 0.45) * z, rng.uniform(-0.35, 0.35) * z, z])
        elif kind in ("f",):                                  # far away: the rays are nearly parallel
            z = rng.uniform(150.0, 400.0)
            P = 0.5 * (O[0] + O[1]) + np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.25, 0.25) * z, z])
        elif kind == "e_turned":
            P = None
        elif kind == "h_behind":                              # unprojected a little in front of key frame 1: behind key frame 2
            e = rng.normal(0, 1, 3)
            e -= axis * (e @ axis)
            P = O[0] + rng.uniform(0.25, 0.5) * axis + 0.004 * e / np.linalg.norm(e)
        else:                                                 # near the line through both centres, beyond key frame 2: low ray parallax
            e = rng.normal(0, 1, 3)
            e -= axis * (e @ axis)
            P = O[1] + rng.uniform(3.0, 6.0) * axis + rng.uniform(0.02, 0.12) * e / np.linalg.norm(e)
        if P is not None:
            uv = [N._image(L, views[k][0], P) for k in range(2)]
            zc = [float(N._cam(views[k][0], P)[2]) for k in range(2)]
        else:
            # key point 1 anywhere, key point 2 on a ray (of the TURNED key frame 2) at a chosen cosine <= 0 to ray 1
            u1, v1 = rng.uniform(100, W - 100), rng.uniform(100, H - 100)
            r1 = views[0][0]["R"].astype(np.float64).T @ np.array([(u1 - N.MONO_CAM[2]) / N.MONO_CAM[0], (v1 - N.MONO_CAM[3]) / N.MONO_CAM[1], 1.0])
            r1 /= np.linalg.norm(r1)
            a2 = Rt.T @ np.array([0.0, 0.0, 1.0])
            perp = a2 - (a2 @ r1) * r1
            perp /= np.linalg.norm(perp)
            cosine = -[0.001, 0.002, 0.006, 0.012, 0.3, 0.5, 0.004, 0.6][want[kind] - 1]
            r2 = np.sqrt(1 - cosine * cosine) * perp + cosine * r1
            c2 = Rt @ r2
            uv = [(f32(u1), f32(v1)), (f32(N.MONO_CAM[0] * c2[0] / c2[2] + N.MONO_CAM[2]), f32(N.MONO_CAM[1] * c2[1] / c2[2] + N.MONO_CAM[3]))]
            zc = [0.5, 0.5]
            if c2[2] <= 0:
                continue
        if not (inside(*uv[0]) and inside(*uv[1])):
            continue
        if P is not None and kind != "f":                     # the class's parallax by a margin: the angle between the rays against the stereo angle
            ra, rb = P - O[0], P - O[1]
            ang = np.arccos(np.clip(ra @ rb / np.linalg.norm(ra) / np.linalg.norm(rb), -1, 1))
            if (kind.startswith("a") and ang < 3 * float(MB) / min(abs(zc[0]), abs(zc[1]))) or \
               (not kind.startswith("a") and kind != "h_behind" and ang > 0.4 * float(MB) / max(abs(zc[0]), abs(zc[1]))):
                continue
        d1 = d2 = None
        n1 = n2 = 0.0
        if kind == "a_between":                              # accepted although the three-term error exceeds 5.991 sigma2: it stays below 7.8 sigma2
            lv[0] = int(rng.integers(0, 3))
            d1, n1 = zc[0] * depth_noise, 2.6 * float(kfs[0]["scale"][lv[0]])
            noise[:] = rng.normal(0, 0.03, (2, 2))
        elif kind == "a_reproj_r":                           # rejected through the right coordinate alone
            d1, n1 = zc[0] * depth_noise, rng.choice([-1.0, 1.0]) * 3.3 * float(kfs[0]["scale"][lv[0]])
            noise[:] = rng.normal(0, 0.03, (2, 2))
        elif kind in ("a_plain", "b"):
            d1, n1 = zc[0] * depth_noise, rng.normal(0, 0.2)
        elif kind == "c":
            d2, n2 = zc[1] * depth_noise, rng.normal(0, 0.2)
        elif kind == "d":
            d1, d2, n1, n2 = zc[0] * depth_noise, zc[1] * depth_noise, rng.normal(0, 0.2), rng.normal(0, 0.2)
        elif kind == "e_turned":
            d1 = 0.5
        elif kind == "f":
            d1 = [0.0, -1.0, -0.0, -3.5][want[kind] % 4]
        elif kind == "h_reproj_2":
            d1, lv = zc[0] * depth_noise, [0, 0]
            noise[1] = rng.choice([-1.0, 1.0], 2) * rng.uniform(4.0, 6.0, 2)
        elif kind == "h_behind":
            d1 = abs(zc[0]) * depth_noise
        elif kind == "h_scale":
            d1, lv = zc[0] * depth_noise, [7, 0]
        set_feature(0, i1, uv[0][0] + f32(noise[0][0]), uv[0][1] + f32(noise[0][1]), lv[0], d1, n1)
        set_feature(1, i2, uv[1][0] + f32(noise[1][0]), uv[1][1] + f32(noise[1][1]), lv[1], d2, n2)
        if kind == "c" and want[kind] > 2:                    # unprojected from key frame 2's RAW key point, which differs from the undistorted one
            kfs[1]["keys_xy"][i2] = kfs[1]["keys_xy"][i2] + f32([0.75, -0.5])
        free[0].pop(); free[1].pop()
        pairs.append((i1, i2)); kinds.append(kind)
        want[kind] -= 1
    assert not any(want.values()), want
    # round robin over the classes, so that a prefix holds some of each; then the base scene's pairs (class (g) among them)
    by_class = {c: [k for k in range(len(pairs)) if kinds[k] == c] for c in CLASSES}
    order = [by_class[c][j] for j in range(PER_CLASS) for c in CLASSES]
    idx1 = np.concatenate([[pairs[o][0] for o in order], base["idx1"]]).astype(np.int32)
    idx2 = np.concatenate([[pairs[o][1] for o in order], base["idx2"]]).astype(np.int32)
    all_kinds = [kinds[o] for o in order] + ["g:" + k for k in base["kinds"]]
    for kf in kfs:
        from orb_slam3_amd import KP_DTYPE
        kp = np.zeros(len(kf["x"]), KP_DTYPE)
        kp["x"], kp["y"], kp["octave"] = kf["x"], kf["y"], kf["octave"]
        kp["size"], kp["class_id"] = 31.0, -1
        kf["kps"], kf["kps_right"] = kp, kp[:0].copy()
    b = dict(base["variants"]["base"], mb=(MB, MB), mbf=(MBF, MBF))
    shifted = [[dict(views[0][0], t=(views[0][0]["t"] - f32([0, 0, 10])).astype(f32))], list(views[1])]   # tcw1 inconsistent with Ow1: z1 = depth - 10
    variants = dict(base=b, inertial=dict(b, inertial=1), far=dict(b, far_points=1, th_far_points=N.FAR_THRESHOLD), turned=dict(b, views=turned),
                    shifted=dict(b, views=shifted), other_rig=dict(b, mb=(f32(0.54), MB), mbf=(f32(0.54) * fx, f32(MBF * f32(1.5)))))
    return dict(rig=False, W=W, H=H, key_frames=kfs, idx1=idx1, idx2=idx2, kinds=all_kinds, variants=variants, n_designed=len(order))


_STEREO_SCENES, _STEREO_REFS = {}, {}


def make_stereo_scene(seed):
    if seed not in _STEREO_SCENES:
        _STEREO_SCENES[seed] = _make_stereo(seed)
    return _STEREO_SCENES[seed]


def stereo_reference(scene, variant):
    """reference_stereo over all pairs of the scene, once per (scene, variant); a prefix of the pairs has a prefix of it."""
    key = (id(scene), variant)
    if key not in _STEREO_REFS:
        _STEREO_REFS[key] = reference_stereo(scene, variant, scene["idx1"], scene["idx2"])
    return _STEREO_REFS[key]


def stereo_key_frames(osa, m, scene, depth=(True, True)):
    """The two key frames from host arrays: with mvDepth and the raw key points (create_host_stereo), or as they were before (from_host)."""
    out = []
    for kf, with_depth in zip(scene["key_frames"], depth):
        view = osa.FrameView(kf["kps"], kf["desc"], 0.0, scene["W"], 0.0, scene["H"], kf["scale"], kf["u_right"])
        out.append(osa.DeviceKeyFrame.create_host_stereo(m, view, kf["depth"], kf["keys_xy"], None) if with_depth else osa.DeviceKeyFrame.from_host(m, view, None))
    return out


def stereo_call(scene, variant):
    """The arguments of TriangulatePairsKeyFramesStereo between the key frames and the pairs."""
    V = scene["variants"][variant]
    v1, v2 = N.call_views(scene, variant)
    p = N.call_params(scene, variant)
    return (v1, v2, p["level_sigma2_1"], p["level_sigma2_2"], p["ratio_factor"], float(V["mb"][0]), float(V["mbf"][0]), float(V["mb"][1]), float(V["mbf"][1])), \
        (p["inertial"], p["far_points"], p["th_far_points"])


def check_conditions_stereo(scene):
    """What the key-frame tests demand of the scene, from the reference alone.  Returns, for the caller's test over the seeds, the verdicts of class (e)."""
    kf1, kf2 = scene["key_frames"]
    idx1, idx2, kinds = scene["idx1"], scene["idx2"], np.array(scene["kinds"])
    assert (len(kf1["x"]), len(kf2["x"])) == N.MONO_N and (len(kf1["scale"]), len(kf2["scale"])) == (8, 5)
    for kf in (kf1, kf2):
        differs = (kf["keys_xy"] != np.stack([kf["x"], kf["y"]], axis=1)).any(axis=1)
        assert 0.35 < differs.mean() < 0.65, differs.mean()
    st, pos, info = stereo_reference(scene, "base")
    assert not np.isnan(pos[st == N.OK]).any()
    s1, s2 = kf1["u_right"][idx1] >= 0, np.where(idx2 >= 0, kf2["u_right"][np.maximum(idx2, 0)] >= 0, False)

    def of(kind):
        sel = kinds == kind
        assert sel.sum() >= PER_CLASS, kind
        return sel
    for kind in ("a_between", "a_reproj_r", "a_plain"):       # (a) stereo on 1 only, triangulated
        sel = of(kind)
        assert (s1[sel] & ~s2[sel]).all() and (info["path"][sel] == 1).all(), kind
    sel = of("a_between")
    assert ((st[sel] == N.OK) & (info["three"][sel] > 5.991) & (info["three"][sel] < 7.8)).sum() >= 5, (st[sel], info["three"][sel])
    sel = of("a_reproj_r")
    assert ((st[sel] == N.REPROJ_1) & (info["two"][sel] < 5.991)).sum() >= 5, (st[sel], info["two"][sel])
    sel = of("b")                                             # (b) stereo on 1 only, unprojected from key frame 1
    assert (s1[sel] & ~s2[sel]).all() and (info["path"][sel] == 2).all() and (st[sel] == N.OK).sum() >= 5, (info["path"][sel], st[sel])
    sel = of("c")                                             # (c) stereo on 2 only, unprojected from key frame 2, the raw key point differs
    assert (~s1[sel] & s2[sel]).all() and (info["path"][sel] == 3).all() and (st[sel] == N.OK).sum() >= 5, (info["path"][sel], st[sel])
    raw = kf2["keys_xy"][idx2[sel]]
    un = np.stack([kf2["x"][idx2[sel]], kf2["y"][idx2[sel]]], axis=1)
    moved, _ = reference_unproject(un, kf2["depth"][idx2[sel]], scene["variants"]["base"]["views"][1][0])
    ok = st[sel] == N.OK
    assert ((raw != un).any(axis=1) & ok & (bits(moved) != bits(pos[sel])).any(axis=1)).sum() >= 5
    sel = of("d")                                             # (d) stereo on both, depth2 < depth1: the member's `else if` unprojects from key frame 1
    assert (s1[sel] & s2[sel]).all() and (kf2["depth"][idx2[sel]] < kf1["depth"][idx1[sel]]).all() and (info["path"][sel] == 2).all(), info["path"][sel]
    sel = of("f")                                             # (f) mvuRight >= 0, depth <= 0
    assert s1[sel].all() and (kf1["depth"][idx1[sel]] <= 0).all() and (st[sel] == UNPROJECT_FAILED).all(), st[sel]
    g = (~s1) & (~s2) & (idx2 >= 0)                           # (g) no stereo observation: new_points_scene's reference, the existing call's bits
    assert g.sum() >= 100 and (info["path"][g] == 0).all() and (st[g] == N.OK).sum() >= 50
    for kind, status in (("h_reproj_2", N.REPROJ_2), ("h_behind", N.BEHIND_2), ("h_scale", N.SCALE_RATIO)):   # (h) reached from an unprojected point
        sel = of(kind)
        assert ((info["path"][sel] == 2) & (st[sel] == status)).sum() >= 5, (kind, info["path"][sel], st[sel])
    sst, _, sinfo = stereo_reference(scene, "shifted")
    assert ((sinfo["path"] == 2) & (sst == N.BEHIND_1)).sum() >= 5
    tst, _, tinfo = stereo_reference(scene, "turned")         # (e) cosParallaxRays <= 0 with a stereo observation
    sel = of("e_turned")
    assert (tinfo["cosr"][sel] <= 0).all(), tinfo["cosr"][sel]
    # every prefix the tests use holds some of every class
    for n in PAIR_COUNTS:
        if n >= len(CLASSES) * 5:
            assert all((kinds[:n] == c).sum() >= 5 for c in CLASSES), n
    ost = stereo_reference(scene, "other_rig")[0]
    assert (ost != st).sum() >= 3                             # mb / mbf enter the verdicts
    return {int(s) for s in tst[sel]}
