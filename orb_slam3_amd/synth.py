"""Seeded synthetic frame generator.

No dataset is available offline, so every config of BASELINE.json runs on synthetic
camera-like frames: a large canvas (smooth background + random filled convex quads of
random grey levels, i.e. plenty of FAST corners at every pyramid scale) from which frame t
is the crop at offset (2t, t) plus per-frame Gaussian sensor noise.  Pure numpy; used by
tests, bench.py and __graft_entry__.smoke().
"""
from __future__ import annotations

import numpy as np

__all__ = ["make_canvas", "make_texture_canvas", "frame_from_canvas", "make_frames", "make_stereo_pair", "make_test_image"]


def _bilinear_upsample(small: np.ndarray, size: int) -> np.ndarray:
    n = small.shape[0]
    xs = np.linspace(0, n - 1, size)
    x0 = np.clip(np.floor(xs).astype(int), 0, n - 2)
    fx = (xs - x0).astype(np.float32)
    wmat = np.zeros((size, n), np.float32)  # interpolation matrix, 2 non-zeros per row
    wmat[np.arange(size), x0] = 1 - fx
    wmat[np.arange(size), x0 + 1] += fx
    return wmat @ small.astype(np.float32) @ wmat.T


def make_canvas(seed: int, size: int = 2048, n_shapes: int = 2400) -> np.ndarray:
    """float32 canvas in [0,255]: background + `n_shapes` random filled convex quads."""
    rng = np.random.default_rng(seed)
    canvas = _bilinear_upsample(rng.uniform(40, 215, (32, 32)), size).astype(np.float32)
    for _ in range(n_shapes):
        cx, cy = rng.uniform(0, size, 2)
        half = rng.uniform(4, 48, 2)
        ang = rng.uniform(0, np.pi)
        grey = rng.uniform(0, 255)
        skew = rng.uniform(0.7, 1.3, 4)
        # 4 corners of a skewed rotated rectangle (convex)
        base = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64) * half * skew[:, None]
        c, s = np.cos(ang), np.sin(ang)
        pts = base @ np.array([[c, s], [-s, c]]) + (cx, cy)
        x0 = int(max(0, np.floor(pts[:, 0].min())))
        x1 = int(min(size, np.ceil(pts[:, 0].max()) + 1))
        y0 = int(max(0, np.floor(pts[:, 1].min())))
        y1 = int(min(size, np.ceil(pts[:, 1].max()) + 1))
        if x1 <= x0 or y1 <= y0:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        inside = np.ones(xx.shape, dtype=bool)
        for k in range(4):
            ax, ay = pts[k]
            bx, by = pts[(k + 1) % 4]
            inside &= ((bx - ax) * (yy - ay) - (by - ay) * (xx - ax)) >= 0
        canvas[y0:y1, x0:x1][inside] = grey
    return canvas


def make_texture_canvas(seed: int, size: int = 2048) -> np.ndarray:
    """float32 canvas in [0,255] with NATURAL-IMAGE statistics instead of flat quads: 1/f ("pink") noise -- the amplitude spectrum of natural
    scenes -- at high contrast, plus a dense layer of small high-contrast texture elements (speckles, short strokes, checker patches: foliage /
    gravel / brick-like detail).  Several times the FAST candidates of make_canvas per frame, corners crowded next to each other (NMS ties,
    full candidate queues), few flat cells.  The stress scene of the constants the kernels were tuned on the quad scene with (queue
    capacities, quad-tree tier thresholds, the share of cells that take the minThFAST pass)."""
    rng = np.random.default_rng(seed)
    fy = np.fft.fftfreq(size)[:, None]
    fx = np.fft.rfftfreq(size)[None, :]
    f = np.sqrt(fx * fx + fy * fy)
    f[0, 0] = 1.0
    spec = (rng.normal(size=f.shape) + 1j * rng.normal(size=f.shape)) / f       # amplitude ~ 1 / f
    spec[0, 0] = 0.0
    pink = np.fft.irfft2(spec, s=(size, size)).astype(np.float32)
    pink = (pink - pink.mean()) / (pink.std() + 1e-9)
    canvas = np.clip(128.0 + 46.0 * pink, 0, 255).astype(np.float32)
    # dense texture elements: ~1 per 12 x 12 px
    n_el = (size // 12) ** 2
    cx = rng.integers(2, size - 10, n_el)
    cy = rng.integers(2, size - 10, n_el)
    kind = rng.integers(0, 3, n_el)
    grey = np.where(rng.random(n_el) < 0.5, rng.uniform(0, 70, n_el), rng.uniform(185, 255, n_el)).astype(np.float32)
    ew = rng.integers(1, 6, n_el)
    eh = rng.integers(1, 6, n_el)
    for i in range(n_el):
        x, y = int(cx[i]), int(cy[i])
        if kind[i] == 0:      # speckle / blob
            canvas[y:y + eh[i], x:x + ew[i]] = grey[i]
        elif kind[i] == 1:    # short stroke
            if ew[i] >= eh[i]:
                canvas[y:y + 1 + (eh[i] > 3), x:x + 2 * ew[i]] = grey[i]
            else:
                canvas[y:y + 2 * eh[i], x:x + 1 + (ew[i] > 3)] = grey[i]
        else:                 # 2 x 2 checker of cells ew x eh
            canvas[y:y + eh[i], x:x + ew[i]] = grey[i]
            canvas[y + eh[i]:y + 2 * eh[i], x + ew[i]:x + 2 * ew[i]] = grey[i]
            canvas[y:y + eh[i], x + ew[i]:x + 2 * ew[i]] = 255.0 - grey[i]
            canvas[y + eh[i]:y + 2 * eh[i], x:x + ew[i]] = 255.0 - grey[i]
    return canvas


def frame_from_canvas(canvas: np.ndarray, t: int, w: int, h: int, noise_seed: int, sigma: float = 3.0,
                      dx: int = 2, dy: int = 1, x0: int = 0, y0: int = 0) -> np.ndarray:
    size = canvas.shape[0]
    ox = (x0 + dx * t) % (size - w)
    oy = (y0 + dy * t) % (size - h)
    crop = canvas[oy:oy + h, ox:ox + w]
    rng = np.random.default_rng(noise_seed)
    noisy = crop + rng.normal(0.0, sigma, crop.shape).astype(np.float32)
    return np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


def make_frames(seed: int, n: int, w: int, h: int, canvas: np.ndarray | None = None) -> np.ndarray:
    """(n, h, w) uint8 frames of scene `seed` (frame t = crop at (2t, t) + noise seeded 1000*seed+t)."""
    if canvas is None:
        canvas = make_canvas(seed, size=max(2048, 2 * max(w, h)))
    return np.stack([frame_from_canvas(canvas, t, w, h, 1000 * seed + t) for t in range(n)])


def make_stereo_pair(seed: int, t: int, w: int, h: int, canvas: np.ndarray | None = None):
    """Rectified stereo pair: the right image sees the canvas shifted by a per-band disparity."""
    if canvas is None:
        canvas = make_canvas(seed, size=max(2048, 2 * max(w, h)))
    left = frame_from_canvas(canvas, t, w, h, 3000 + t, x0=128)
    right = np.empty_like(left)
    bands = [8, 16, 32, 64]
    bh = h // len(bands)
    for k, d in enumerate(bands):
        ys = slice(k * bh, h if k == len(bands) - 1 else (k + 1) * bh)
        full = frame_from_canvas(canvas, t, w, h, 4000 + t, x0=128 + d)
        right[ys] = full[ys]
    return left, right


def make_test_image(seed: int, w: int, h: int) -> np.ndarray:
    """Small structured + noisy image for unit tests (fast to build)."""
    canvas = make_canvas(seed, size=max(512, 2 * max(w, h)), n_shapes=150)
    return frame_from_canvas(canvas, 0, w, h, seed + 77)


def make_scene_canvas(scene: str, seed: int, size: int = 2048) -> np.ndarray:
    """Canvas by scene name: "quads" (make_canvas: SURVEY.md 8(d)'s scene, the metric), "texture" (make_texture_canvas: 13 x the FAST candidates), or
    "blend:<a>" with 0 <= a <= 1: (1 - a) * quads + a * texture, pixel by pixel -- candidate densities in between (bench.py --scene, tools/density_sweep.sh)."""
    if scene == "quads":
        return make_canvas(seed, size=size) if size != 2048 else make_canvas(seed)
    if scene == "texture":
        return make_texture_canvas(seed, size)
    if scene.startswith("blend:"):
        a = float(scene.split(":", 1)[1])
        if not 0.0 <= a <= 1.0:
            raise ValueError("blend factor must lie in [0, 1]")
        q = make_canvas(seed, size=size) if size != 2048 else make_canvas(seed)
        t = make_texture_canvas(seed, size)
        return ((1.0 - a) * q.astype(np.float32) + a * t.astype(np.float32)).astype(np.float32)
    raise ValueError(f"unknown scene {scene!r}")


# Examples/Stereo/TUM-VI.yaml Camera1 / Camera2: fx, fy, cx, cy, k0..k3 (KannalaBrandt8::mvParameters)
TUMVI_L = (190.978477, 190.973307, 254.931706, 256.897442, 0.0034823894, 0.0007150348, -0.0020532361, 0.0002029367)
TUMVI_R = (190.442369, 190.434438, 252.598164, 254.917230, 0.0034003171, 0.0017669271, -0.0026631290, 0.0003299517)


def make_fisheye_keyframes(rng, n_pts: int = 420, with_poses: bool = False):
    """Two key frames of a TUM-VI-like fisheye rig looking at common 3-D points: features = mvKeys | mvKeysRight, descriptors noisy copies of the point's,
    and the four relative poses of ORBmatcher.cc:934-944 (ll, lr, rl, rr).  Returns (k1, n_left1, d1, id1, k2, n_left2, d2, id2, R12, t12, cams)."""
    from . import KP_DTYPE

    def rot(a):
        ax, ay, az = a
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        return Rz @ Ry @ Rx

    def se3(R, t):
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
        return T
    Trl = se3(rot(rng.uniform(-0.01, 0.01, 3)), [-0.101, 0.002, 0.001])     # right camera from left camera
    Tw2 = se3(rot(rng.uniform(-0.04, 0.04, 3)), [0.25, 0.03, -0.02])         # KF2's left camera in the world = KF1's left camera frame (T1w = I)
    Tlr = np.linalg.inv(Trl)
    pair = [Tw2, Tw2 @ Tlr, Trl @ Tw2, Trl @ Tw2 @ Tlr]                      # Tll, Tlr, Trl, Trr: x_cam1 = T * x_cam2
    R12 = np.stack([T[:3, :3] for T in pair]).astype(np.float32)
    t12 = np.stack([T[:3, 3] for T in pair]).astype(np.float32)
    P = np.stack([rng.uniform(-3, 3, n_pts), rng.uniform(-3, 3, n_pts), rng.uniform(1.0, 8, n_pts), np.ones(n_pts)], axis=1)
    pdesc = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)

    def proj(prm, X):
        th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2]); psi = np.arctan2(X[:, 1], X[:, 0])
        r = th + prm[4] * th ** 3 + prm[5] * th ** 5 + prm[6] * th ** 7 + prm[7] * th ** 9
        return np.stack([prm[0] * r * np.cos(psi) + prm[2], prm[1] * r * np.sin(psi) + prm[3]], axis=1)

    def keyframe(Tcw_left):
        parts, ids = [], []
        for T, prm in ((Tcw_left, TUMVI_L), (Trl @ Tcw_left, TUMVI_R)):
            X = (T @ P.T).T[:, :3]
            uv = proj(prm, X) + rng.choice([0.2, 1.0, 5.0], n_pts)[:, None] * rng.uniform(-1, 1, (n_pts, 2))
            seen = np.nonzero((rng.random(n_pts) < 0.7) & (uv[:, 0] > 5) & (uv[:, 0] < 507) & (uv[:, 1] > 5) & (uv[:, 1] < 507))[0]
            k = np.zeros(len(seen), KP_DTYPE)
            k["x"], k["y"] = uv[seen, 0], uv[seen, 1]
            k["octave"] = rng.integers(0, 8, len(seen))
            k["angle"] = rng.uniform(0, 360, len(seen))
            k["size"], k["class_id"] = 31.0, -1
            parts.append(k); ids.append(seen)
        kps = np.concatenate(parts)
        pid = np.concatenate(ids)
        flip = rng.random((len(pid), 256)) < 0.04
        return kps, len(parts[0]), pdesc[pid] ^ np.packbits(flip, axis=1, bitorder="little"), pid
    k1, nl1, d1, id1 = keyframe(np.eye(4))
    k2, nl2, d2, id2 = keyframe(np.linalg.inv(Tw2))
    out = (k1, nl1, d1, id1, k2, nl2, d2, id2, R12, t12, np.array([TUMVI_L, TUMVI_R], np.float32))
    if with_poses:   # Tcw of the two left cameras and Trl, each (R, t) in float32: what a KeyFrame holds (GetPose, GetRelativePoseTrl)
        T2w = np.linalg.inv(Tw2)
        f = lambda T: (T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32))
        out += (dict(pose1=f(np.eye(4)), pose2=f(T2w), trl=f(Trl)),)
    return out


def make_fisheye_stereo_frame(rng, n_pts: int = 1500, n_left: int | None = None, n_right: int | None = None, mono_left: int = 0, mono_right: int = 0,
                              flip: float = 0.04):
    """One frame of a TUM-VI-like fisheye rig (make_fisheye_keyframes' first key frame): mvKeys / mvKeysRight with their descriptors, arranged as
    ORBextractor leaves them -- the features outside the lapping area first, the lapping-area tail last (monoLeft / monoRight).  The left tail holds points
    seen by both cameras; the right tail holds as many of those same points as fit (in another order), then others.  Descriptors: one random descriptor
    per 3-D point, each feature's a copy with `flip` of its bits flipped (flip = 0: true correspondents have EQUAL descriptors, unrelated ones distinct).
    n_left / n_right default to the features there are; n_pts must be large enough for the sizes asked (ValueError otherwise).
    Returns (kl, dl, kr, dr, mono_left, mono_right, rig, id_left, id_right); rig = dict(cam_left, cam_right, R_lr, t_lr) (mRlr, mtlr: x_left = R_lr x_right + t_lr)."""
    k1, nl1, _, id1, _, _, _, _, _, _, cams, poses = make_fisheye_keyframes(rng, n_pts, with_poses=True)
    Rrl, trl = [np.asarray(x, np.float64) for x in poses["trl"]]
    R_lr = Rrl.T
    t_lr = -Rrl.T @ trl
    left, right = np.arange(nl1), np.arange(nl1, len(k1))
    n_left = len(left) if n_left is None else n_left
    n_right = len(right) if n_right is None else n_right
    if not (0 <= mono_left <= n_left and 0 <= mono_right <= n_right):
        raise ValueError("mono index outside [0, n]")
    nq, nt = n_left - mono_left, n_right - mono_right
    pos_r = {int(id1[j]): j for j in right}
    common = rng.permutation([i for i in left if int(id1[i]) in pos_r])
    only_l = rng.permutation([i for i in left if int(id1[i]) not in pos_r])
    tail_l = list(common[:nq]) + list(only_l[:max(0, nq - len(common))])
    used_l = set(tail_l)
    head_l = [i for i in rng.permutation(left) if i not in used_l][:mono_left]
    shared = [pos_r[int(id1[i])] for i in tail_l if int(id1[i]) in pos_r][:nt]
    used_r = set(shared)
    rest_r = [j for j in rng.permutation(right) if j not in used_r]
    tail_r = list(rng.permutation(shared + rest_r[:nt - len(shared)])) if nt else []
    used_r |= set(tail_r)
    head_r = [j for j in rest_r if j not in used_r][:mono_right]
    if len(tail_l) != nq or len(head_l) != mono_left or len(tail_r) != nt or len(head_r) != mono_right:
        raise ValueError(f"n_pts = {n_pts} too small for ({n_left}, {n_right}, {mono_left}, {mono_right})")
    il = np.array(head_l + list(rng.permutation(tail_l)), np.int64)
    ir = np.array(head_r + tail_r, np.int64)
    pdesc = rng.integers(0, 256, (int(id1.max()) + 1, 32), dtype=np.uint8)

    def desc(ids):
        d = pdesc[ids]
        if flip > 0:
            d = d ^ np.packbits(rng.random((len(ids), 256)) < flip, axis=1, bitorder="little")
        return np.ascontiguousarray(d)
    kl, kr = k1[il].copy(), k1[ir].copy()
    rig = dict(cam_left=cams[0].copy(), cam_right=cams[1].copy(), R_lr=R_lr.astype(np.float32), t_lr=t_lr.astype(np.float32))
    return kl, desc(id1[il]), kr, desc(id1[ir]), mono_left, mono_right, rig, id1[il].copy(), id1[ir].copy()


def make_fuse_scene(rng, n_kf: int = 20, n_mp: int = 1000, outliers: bool = True, n_clutter: int = 300, bounds=(0.0, 752.0, 0.0, 480.0),
                    nlevels: int = 8, scale_factor: float = 1.2):
    """A LocalMapping::SearchInNeighbors scene: n_mp map points seen from n_kf covisible key frames (EuRoC intrinsics, poses within about 0.5 m /
    0.06 rad of each other; key frame 0 has the identity pose).  Each key frame's features sit at 70 % of the map points' projections into it (0.8 px
    noise, 2 - 25 % flipped descriptor bits, octave = the level the distance predicts) plus n_clutter random ones; half of the features have u_right.
    outliers: 8 % of the points mirrored behind the cameras, 8 % with x * 2.5 (outside the image), 4 % with mfMaxDistance * 0.3, 4 % with mfMinDistance
    = 2 mfMaxDistance, 10 % with random normals -- one population per gate of ORBmatcher::Fuse.  bounds: one (minX, maxX, minY, maxY) for all key
    frames or one per key frame.  Feature placement uses a plain float64 projection: the exact gates are the caller's (or the library's) business.
    Returns dict(cams [n_kf] orbx_camera tuples, poses [n_kf] (Rcw, tcw, Ow) float32, bounds [n_kf, 4], scale_factors, inv_level_sigma2,
    log_scale_factor, map_points dict(pos, normal, min_dist, max_dist, desc), key_frames [n_kf] dict(kps KP_DTYPE, desc, u_right))."""
    from ._lib import KP_DTYPE
    f32 = np.float32
    fx, fy, cx, cy, bf = 458.654, 457.296, 367.215, 248.375, 47.9
    sf = (f32(scale_factor) ** np.arange(nlevels)).astype(f32)
    log_sf = float(np.log(f32(scale_factor)))
    b = np.broadcast_to(np.asarray(bounds, f32).reshape(-1, 4), (n_kf, 4)).copy()
    # map points in front of key frame 0, spread over its image
    z = rng.uniform(2.0, 12.0, n_mp)
    u0, v0 = rng.uniform(30, 720, n_mp), rng.uniform(30, 450, n_mp)
    pos = np.stack([(u0 - cx) / fx * z, (v0 - cy) / fy * z, z], axis=1)
    ref_dist = np.linalg.norm(pos, axis=1)
    ref_level = rng.integers(0, nlevels - 1, n_mp)
    max_d = ref_dist * sf[ref_level].astype(np.float64) * rng.uniform(0.95, 1.05, n_mp)
    min_d = max_d / float(sf[-1])
    normal = pos / ref_dist[:, None] + rng.normal(0, 0.15, pos.shape)   # MapPoint::mNormalVector: the mean viewing direction (camera -> point)
    normal = normal / np.linalg.norm(normal, axis=1, keepdims=True)
    if outliers:
        kind = rng.choice(6, n_mp, p=[0.66, 0.08, 0.08, 0.04, 0.04, 0.10])
        pos[kind == 1] *= -1.0
        pos[kind == 2, 0] *= 2.5
        max_d[kind == 3] *= 0.3
        min_d[kind == 3] = max_d[kind == 3] / float(sf[-1])
        min_d[kind == 4] = 2.0 * max_d[kind == 4]
        rn = rng.normal(0, 1, (int((kind == 5).sum()), 3))
        normal[kind == 5] = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    mp_desc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    pos, normal, min_d, max_d = pos.astype(f32), normal.astype(f32), min_d.astype(f32), max_d.astype(f32)
    cams, poses, kfs = [], [], []
    for k in range(n_kf):
        if k == 0:
            R, t = np.eye(3), np.zeros(3)
        else:
            w = rng.normal(0, 0.035, 3)
            th = np.linalg.norm(w)
            K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-12)
            R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
            t = rng.normal(0, 0.3, 3)
        Rcw, tcw = R.astype(f32), t.astype(f32)
        Ow = (-Rcw.astype(np.float64).T @ tcw.astype(np.float64)).astype(f32)
        cams.append((fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0, bf))
        poses.append((Rcw, tcw, Ow))
        # plain projection for the feature placement
        pc = pos.astype(np.float64) @ Rcw.astype(np.float64).T + tcw
        with np.errstate(divide="ignore", invalid="ignore"):
            uu, vv = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
        d3 = np.linalg.norm(pos.astype(np.float64) - Ow, axis=1)
        vis = (pc[:, 2] > 0) & (uu > b[k, 0] + 2) & (uu < b[k, 1] - 2) & (vv > b[k, 2] + 2) & (vv < b[k, 3] - 2)
        sel = np.nonzero(vis & (rng.random(n_mp) < 0.7))[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            lvl = np.clip(np.ceil(np.log(max_d[sel].astype(np.float64) / d3[sel]) / log_sf), 0, nlevels - 1).astype(np.int32)
        lvl = np.where(rng.random(len(sel)) < 0.25, np.maximum(lvl - 1, 0), lvl)
        n = len(sel) + n_clutter
        kp = np.zeros(n, KP_DTYPE)
        kp["x"][:len(sel)] = uu[sel] + rng.normal(0, 0.8, len(sel))
        kp["y"][:len(sel)] = vv[sel] + rng.normal(0, 0.8, len(sel))
        kp["octave"][:len(sel)] = lvl
        kp["x"][len(sel):] = rng.uniform(b[k, 0] + 1, b[k, 1] - 1, n_clutter)
        kp["y"][len(sel):] = rng.uniform(b[k, 2] + 1, b[k, 3] - 1, n_clutter)
        kp["octave"][len(sel):] = rng.integers(0, nlevels, n_clutter)
        kp["size"] = 31.0 * sf[kp["octave"]]
        kp["angle"] = rng.uniform(0, 360, n)
        kp["response"] = rng.integers(7, 200, n)
        kp["class_id"] = -1
        flip = rng.uniform(0.02, 0.25, len(sel))[:, None]
        d = np.concatenate([mp_desc[sel] ^ np.packbits(rng.random((len(sel), 256)) < flip, axis=1, bitorder="little"),
                            rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
        ur = np.full(n, -1.0, f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            ur[:len(sel)] = (kp["x"][:len(sel)] - bf / pc[sel, 2] + rng.normal(0, 0.5, len(sel))).astype(f32)
        ur[len(sel):] = kp["x"][len(sel):] - rng.uniform(2, 40, n_clutter).astype(f32)
        ur[rng.random(n) < 0.5] = -1.0
        perm = rng.permutation(n)
        kfs.append(dict(kps=np.ascontiguousarray(kp[perm]), desc=np.ascontiguousarray(d[perm]), u_right=np.ascontiguousarray(ur[perm])))
    return dict(cams=cams, poses=poses, bounds=b, scale_factors=sf, inv_level_sigma2=(f32(1.0) / (sf * sf)).astype(f32), log_scale_factor=log_sf,
                map_points=dict(pos=pos, normal=normal, min_dist=min_d, max_dist=max_d, desc=mp_desc), key_frames=kfs)


def make_fisheye_fuse_scene(rng, n_kf: int = 20, n_mp: int = 1000, outliers: bool = True, n_clutter=300, bounds=(0.0, 512.0, 0.0, 512.0),
                            nlevels: int = 8, scale_factor: float = 1.2):
    """make_fuse_scene for a fisheye-stereo rig: n_mp map points seen from n_kf covisible TUM-VI-like rigs (TUMVI_L / TUMVI_R, the baseline of
    make_fisheye_keyframes; key frame 0's left camera has the identity pose).  Map points: x, y within 4 m, z in 1 .. 8 m of key frame 0, with
    make_fuse_scene's six populations -- the x-outliers scaled by 6, not 2.5: a 512 x 512 fisheye image sees far more of the half space than a pinhole
    one.  Each camera's features sit at 70 % of the map points' projections into it (0.8 px noise, 2 - 25 % flipped descriptor bits, octave = the level
    the distance predicts) plus clutter; n_clutter: one number or (left, right).  bounds: one (minX, maxX, minY, maxY) for all key frames or one per
    key frame.  Feature placement uses a plain float64 projection: the exact gates are the caller's (or the library's) business.
    Returns dict(views [n_kf] of (left, right), each (R, t, twc, params8) float32 as orbx_fisheye_view -- GetPose() / GetCameraCenter() / mpCamera and
    GetRightPose() / GetRightCameraCenter() / mpCamera2 --, bounds [n_kf, 4], scale_factors, inv_level_sigma2, log_scale_factor, map_points
    dict(pos, normal, min_dist, max_dist, desc), key_frames [n_kf] dict(kps_left, kps_right KP_DTYPE, desc [N_left + N_right, 32]), trl (Rrl, trl))."""
    from ._lib import KP_DTYPE
    f32 = np.float32
    sf = (f32(scale_factor) ** np.arange(nlevels)).astype(f32)
    log_sf = float(np.log(f32(scale_factor)))
    b = np.broadcast_to(np.asarray(bounds, f32).reshape(-1, 4), (n_kf, 4)).copy()
    ncl = (int(n_clutter),) * 2 if np.isscalar(n_clutter) else tuple(int(x) for x in n_clutter)

    def rodrigues(w):
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-12)
        return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    Rrl, trl = rodrigues(rng.uniform(-0.01, 0.01, 3)).astype(f32), np.array([-0.101, 0.002, 0.001], f32)   # right camera from left camera
    tlr = -Rrl.astype(np.float64).T @ trl.astype(np.float64)                                                # mTlr.translation()
    pos = np.stack([rng.uniform(-4, 4, n_mp), rng.uniform(-4, 4, n_mp), rng.uniform(1.0, 8.0, n_mp)], axis=1)
    ref_dist = np.linalg.norm(pos, axis=1)
    ref_level = rng.integers(0, nlevels - 1, n_mp)
    max_d = ref_dist * sf[ref_level].astype(np.float64) * rng.uniform(0.95, 1.05, n_mp)
    min_d = max_d / float(sf[-1])
    normal = pos / ref_dist[:, None] + rng.normal(0, 0.15, pos.shape)
    normal = normal / np.linalg.norm(normal, axis=1, keepdims=True)
    if outliers:
        kind = rng.choice(6, n_mp, p=[0.66, 0.08, 0.08, 0.04, 0.04, 0.10])
        pos[kind == 1] *= -1.0
        pos[kind == 2, 0] *= 6.0
        max_d[kind == 3] *= 0.3
        min_d[kind == 3] = max_d[kind == 3] / float(sf[-1])
        min_d[kind == 4] = 2.0 * max_d[kind == 4]
        rn = rng.normal(0, 1, (int((kind == 5).sum()), 3))
        normal[kind == 5] = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    mp_desc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    pos, normal, min_d, max_d = pos.astype(f32), normal.astype(f32), min_d.astype(f32), max_d.astype(f32)

    def proj(prm, X):   # KannalaBrandt8::project in float64
        th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2]); psi = np.arctan2(X[:, 1], X[:, 0])
        r = th + prm[4] * th ** 3 + prm[5] * th ** 5 + prm[6] * th ** 7 + prm[7] * th ** 9
        return prm[0] * r * np.cos(psi) + prm[2], prm[1] * r * np.sin(psi) + prm[3]
    views, kfs = [], []
    for k in range(n_kf):
        if k == 0:
            R, t = np.eye(3), np.zeros(3)
        else:
            R, t = rodrigues(rng.normal(0, 0.035, 3)), rng.normal(0, 0.3, 3)
        Rcw, tcw = R.astype(f32), t.astype(f32)
        R64, t64 = Rcw.astype(np.float64), tcw.astype(np.float64)
        Ow = -R64.T @ t64
        Rr = (Rrl.astype(np.float64) @ R64).astype(f32)                                   # GetRightPose() = mTrl * mTcw
        tr = (Rrl.astype(np.float64) @ t64 + trl.astype(np.float64)).astype(f32)
        Owr = (R64.T @ tlr + Ow).astype(f32)                                              # GetRightCameraCenter() = mRwc * mTlr.translation() + mOw
        pair = ((Rcw, tcw, Ow.astype(f32), np.array(TUMVI_L, f32)), (Rr, tr, Owr, np.array(TUMVI_R, f32)))
        views.append(pair)
        parts, descs = [], []
        for s, (Rs, ts, Os, prm) in enumerate(pair):
            pc = pos.astype(np.float64) @ Rs.astype(np.float64).T + ts
            uu, vv = proj(prm.astype(np.float64), pc)
            d3 = np.linalg.norm(pos.astype(np.float64) - Os, axis=1)
            vis = (pc[:, 2] > 0) & (uu > b[k, 0] + 2) & (uu < b[k, 1] - 2) & (vv > b[k, 2] + 2) & (vv < b[k, 3] - 2)
            sel = np.nonzero(vis & (rng.random(n_mp) < 0.7))[0]
            with np.errstate(divide="ignore", invalid="ignore"):
                lvl = np.clip(np.ceil(np.log(max_d[sel].astype(np.float64) / d3[sel]) / log_sf), 0, nlevels - 1).astype(np.int32)
            lvl = np.where(rng.random(len(sel)) < 0.25, np.maximum(lvl - 1, 0), lvl)
            n = len(sel) + ncl[s]
            kp = np.zeros(n, KP_DTYPE)
            kp["x"][:len(sel)] = uu[sel] + rng.normal(0, 0.8, len(sel))
            kp["y"][:len(sel)] = vv[sel] + rng.normal(0, 0.8, len(sel))
            kp["octave"][:len(sel)] = lvl
            kp["x"][len(sel):] = rng.uniform(b[k, 0] + 1, b[k, 1] - 1, ncl[s])
            kp["y"][len(sel):] = rng.uniform(b[k, 2] + 1, b[k, 3] - 1, ncl[s])
            kp["octave"][len(sel):] = rng.integers(0, nlevels, ncl[s])
            kp["size"] = 31.0 * sf[kp["octave"]]
            kp["angle"] = rng.uniform(0, 360, n)
            kp["response"] = rng.integers(7, 200, n)
            kp["class_id"] = -1
            flip = rng.uniform(0.02, 0.25, len(sel))[:, None]
            d = np.concatenate([mp_desc[sel] ^ np.packbits(rng.random((len(sel), 256)) < flip, axis=1, bitorder="little"),
                                rng.integers(0, 256, (ncl[s], 32), dtype=np.uint8)])
            perm = rng.permutation(n)
            parts.append(np.ascontiguousarray(kp[perm]))
            descs.append(d[perm])
        kfs.append(dict(kps_left=parts[0], kps_right=parts[1], desc=np.ascontiguousarray(np.concatenate(descs))))
    return dict(views=views, bounds=b, scale_factors=sf, inv_level_sigma2=(f32(1.0) / (sf * sf)).astype(f32), log_scale_factor=log_sf,
                map_points=dict(pos=pos, normal=normal, min_dist=min_d, max_dist=max_d, desc=mp_desc), key_frames=kfs, trl=(Rrl, trl))
