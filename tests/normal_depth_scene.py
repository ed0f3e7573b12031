"""Scenes and the composed reference of the MapPoint::UpdateNormalAndDepth tests on resident key frames (tests/test_gpu_normal_depth.py,
tests/test_normal_depth_abi.py, tools/normal_depth_latency.py).

reference_normal_depth restates the member (include/orbx.h, orbx_keyframe_update_normal_and_depth) in float32 numpy, one rounding per operation and
a Python loop over the observations for the ordered sum; nothing here runs device code.  A key frame is a dict(n_left, n_right (-1: monocular),
octave [N] in the reference's numbering (left then right), scale [nlevels], center [3], center_right [3] or None, plus kps / kps_right / desc for the
builders of the device objects)."""
import numpy as np

f32 = np.float32
W, H = 640.0, 480.0
PYRAMIDS = ((8, 1.2), (5, 1.1))                                   # (mnScaleLevels, mfScaleFactor): key frames of one scene differ in both
MONO_N = (150, 257, 400)
RIG_N = ((120, 90), (200, 160))
EDGE_SIZES = [0, 1, 2, 3, 63, 64, 65, 128, 129, 300]             # the wave walks a set in chunks of 64
N_RANDOM = 200
SEEDS = (71, 72, 73)


def scale_factors(nlevels, factor):
    s = np.ones(nlevels, f32)
    for i in range(1, nlevels):                                   # ORBextractor.cc: mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor
        s[i] = f32(s[i - 1] * f32(factor))
    return s


def _dot3(a):
    return f32(f32(f32(f32(0) + f32(a[0] * a[0])) + f32(a[1] * a[1])) + f32(a[2] * a[2]))


def reference_normal_depth(key_frames, set_ptr, obs_kf, obs_idx, ref_obs, pos, reverse=False):
    """(normal [n_sets, 3], min_dist, max_dist) as MapPoint::UpdateNormalAndDepth leaves them, float32, one rounding per operation; the rows of
    empty sets are zeros.  reverse: the observations of every set summed last to first (check_conditions: is the order observable?)."""
    n_sets = len(set_ptr) - 1
    normal, mn, mx = np.zeros((n_sets, 3), f32), np.zeros(n_sets, f32), np.zeros(n_sets, f32)
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(n_sets):
            b, e = int(set_ptr[s]), int(set_ptr[s + 1])
            if e <= b:
                continue
            P = pos[s]
            acc = np.zeros(3, f32)
            order = range(e - 1, b - 1, -1) if reverse else range(b, e)
            for o in order:
                kf = key_frames[int(obs_kf[o])]
                right = kf["n_right"] >= 0 and int(obs_idx[o]) >= kf["n_left"]
                d = (P - f32(kf["center_right"] if right else kf["center"])).astype(f32)       # three subtractions
                nrm = f32(np.sqrt(_dot3(d)))
                acc = (acc + (d / nrm).astype(f32)).astype(f32)                                   # three divisions, three additions
            normal[s] = (acc / f32(e - b)).astype(f32)
            o = b + int(ref_obs[s])
            kf = key_frames[int(obs_kf[o])]
            pc = (P - f32(kf["center"])).astype(f32)                                             # always the left centre
            dist = f32(np.sqrt(_dot3(pc)))
            level = int(kf["octave"][int(obs_idx[o])])
            mx[s] = f32(dist * kf["scale"][level])
            mn[s] = f32(mx[s] / kf["scale"][len(kf["scale"]) - 1])
    return normal, mn, mx


def _keypoints(rng, n, nlevels):
    from orb_slam3_amd import KP_DTYPE
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = rng.uniform(1, W - 1, n), rng.uniform(1, H - 1, n)
    k["octave"] = rng.integers(0, nlevels, n)
    k["size"], k["class_id"] = 31.0, -1
    return k


def make_key_frames(rng):
    """Three monocular key frames of unequal N and two rigs; the pyramids alternate between PYRAMIDS, so neighbours in a set differ.  Rows 0 and 1
    of every camera carry octave 0 and nlevels - 1 (the explicit sets of make_scene take them as reference observations)."""
    kfs = []
    shapes = [(n, -1) for n in MONO_N] + list(RIG_N)
    for k, (nl, nr) in enumerate(shapes):
        nlevels, factor = PYRAMIDS[k % 2]
        kl = _keypoints(rng, nl, nlevels)
        kr = _keypoints(rng, max(nr, 0), nlevels)
        for side in (kl, kr):
            if len(side) >= 2:
                side["octave"][0], side["octave"][1] = 0, nlevels - 1
        center = rng.normal(0, 2, 3).astype(f32)
        kfs.append(dict(n_left=nl, n_right=nr, kps=kl, kps_right=kr, octave=np.concatenate([kl["octave"], kr["octave"]]).astype(np.int32),
                        scale=scale_factors(nlevels, factor), center=center,
                        center_right=(center + rng.normal(0, 0.08, 3).astype(f32)).astype(f32) if nr >= 0 else None,
                        desc=rng.integers(0, 256, (nl + max(nr, 0), 32), dtype=np.uint8)))
    return kfs


def _random_set(rng, kfs, n):
    """n observations in std::map order (ascending key frame); of a rig observation leftIndex, then rightIndex, each where it exists.  A key frame
    may appear more than once (the sets of several hundred observations need it with five key frames; the calls do not mind)."""
    out = []
    for k in np.sort(rng.integers(0, len(kfs), n)):
        kf = kfs[int(k)]
        if kf["n_right"] < 0:
            out.append((int(k), int(rng.integers(0, kf["n_left"]))))
            continue
        u = rng.random()
        if u < 0.8:
            out.append((int(k), int(rng.integers(0, kf["n_left"]))))
        if u >= 0.4:
            out.append((int(k), kf["n_left"] + int(rng.integers(0, kf["n_right"]))))
    return out[:n] if len(out) >= n else out + _random_set(rng, kfs, n - len(out))[:n - len(out)]


def _pick_ref(rng, kfs, obs):
    """A random observation; of a rig pair (left, right of the same key frame, adjacent) the left one."""
    r = int(rng.integers(0, len(obs)))
    k, i = obs[r]
    if kfs[k]["n_right"] >= 0 and i >= kfs[k]["n_left"] and r > 0 and obs[r - 1][0] == k and obs[r - 1][1] < kfs[k]["n_left"]:
        r -= 1
    return r


def make_scene(seed, sizes=None, n_sets=None):
    """sizes: the set sizes (default: EDGE_SIZES + N_RANDOM sizes in 1..40), cut or cycled to n_sets where given.  The first explicit sets replace
    random ones of the same size where the sizes allow (they need 1 to 5 observations); set `nan_set` has Pos == the centre of its first key frame.
    Returns dict(key_frames, sizes, set_ptr, obs_kf, obs_idx, ref_obs, pos, nan_set)."""
    rng = np.random.default_rng(seed)
    kfs = make_key_frames(rng)
    if sizes is None:
        sizes = EDGE_SIZES + [int(n) for n in rng.integers(1, 41, N_RANDOM)]
    sizes = list(sizes)
    if n_sets is not None:
        sizes = [sizes[j % len(sizes)] for j in range(n_sets)]
    explicit = []                                    # (observations, reference position)
    for k, kf in enumerate(kfs):
        nl, nr = kf["n_left"], kf["n_right"]
        explicit.append(([(k, 0)], 0))                                                 # reference level 0
        explicit.append(([(k, 1), (k, 0)], 0))                                         # reference level nlevels - 1
        if nr >= 0:
            explicit.append(([(0, 3), (k, nl + 1)], 1))                                # a right row alone is the reference, second key frame of the set
            explicit.append(([(1, 7), (2, 9), (k, nl)], 2))                            # likewise, third; index N_left
            explicit.append(([(k, nl - 1), (k, nl), (k, nl + nr - 1), (0, 0), (k, 0)], 0))   # N_left - 1, N_left, N - 1
            explicit.append(([(k, nl + nr - 1)], 0))
    by_size = {}
    for obs, r in explicit:
        by_size.setdefault(len(obs), []).append((obs, r))
    sets, refs = [], []
    for n in sizes:
        if by_size.get(n):
            obs, r = by_size[n].pop()
        elif n == 0:
            obs, r = [], 0
        else:
            obs = _random_set(rng, kfs, n)
            r = _pick_ref(rng, kfs, obs)
        sets.append(obs)
        refs.append(r)
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    obs_kf = np.array([k for s in sets for k, _ in s], np.int32)
    obs_idx = np.array([i for s in sets for _, i in s], np.int32)
    mid = np.mean([kf["center"] for kf in kfs], axis=0)
    d = rng.normal(0, 1, (len(sizes), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (mid + d * rng.uniform(8, 14, (len(sizes), 1))).astype(f32)   # 2 .. 20 m from every centre (the centres lie a few metres around `mid`)
    nan_set = -1
    for s, obs in enumerate(sets):
        if len(obs) >= 3 and kfs[obs[0][0]]["n_right"] < 0:
            pos[s] = kfs[obs[0][0]]["center"]
            nan_set = s
            break
    return dict(key_frames=kfs, sizes=sizes, set_ptr=set_ptr, obs_kf=obs_kf, obs_idx=obs_idx, ref_obs=np.array(refs, np.int32), pos=pos,
                nan_set=nan_set)


def centers(scene):
    """(centers [K, 3], centers_right [K, 3]) as the calls take them; the right centre of a monocular key frame is never read (NaN here)."""
    kfs = scene["key_frames"]
    c = np.stack([kf["center"] for kf in kfs]).astype(f32)
    cr = np.stack([kf["center_right"] if kf["center_right"] is not None else np.full(3, np.nan, f32) for kf in kfs]).astype(f32)
    return c, cr


def device_key_frames(osa, m, scene):
    out = []
    for kf in scene["key_frames"]:
        view = osa.FrameView(kf["kps"], kf["desc"], 0.0, W, 0.0, H, kf["scale"])
        out.append(osa.DeviceKeyFrame.from_host(m, view, None) if kf["n_right"] < 0 else
                   osa.DeviceKeyFrame.from_host_fisheye(m, view, kf["kps_right"], None))
    return out


def reference(scene, reverse=False):
    return reference_normal_depth(scene["key_frames"], scene["set_ptr"], scene["obs_kf"], scene["obs_idx"], scene["ref_obs"], scene["pos"], reverse)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check_conditions(scene):
    """What the GPU tests demand of their inputs, asserted on the reference alone (no device code runs)."""
    kfs, sp, ok, oi, ro = scene["key_frames"], scene["set_ptr"], scene["obs_kf"], scene["obs_idx"], scene["ref_obs"]
    assert len({kf["n_left"] for kf in kfs if kf["n_right"] < 0}) == 3 and sum(kf["n_right"] >= 0 for kf in kfs) == 2
    assert {(len(kf["scale"]), float(kf["scale"][1])) for kf in kfs} == {(8, float(f32(1.2))), (5, float(f32(1.1)))}
    normal, mn, mx = reference(scene)
    rev = reference(scene, reverse=True)[0]
    sizes = np.diff(sp)
    order_matters = [s for s in range(len(sizes)) if sizes[s] >= 8 and s != scene["nan_set"] and not np.array_equal(bits(normal[s]), bits(rev[s]))]
    assert len(order_matters) >= 10, len(order_matters)
    right_alone, not_first, levels = 0, 0, set()
    for s in range(len(sizes)):
        b, e = int(sp[s]), int(sp[s + 1])
        if e <= b:
            continue
        o = b + int(ro[s])
        assert 0 <= ro[s] < e - b
        kf = kfs[ok[o]]
        lv = int(kf["octave"][oi[o]])
        levels.add(("first" if lv == 0 else "last" if lv == len(kf["scale"]) - 1 else "mid", len(kf["scale"])))
        not_first += int(ok[o] != ok[b])
        if kf["n_right"] >= 0 and oi[o] >= kf["n_left"]:
            right_alone += int(not any(ok[q] == ok[o] and oi[q] < kf["n_left"] for q in range(b, e)))
    assert right_alone >= 5 and not_first >= 5, (right_alone, not_first)
    assert {("first", 8), ("last", 8), ("first", 5), ("last", 5)} <= levels, levels
    for k, kf in enumerate(kfs):
        if kf["n_right"] >= 0:
            mine = {int(i) for q, i in zip(ok, oi) if q == k}
            assert {kf["n_left"] - 1, kf["n_left"], kf["n_left"] + kf["n_right"] - 1} <= mine, k
    nan_rows = np.isnan(normal).any(axis=1) | np.isnan(mn) | np.isnan(mx)
    assert scene["nan_set"] >= 0 and list(np.flatnonzero(nan_rows)) == [scene["nan_set"]], np.flatnonzero(nan_rows)
    live = sizes > 0
    live[scene["nan_set"]] = False
    far = np.array([[np.linalg.norm(scene["pos"][s].astype(np.float64) - kf["center"]) for kf in kfs] for s in np.flatnonzero(live)])
    assert far.min() >= 2.0 and far.max() <= 20.0, (far.min(), far.max())
    assert (mn[live] > 0).all() and (mx[live] > mn[live]).all()
    return normal, mn, mx
