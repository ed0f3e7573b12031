"""The scene and the COMPOSED reference of the Sim3 projection searches on fisheye-stereo resident key frames (tests/test_gpu_keyframe_sim3_fisheye.py,
tools/loop_closing_fisheye_latency.py).  Nothing here calls the code under test.  The three members (ORBmatcher.cc:427-532, :534-646, :1339-1455)
read the LEFT camera only, so a key frame is its left view, its left keypoints and descriptor rows [0, N_left):
  camera form  the gates of tests/test_gpu_keyframe_fisheye.py (_gates) on the left view: the oracle's is_in_frustum_checks (KannalaBrandt8::project),
               the strict image edge and the double-precision angle test;
  invz form    tests/sim3_scene.py's gates(form = 1) on a copy of the scene whose camera k is the pinhole (params[0..3]) and whose pose k is
               (R, t, twc) of the left view: the reference writes that projection out whatever the camera model is (:573-578);
  searches     the oracle's search_by_projection_window / gate-less fuse_search on an OracleGrid of the LEFT keypoints."""
import numpy as np

import sim3_scene as S
import test_gpu_keyframe_fisheye as TF

f32 = np.float32
TH_LOW = S.TH_LOW
N_MP, N_CLUTTER, N_DUP = 240, (80, 50), 60
SEEDS = {5: 3, 6: 3, 7: 1}   # seed -> K
EQUAL = (0.0, 512.0, 0.0, 512.0)


def make_scene(oracle, seed, K, bounds=EQUAL, n_mp=N_MP, n_clutter=N_CLUTTER, n_dup=N_DUP, special=True):
    """make_fisheye_fuse_scene + sim3_scene.make_scene's n_dup near-duplicates (position jittered by 1 cm, 3 % of the descriptor's bits flipped) and
    permutation, then the exact-mnMaxX and on-the-gate angle points of key frame 0 (test_gpu_keyframe_fisheye._add_special_points: one edge point and
    12 angle points per camera -- the left camera's are the ones that matter here).  bounds: one for all key frames (the search form wants them
    equal) or one per key frame."""
    from orb_slam3_amd import synth
    sc = synth.make_fisheye_fuse_scene(np.random.default_rng(seed), K, n_mp, n_clutter=n_clutter, bounds=bounds)
    rng = np.random.default_rng(1000 + seed)
    mp = sc["map_points"]
    src = rng.integers(0, n_mp, n_dup)
    dup = dict(pos=(mp["pos"][src] + rng.normal(0, 0.01, (n_dup, 3))).astype(f32), normal=mp["normal"][src], min_dist=mp["min_dist"][src],
               max_dist=mp["max_dist"][src], desc=mp["desc"][src] ^ np.packbits(rng.random((n_dup, 256)) < 0.03, axis=1, bitorder="little"))
    perm = rng.permutation(n_mp + n_dup)
    sc["map_points"] = {key: np.ascontiguousarray(np.concatenate([mp[key], dup[key]])[perm]) for key in mp}
    sc["special"] = TF._add_special_points(oracle, sc) if special else ([], [])
    return sc


def left_views(sc, ks, form=0):
    """views[k] of the new calls: the left camera's (R, t, twc, params8); form 1: params8[0..3] = pKF->fx, fy, cx, cy, the rest unread (zeroed here)."""
    out = []
    for k in ks:
        R, t, twc, prm = sc["views"][k][0]
        out.append((R, t, twc, np.concatenate([prm[:4], np.zeros(4, f32)]).astype(f32) if form == 1 else prm))
    return out


def pinhole_copy(sc):
    """The scene as sim3_scene.gates reads it, with the pinhole (fx, fy, cx, cy) = params[0..3] and the pose of every left view."""
    K = len(sc["views"])
    cams = [tuple(float(x) for x in sc["views"][k][0][3][:4]) + (0.0,) * 6 for k in range(K)]
    return dict(sc, cams=cams, poses=[sc["views"][k][0][:3] for k in range(K)])


def gates(oracle, sc, k, form):
    """(ok, u, v, level, stats) of every map point against the left camera of key frame k"""
    if form == 0:
        ok, u, v, lvl, st = TF._gates(oracle, sc, k, 0)
        return ok, u, v, lvl, st
    return S.gates(oracle, pinhole_copy(sc), k, 1)


def left_side(sc, k):
    kf = sc["key_frames"][k]
    nl = len(kf["kps_left"])
    return kf["kps_left"], np.ascontiguousarray(kf["desc"][:nl]), nl, len(kf["desc"])


def grid_of(oracle, sc, k):
    b = sc["bounds"][k]
    return oracle.OracleGrid(left_side(sc, k)[0], float(b[0]), float(b[1]), float(b[2]), float(b[3]))


def search_reference(oracle, sc, kfs_idx, th, ratio, form, skip=None, occupied=None):
    """The composed reference of orbx_keyframe_search_by_projection_sim3_fisheye: per key frame the surviving pairs, in map-point order, through the
    oracle's window search on the LEFT features (accept iff (float)bestDist <= TH_LOW * ratio, no rotation check, a matched feature becomes
    occupied), indices mapped back to map points; match rows of N = N_left + N_right entries, -1 from N_left on; occupied rows of N entries, read
    below N_left.  Returns dict(nm [K], match [K arrays], projected [K, n], u, v [K, n], recs [(sel, q)], stats)."""
    mp = sc["map_points"]
    n, K = len(mp["pos"]), len(kfs_idx)
    out = dict(nm=np.zeros(K, np.int32), match=[], projected=np.zeros((K, n), np.uint8), u=np.zeros((K, n), f32), v=np.zeros((K, n), f32), recs=[],
               stats=[])
    for row, k in enumerate(kfs_idx):
        ok, u, v, lvl, st = gates(oracle, sc, k, form)
        if skip is not None:
            ok = ok & (skip[row] == 0)
        sel = np.nonzero(ok)[0]
        q = dict(x=u[sel], y=v[sel], r=(f32(th) * sc["scale_factors"][lvl[sel]]).astype(f32), min_level=(lvl[sel] - 1).astype(np.int32),
                 max_level=lvl[sel].astype(np.int32), desc=np.ascontiguousarray(mp["desc"][sel]))
        kps, desc, nl, N = left_side(sc, k)
        occ = None if occupied is None or occupied[row] is None else np.ascontiguousarray(occupied[row][:nl], np.uint8)
        full = np.full(N, -1, np.int32)
        if nl:
            nm, m = oracle.search_by_projection_window(grid_of(oracle, sc, k), desc, q, float(f32(TH_LOW) * f32(ratio)), False, occupied=occ)
            full[:nl] = np.where(m >= 0, sel[np.maximum(m, 0)], -1)
            out["nm"][row] = nm
        out["match"].append(full)
        out["projected"][row, sel] = 1
        out["u"][row], out["v"][row] = u, v
        out["recs"].append((sel, q))
        out["stats"].append(st)
    return out


def fuse_reference(oracle, sc, kfs_idx, th, skip=None):
    """The composed reference of orbx_keyframe_fuse_map_points_sim3_fisheye: camera-form gates, then the oracle's gate-less fuse_search (no chi2, no
    mvuRight) on the LEFT features.  Returns (best_idx, best_dist, projected [K, n], recs [(sel, q)])."""
    mp = sc["map_points"]
    n, K = len(mp["pos"]), len(kfs_idx)
    bi, bd, pr = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32), np.zeros((K, n), np.uint8)
    recs = []
    for row, k in enumerate(kfs_idx):
        ok, u, v, lvl, _ = gates(oracle, sc, k, 0)
        if skip is not None:
            ok = ok & (skip[row] == 0)
        sel = np.nonzero(ok)[0]
        q = dict(u=u[sel], v=v[sel], ur=np.zeros(len(sel), f32), r=(f32(th) * sc["scale_factors"][lvl[sel]]).astype(f32), level=lvl[sel].astype(np.int32),
                 desc=np.ascontiguousarray(mp["desc"][sel]))
        kps, desc, nl, _ = left_side(sc, k)
        if nl:
            i, d = oracle.fuse_search(grid_of(oracle, sc, k), desc, None, None, q)
            bi[row, sel], bd[row, sel] = i, d
        pr[row, sel] = 1
        recs.append((sel, q))
    return bi, bd, pr, recs


def stolen_queries(oracle, sc, kfs_idx, ref, th, ratio):
    """Queries of one call whose independent best feature is acceptable but went to an EARLIER query in the replay (the order matters for them)."""
    total = 0
    for row, k in enumerate(kfs_idx):
        sel, q = ref["recs"][row]
        fq = dict(u=q["x"], v=q["y"], ur=np.zeros(len(sel), f32), r=q["r"], level=q["max_level"], desc=q["desc"])
        bi, bd = oracle.fuse_search(grid_of(oracle, sc, k), left_side(sc, k)[1], None, None, fq)
        owner = ref["match"][row]
        for j in range(len(sel)):
            if bi[j] >= 0 and f32(bd[j]) <= f32(TH_LOW) * f32(ratio) and 0 <= owner[bi[j]] < sel[j]:
                total += 1
    return total


def check_conditions(oracle, sc, kfs_idx):
    """What the issue demands of the inputs, asserted on the reference's output (th = 8, ratioHamming = 1.5, no skip, nothing occupied).  Returns the
    figures."""
    K = len(kfs_idx)
    ref = search_reference(oracle, sc, kfs_idx, 8.0, 1.5, 0)
    total = ref["projected"].size
    fig = dict(projected=float(ref["projected"].mean()), matched=float(ref["nm"].sum()) / total,
               stolen=stolen_queries(oracle, sc, kfs_idx, ref, 8.0, 1.5))
    assert fig["projected"] >= 0.5, fig
    assert fig["matched"] >= 0.2, fig
    assert fig["stolen"] >= 8, fig
    for gate in ("behind", "image", "below", "above", "angle"):
        removed = sum(st[gate] for st in ref["stats"])
        fig[gate] = removed / total
        assert removed >= 0.01 * total, (gate, removed, total)
    edge, angle = sc["special"]
    st0 = ref["stats"][0]
    e = [j for s, j in edge if s == 0]       # the left camera's point exactly on mnMaxX: removed by the strict comparison alone
    assert len(e) == 1 and st0["on_edge"][e[0]] and ref["projected"][0, e[0]] == 0, fig
    idx = [i for s, i in angle if s == 0]    # the left camera's 6 + 6 angle points
    r = st0["dot"][idx].astype(np.float64) / st0["dist"][idx].astype(np.float64)
    assert len(idx) == 12 and np.all(np.abs(r - 0.5) < 1e-6)
    rej = st0["dot"][idx].astype(np.float64) < 0.5 * st0["dist"][idx].astype(np.float64)
    assert rej.sum() == 6 and (~rej).sum() == 6
    assert np.array_equal(ref["projected"][0, idx] == 0, rej), "an angle-gate point was removed by another gate"
    # the invz form: a different camera model, so verdicts differ from the camera form's -- and it still finds matches
    inv = search_reference(oracle, sc, kfs_idx, 8.0, 1.5, 1)
    fig["invz_differ"] = [int((inv["projected"][k] != ref["projected"][k]).sum()) for k in range(K)]
    fig["invz_matches"] = [int(x) for x in inv["nm"]]
    assert min(fig["invz_differ"]) >= 20 and min(fig["invz_matches"]) >= 20, fig
    assert len(sc["map_points"]["pos"]) == 300 and K == len(ref["match"])
    return fig
