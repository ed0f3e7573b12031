"""The scene and the COMPOSED reference of the Sim3 projection searches on resident key frames (tests/test_gpu_keyframe_sim3.py,
tests/test_keyframe_sim3_abi.py, tools/loop_closing_latency.py).  Nothing here calls the code under test: the gates come from the oracle's
is_in_frustum(cos_limit = -2), the strict-edge removal and the double-precision angle test of tests/test_gpu_keyframe.py (_gates), the second
projection form from float32 numpy, the searches from the oracle's search_by_projection_window / fuse_search."""
import numpy as np

import test_gpu_keyframe as T

f32 = np.float32
TH_LOW = 50
N_MP, N_CLUTTER, N_DUP = 240, 80, 60
SEEDS = {5: 3, 6: 3, 7: 1}   # seed -> K


def make_scene(seed, K, n_mp=N_MP, n_clutter=N_CLUTTER, n_dup=N_DUP, special=True, **kw):
    """make_fuse_scene + n_dup duplicates of random map points (position jittered by 1 cm, 3 % of the descriptor's bits flipped: they compete for one
    feature, so the order of the replay shows), all points permuted, then the exact-mnMaxX and on-the-gate angle points of key frame 0."""
    from orb_slam3_amd import synth
    sc = synth.make_fuse_scene(np.random.default_rng(seed), K, n_mp=n_mp, n_clutter=n_clutter, **kw)
    rng = np.random.default_rng(1000 + seed)
    mp = sc["map_points"]
    src = rng.integers(0, n_mp, n_dup)
    dup = dict(pos=(mp["pos"][src] + rng.normal(0, 0.01, (n_dup, 3))).astype(f32), normal=mp["normal"][src], min_dist=mp["min_dist"][src],
               max_dist=mp["max_dist"][src], desc=mp["desc"][src] ^ np.packbits(rng.random((n_dup, 256)) < 0.03, axis=1, bitorder="little"))
    perm = rng.permutation(n_mp + n_dup)
    sc["map_points"] = {key: np.ascontiguousarray(np.concatenate([mp[key], dup[key]])[perm]) for key in mp}
    sc["special"] = T._add_special_points(sc) if special else ([], [])
    return sc


def gates(oracle, sc, k, form):
    """(ok, u, v, level, stats) of every map point against key frame k for projection form 0 (Pinhole::project, the oracle's) or 1 (invz written out,
    ORBmatcher.cc:573-578, float32 numpy).  stats as T._gates, plus `uv_differ`: the pairs past the image test whose (u, v) differ in bits between
    the forms.  The image tests of the two forms are asserted to agree on every pair in front of the camera; the other gates do not read (u, v)."""
    ok, u0, v0, _, lvl, st = T._gates(oracle, sc, k)
    mp = sc["map_points"]
    Rcw, tcw, _ = sc["poses"][k]
    fx, fy, cx, cy = [f32(x) for x in sc["cams"][k][:4]]
    b = sc["bounds"][k]
    R, P = Rcw.astype(f32), mp["pos"].astype(f32)
    Pc = [((R[r, 0] * P[:, 0] + R[r, 1] * P[:, 1]) + R[r, 2] * P[:, 2]) + tcw[r] for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ua, va = (fx * Pc[0]) / Pc[2] + cx, (fy * Pc[1]) / Pc[2] + cy
        invz = f32(1) / Pc[2]
        ub, vb = fx * (Pc[0] * invz) + cx, fy * (Pc[1] * invz) + cy
    assert ua.dtype == f32 and ub.dtype == f32
    front = ~(Pc[2] < 0)
    img_a = front & (ua >= b[0]) & (ua < b[1]) & (va >= b[2]) & (va < b[3])
    img_b = front & (ub >= b[0]) & (ub < b[1]) & (vb >= b[2]) & (vb < b[3])
    assert np.array_equal(img_a, img_b), "the two projection forms disagree on the image test for a pair of this scene"
    assert np.array_equal(ua[img_a].view(np.uint32), u0[img_a].view(np.uint32)) and np.array_equal(va[img_a].view(np.uint32), v0[img_a].view(np.uint32))
    assert not (ok & ~img_a).any()
    st = dict(st, uv_differ=int((ok & ((ua.view(np.uint32) != ub.view(np.uint32)) | (va.view(np.uint32) != vb.view(np.uint32)))).sum()))
    return (ok, ua, va, lvl, st) if form == 0 else (ok, ub, vb, lvl, st)


def grid_of(oracle, sc, k):
    kf, b = sc["key_frames"][k], sc["bounds"][k]
    return oracle.OracleGrid(kf["kps"], float(b[0]), float(b[1]), float(b[2]), float(b[3]))


def search_reference(oracle, sc, kfs_idx, th, ratio, form, skip=None, occupied=None):
    """The composed reference of orbx_keyframe_search_by_projection_sim3: per key frame the surviving pairs, in map-point order, through the oracle's
    window search (accept iff (float)bestDist <= TH_LOW * ratio, no rotation check, a matched feature becomes occupied), indices mapped back to map
    points.  Returns dict(nm [K], match [K arrays], projected [K, n], u, v [K, n], recs [(sel, q)], stats)."""
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
        occ = None if occupied is None or occupied[row] is None else np.ascontiguousarray(occupied[row], np.uint8)
        nm, m = oracle.search_by_projection_window(grid_of(oracle, sc, k), sc["key_frames"][k]["desc"], q, float(f32(TH_LOW) * f32(ratio)), False,
                                                   occupied=occ)
        out["nm"][row] = nm
        out["match"].append(np.where(m >= 0, sel[np.maximum(m, 0)], -1).astype(np.int32))
        out["projected"][row, sel] = 1
        out["u"][row], out["v"][row] = u, v
        out["recs"].append((sel, q))
        out["stats"].append(st)
    return out


def fuse_reference(oracle, sc, kfs_idx, th, skip=None):
    """The composed reference of orbx_keyframe_fuse_map_points_sim3: form 0 gates, then the oracle's gate-less fuse_search (no chi2, no mvuRight).
    Returns (best_idx, best_dist, projected [K, n], recs [(sel, q)])."""
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
        i, d = oracle.fuse_search(grid_of(oracle, sc, k), sc["key_frames"][k]["desc"], None, None, q)
        bi[row, sel], bd[row, sel], pr[row, sel] = i, d, 1
        recs.append((sel, q))
    return bi, bd, pr, recs


def stolen_queries(oracle, sc, kfs_idx, ref, th, ratio):
    """Queries of one call whose independent best feature is acceptable but went to an EARLIER query in the replay (the order matters for them)."""
    total = 0
    for row, k in enumerate(kfs_idx):
        sel, q = ref["recs"][row]
        fq = dict(u=q["x"], v=q["y"], ur=np.zeros(len(sel), f32), r=q["r"], level=q["max_level"], desc=q["desc"])
        bi, bd = oracle.fuse_search(grid_of(oracle, sc, k), sc["key_frames"][k]["desc"], None, None, fq)
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
               stolen=stolen_queries(oracle, sc, kfs_idx, ref, 8.0, 1.5), uv_differ=[st["uv_differ"] for st in ref["stats"]])
    assert fig["projected"] >= 0.5, fig
    assert fig["matched"] >= 0.2, fig
    assert fig["stolen"] >= 8, fig
    for gate in ("behind", "image", "below", "above", "angle"):
        removed = sum(st[gate] for st in ref["stats"])
        fig[gate] = removed / total
        assert removed >= 0.01 * total, (gate, removed, total)
    edge, angle = sc["special"]
    st0 = ref["stats"][0]
    assert len(edge) == 2 and st0["edge"] >= 1 and all(ref["projected"][0, j] == 0 for j in edge)
    ratio = st0["dot"][angle].astype(np.float64) / st0["dist"][angle].astype(np.float64)
    assert len(angle) == 24 and np.all(np.abs(ratio - 0.5) < 1e-6)
    rej = st0["dot"][angle].astype(np.float64) < 0.5 * st0["dist"][angle].astype(np.float64)
    assert rej.sum() == 12 and (~rej).sum() == 12
    assert min(fig["uv_differ"]) >= 20, fig
    assert len(sc["map_points"]["pos"]) == 300 and K == len(ref["match"])
    return fig
