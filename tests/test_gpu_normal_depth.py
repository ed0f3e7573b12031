"""MapPoint::UpdateNormalAndDepth on resident key frames (orbx_keyframe_update_normal_and_depth, ..._to_map, orbx_keyframe_refresh_map_points_to_map;
DESIGN.md section 7o).  The reference is tests/normal_depth_scene.py's float32 restatement of the member, computed once per scene; every float result
is compared as uint32 bits (NaN against NaN).  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import functools
import threading

import numpy as np
import pytest

import normal_depth_scene as ND
from test_gpu_keyframe_distinctive import batch  # noqa: F401  (two 320 x 240 stereo pairs through both extractors and the fisheye stage)

pytestmark = pytest.mark.gpu

f32 = np.float32
BAD = -2
FIELDS = ("pos", "normal", "min_dist", "max_dist", "desc")
LAYOUT_ALIGN = 256   # orbx::Layout::pad (matcher_context.h)
BLOCK_SEED = 74      # the scene of 258 sets whose runs of 1, 4, 5, 256 and 257 sets are taken (four sets per block)


def _pad(n):
    return (n + LAYOUT_ALIGN - 1) // LAYOUT_ALIGN * LAYOUT_ALIGN


@functools.lru_cache(maxsize=None)
def _scene(seed, n_sets=None):
    sc = ND.make_scene(seed, n_sets=n_sets)
    sc["want"] = ND.check_conditions(sc)
    return sc


def _same_f32(got, want):
    """Equal bits, or NaN where the reference is NaN (payloads may differ)."""
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return g.shape == w.shape and bool(np.all((ND.bits(g) == ND.bits(w)) | (np.isnan(g) & np.isnan(w))))


def _assert_results(got, want, live):
    for g, w, name in zip(got, want, ("normal", "min_dist", "max_dist")):
        assert _same_f32(g[live], w[live]), (name, np.flatnonzero(ND.bits(g[live]) != ND.bits(w[live]))[:10])
        assert np.array_equal(np.isnan(g[live]), np.isnan(w[live])), name


def _random_points(rng, n, pos):
    return dict(pos=np.ascontiguousarray(pos, f32), normal=rng.normal(0, 1, (n, 3)).astype(f32), min_dist=rng.uniform(0.1, 1, n).astype(f32),
                max_dist=rng.uniform(5, 50, n).astype(f32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))


def _same_records(a, b):
    return all(_same_f32(a[k], b[k]) for k in FIELDS[:4]) and np.array_equal(a["desc"], b["desc"])


def _table(osa, m, rng, sc, capacity=1024):
    """A table whose slots set_id (random, the last slot among them) hold the scene's positions and random other fields; every other slot holds a
    random point.  Returns (map, set_id, other ids, what the table holds per id)."""
    n = len(sc["sizes"])
    assert n < capacity
    ids = rng.permutation(capacity - 1).astype(np.int32)
    set_id = np.ascontiguousarray(np.concatenate([[capacity - 1], ids[:n - 1]]).astype(np.int32)[rng.permutation(n)])
    others = np.ascontiguousarray(ids[n - 1:])
    M = osa.DeviceMap(capacity)
    mine, rest = _random_points(rng, n, sc["pos"]), _random_points(rng, len(others), rng.normal(0, 5, (len(others), 3)))
    M.update(m, set_id, **mine)
    M.update(m, others, **rest)
    return M, set_id, others, mine, rest


def _args(sc):
    c, cr = ND.centers(sc)
    return c, cr, sc["set_ptr"], sc["obs_kf"], sc["obs_idx"], sc["ref_obs"]


# ---- (1) the flat form against the reference ----
@pytest.mark.parametrize("seed", ND.SEEDS)
def test_flat_form_equals_the_reference(seed):
    """Set sizes 0, 1, 2, 3, 63, 64, 65, 128, 129, 300 and 200 random sizes in 1..40 over three monocular key frames and two rigs with two different
    pyramids; the one set with Pos == Owi gives NaN exactly where the reference does."""
    import orb_slam3_amd as osa
    sc = _scene(seed)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, sc)
    got = m.UpdateNormalAndDepthKeyFrames(kfs, *_args(sc), sc["pos"])
    t = m.last_transfers()
    live = np.diff(sc["set_ptr"]) > 0
    _assert_results(got, sc["want"], live)
    assert np.isnan(got[0][sc["nan_set"]]).any() and not np.isnan(got[1]).any()
    assert all(not g[~live].any() for g in got)   # an empty set's entries keep the caller's values (zeros here)
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t


@pytest.mark.parametrize("n_sets", [1, 4, 5, 256, 257])
def test_flat_form_with_the_last_block_full_and_not(n_sets):
    """Sets [1, 1 + n_sets) of one scene (set 0 is empty: set_ptr[0] of the call is not 0 from n_sets = ... on; four sets per 256-lane block)."""
    import orb_slam3_amd as osa
    sc = _scene(BLOCK_SEED, 258)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, sc)
    c, cr = ND.centers(sc)
    for first in (0, 1):
        sl = slice(first, first + n_sets)
        got = m.UpdateNormalAndDepthKeyFrames(kfs, c, cr, sc["set_ptr"][first:first + n_sets + 1], sc["obs_kf"], sc["obs_idx"], sc["ref_obs"][sl],
                                              sc["pos"][sl])
        live = np.diff(sc["set_ptr"][first:first + n_sets + 1]) > 0
        _assert_results(got, [w[sl] for w in sc["want"]], live)


# ---- (2) into the table ----
def test_to_map_form_equals_flat_and_touches_nothing_else():
    import orb_slam3_amd as osa
    sc = _scene(ND.SEEDS[0])
    rng = np.random.default_rng(201)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, sc)
    M, set_id, others, mine, rest = _table(osa, m, rng, sc)
    flat = m.UpdateNormalAndDepthKeyFrames(kfs, *_args(sc), sc["pos"])
    got = m.UpdateNormalAndDepthKeyFramesToMap(kfs, *_args(sc), M, set_id, want_outputs=True)
    t = m.last_transfers()
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t
    live = np.diff(sc["set_ptr"]) > 0
    _assert_results(got, flat, live)
    _assert_results(got, sc["want"], live)
    after = M.read(m, set_id)
    want = dict(mine, normal=np.where(live[:, None], got[0], mine["normal"]), min_dist=np.where(live, got[1], mine["min_dist"]),
                max_dist=np.where(live, got[2], mine["max_dist"]))
    assert _same_records(after, want)                                  # pos and desc of the written slots, and the empty sets' slots whole
    assert np.array_equal(ND.bits(after["pos"]), ND.bits(mine["pos"])) and np.array_equal(after["desc"], mine["desc"])
    assert (~live).sum() >= 1 and _same_records({k: after[k][~live] for k in FIELDS}, {k: mine[k][~live] for k in FIELDS})
    assert _same_records(M.read(m, others), rest)                      # every other slot of the table
    # without outputs: the same records, only the flag comes home
    M2, set_id2, others2, mine2, rest2 = _table(osa, m, np.random.default_rng(201), sc)
    assert m.UpdateNormalAndDepthKeyFramesToMap(kfs, *_args(sc), M2, set_id2) is None
    assert m.last_transfers()["download_bytes"] < t["download_bytes"]
    assert _same_records(M2.read(m, set_id2), after) and _same_records(M2.read(m, others2), rest2)


# ---- (3) both members in one call ----
@pytest.mark.parametrize("seed", ND.SEEDS[:2])
def test_refresh_equals_the_two_calls(oracle, seed):
    import distinctive_sets as DS
    import orb_slam3_amd as osa
    sc = _scene(seed)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, sc)
    A, set_id, others, mine, rest = _table(osa, m, np.random.default_rng(300 + seed), sc)
    B = _table(osa, m, np.random.default_rng(300 + seed), sc)[0]
    best_a = m.DistinctiveDescriptorsKeyFramesToMap(kfs, sc["set_ptr"], sc["obs_kf"], sc["obs_idx"], A, set_id)
    t_distinct = m.last_transfers()
    m.UpdateNormalAndDepthKeyFramesToMap(kfs, *_args(sc), A, set_id)
    best_b = m.RefreshMapPointsToMap(kfs, *_args(sc), B, set_id)
    t = m.last_transfers()
    assert np.array_equal(best_a, best_b)
    rows = DS.gather([kf["desc"] for kf in sc["key_frames"]], sc["obs_kf"], sc["obs_idx"])
    assert np.array_equal(best_b, oracle.distinctive_descriptors(rows, sc["set_ptr"]))
    everything = np.concatenate([set_id, others])
    ra, rb = A.read(m, everything), B.read(m, everything)
    assert _same_records(ra, rb)
    live = np.diff(sc["set_ptr"]) > 0
    got = B.read(m, set_id)
    _assert_results((got["normal"], got["min_dist"], got["max_dist"]), sc["want"], live)
    assert np.array_equal(got["desc"][live], rows[sc["set_ptr"][:-1][live] + best_b[live]]) and np.array_equal(got["desc"][~live], mine["desc"][~live])
    assert np.array_equal(ND.bits(got["pos"]), ND.bits(mine["pos"]))
    # one upload run, one download run; the upload is the distinctive call's plus ref_obs and one 64-byte record per key frame (two more buffers of
    # the arena, each rounded up to the layout's alignment); the download run is the same (best_obs, the flag)
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t
    n_sets, n_kf = len(sc["sizes"]), len(kfs)
    assert t["upload_bytes"] - t_distinct["upload_bytes"] == _pad(4 * n_sets) + _pad(64 * n_kf), (t, t_distinct)
    assert t["download_bytes"] == t_distinct["download_bytes"]


# ---- (4) counts still on the device ----
def _batch_scene(batch, rng):  # noqa: F811
    """Key frame 0 is the monocular handle (the left camera's frame 1), key frame 1 the rig of frame 0: made from batch-loaded handles, their right
    rows start at the handle's left capacity, not at N_left."""
    exl, exr = batch["keep"][:2]
    sf = exl.GetScaleFactors().astype(f32)
    (_, kl0, _), (_, kr0, _) = exl.download(0), exr.download(0)
    _, kl1, _ = exl.download(1)
    nl, nr, _ = batch["host"][0]
    nm = batch["host"][1][0]
    assert (len(kl0), len(kr0), len(kl1)) == (nl, nr, nm)
    kfs = [dict(n_left=nm, n_right=-1, octave=kl1["octave"].astype(np.int32), scale=sf, center=rng.normal(0, 2, 3).astype(f32), center_right=None),
           dict(n_left=nl, n_right=nr, octave=np.concatenate([kl0["octave"], kr0["octave"]]).astype(np.int32), scale=sf,
                center=rng.normal(0, 2, 3).astype(f32), center_right=rng.normal(0, 2, 3).astype(f32))]
    sets = [[(1, nl - 1), (1, nl), (1, nl + nr - 1), (0, nm - 1), (0, 0)], [(0, nm - 1)], [(1, nl + nr - 1), (1, 0)], [(0, 5), (1, nl)]]
    refs = [1, 0, 0, 1]
    for n in [5, 30, 64, 70, 130] + [int(x) for x in rng.integers(2, 30, 30)]:
        sets.append([(0, int(rng.integers(0, nm))) if rng.random() < 0.5 else (1, int(rng.integers(0, nl + nr))) for _ in range(n)])
        refs.append(int(rng.integers(0, n)))
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    sc = dict(key_frames=kfs, sizes=[len(s) for s in sets], set_ptr=set_ptr, obs_kf=np.array([k for s in sets for k, _ in s], np.int32),
              obs_idx=np.array([i for s in sets for _, i in s], np.int32), ref_obs=np.array(refs, np.int32),
              pos=(rng.normal(0, 1, (len(sets), 3)) * 3 + 12).astype(f32), nan_set=-1)
    sc["want"] = ND.reference(sc)
    return sc, (nm, nl, nr)


def test_pending_counts_come_home_with_the_results(batch):  # noqa: F811
    import orb_slam3_amd as osa
    m = batch["m"]
    sc, (nm, nl, nr) = _batch_scene(batch, np.random.default_rng(4))

    def fresh():
        return [osa.DeviceKeyFrame.from_frame(m, batch["mono_handle"], None), osa.DeviceKeyFrame.from_frame_fisheye(m, batch["rig_handles"][0], None)]

    live = np.ones(len(sc["sizes"]), bool)
    pending = fresh()
    got = m.UpdateNormalAndDepthKeyFrames(pending, *_args(sc), sc["pos"])
    t_pending = m.last_transfers()
    _assert_results(got, sc["want"], live)
    assert t_pending["uploads"] == 1 and t_pending["downloads"] == 1 and t_pending["dma_submissions"] == 0 and t_pending["xfer_launches"] == 2, t_pending
    assert [kf.counts() for kf in pending] == [(nm, -1), (nl, nr)]
    assert m.last_transfers() == t_pending                       # the counts were at home: nothing was fetched for them
    got2 = m.UpdateNormalAndDepthKeyFrames(pending, *_args(sc), sc["pos"])
    t_known = m.last_transfers()
    _assert_results(got2, sc["want"], live)
    assert t_known["downloads"] == 1 and 0 < t_pending["download_bytes"] - t_known["download_bytes"] <= 512, (t_pending, t_known)
    # the refresh call brings them home as well (its first kernel does)
    rng = np.random.default_rng(44)
    M = osa.DeviceMap(64)
    set_id = np.ascontiguousarray(rng.permutation(64)[:len(sc["sizes"])].astype(np.int32))
    M.update(m, set_id, **_random_points(rng, len(set_id), sc["pos"]))
    again = fresh()
    m.RefreshMapPointsToMap(again, *_args(sc), M, set_id)
    assert m.last_transfers()["downloads"] == 1 and [kf.counts() for kf in again] == [(nm, -1), (nl, nr)]
    rec = M.read(m, set_id)
    _assert_results((rec["normal"], rec["min_dist"], rec["max_dist"]), sc["want"], live)


def test_a_bad_index_behind_pending_counts_leaves_the_table_alone(batch):  # noqa: F811
    """Index N of a key frame whose count only the device knows: the kernel finds it, the call returns ORBX_E_BAD_ARG, the table is unchanged, and
    the context, the key frames and the table go on working -- for both `_to_map` calls."""
    import orb_slam3_amd as osa
    m = batch["m"]
    sc, (nm, nl, nr) = _batch_scene(batch, np.random.default_rng(5))
    rng = np.random.default_rng(55)
    n = len(sc["sizes"])
    M = osa.DeviceMap(64)
    set_id = np.ascontiguousarray(rng.permutation(64)[:n].astype(np.int32))
    before = _random_points(rng, n, sc["pos"])
    M.update(m, set_id, **before)
    for k, N, call in ((0, nm, "UpdateNormalAndDepthKeyFramesToMap"), (1, nl + nr, "RefreshMapPointsToMap"), (1, nl + nr, "UpdateNormalAndDepthKeyFramesToMap")):
        kfs = [osa.DeviceKeyFrame.from_frame(m, batch["mono_handle"], None), osa.DeviceKeyFrame.from_frame_fisheye(m, batch["rig_handles"][0], None)]
        bad_idx = sc["obs_idx"].copy()
        o = int(np.flatnonzero(sc["obs_kf"] == k)[-1])
        bad_idx[o] = N
        c, cr = ND.centers(sc)
        with pytest.raises(osa.OrbxError) as e:
            getattr(m, call)(kfs, c, cr, sc["set_ptr"], sc["obs_kf"], bad_idx, sc["ref_obs"], M, set_id)
        assert e.value.status == BAD
        assert _same_records(M.read(m, set_id), before)
        assert [kf.count() for kf in kfs] == [nm, nl + nr]
    m.RefreshMapPointsToMap(kfs, *_args(sc), M, set_id)
    rec = M.read(m, set_id)
    _assert_results((rec["normal"], rec["min_dist"], rec["max_dist"]), sc["want"], np.ones(n, bool))


# ---- (5) ordering across contexts ----
def test_update_refresh_and_search_through_two_contexts():
    """orbx_map_update of pos through context A, the refresh through context B with no host synchronisation in between, then
    orbx_keyframe_fuse_map_points_map through A: the results and the table are those of the three calls run one after the other through one context
    with a read of the table (a synchronisation) between them.  From one thread, then from two with a lock around each call."""
    import orb_slam3_amd as osa
    import sim3_scene as S
    import test_gpu_keyframe as T
    fs = S.make_scene(5, 3)
    mp, cams, poses, lsf = fs["map_points"], fs["cams"], fs["poses"], fs["log_scale_factor"]
    n = len(mp["pos"])
    rng = np.random.default_rng(88)
    A, B, ONE = osa.ORBmatcher(0.6, True), osa.ORBmatcher(0.6, True), osa.ORBmatcher(0.6, True)
    kfs = [osa.DeviceKeyFrame.from_host(A, T._view(osa, fs, k), fs["inv_level_sigma2"]) for k in range(3)]
    counts = [len(fs["key_frames"][k]["kps"]) for k in range(3)]
    sizes = rng.integers(1, 6, n)
    set_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    obs_kf = np.concatenate([np.sort(rng.integers(0, 3, s)) for s in sizes]).astype(np.int32)
    obs_idx = np.array([rng.integers(0, counts[k]) for k in obs_kf], np.int32)
    ref_obs = np.array([rng.integers(0, s) for s in sizes], np.int32)
    centers = np.stack([np.asarray(poses[k][2], f32) for k in range(3)])
    ids = np.ascontiguousarray(rng.permutation(1024)[:n].astype(np.int32))
    moved = (mp["pos"] + rng.normal(0, 0.02, mp["pos"].shape)).astype(f32)
    args = (kfs, centers, None, set_ptr, obs_kf, obs_idx, ref_obs)

    def sequential(pos):
        M = osa.DeviceMap(1024)
        M.update(ONE, ids, **mp)
        M.update(ONE, ids, pos=pos)
        M.read(ONE, ids)
        best = ONE.RefreshMapPointsToMap(*args, M, ids)
        M.read(ONE, ids)
        return best, ONE.FuseMapPointsMap(kfs, cams, poses, M, ids, T.TH, lsf), M.read(ONE, ids)

    wants = [sequential(moved), sequential(mp["pos"])]
    assert not _same_records(wants[0][2], wants[1][2])
    M = osa.DeviceMap(1024)
    M.update(A, ids, **mp)

    def check(got, want):
        assert np.array_equal(got[0], want[0])
        for x, y in zip(got[1], want[1]):
            assert np.array_equal(x, y)
        assert _same_records(got[2], want[2])

    for rnd in (0, 1, 0):
        M.update(A, ids, pos=moved if rnd == 0 else mp["pos"])
        best = B.RefreshMapPointsToMap(*args, M, ids)
        fused = A.FuseMapPointsMap(kfs, cams, poses, M, ids, T.TH, lsf)
        check((best, fused, M.read(A, ids)), wants[rnd])
    lock, errors = threading.Lock(), []
    go_b, go_a = threading.Semaphore(0), threading.Semaphore(0)
    out = {}

    def thread_a():
        try:
            for rnd in (1, 0, 1):
                with lock:
                    M.update(A, ids, pos=moved if rnd == 0 else mp["pos"])
                go_b.release()
                go_a.acquire()
                with lock:
                    fused = A.FuseMapPointsMap(kfs, cams, poses, M, ids, T.TH, lsf)
                    check((out["best"], fused, M.read(A, ids)), wants[rnd])
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)
            go_b.release()

    def thread_b():
        try:
            for _ in range(3):
                go_b.acquire()
                with lock:
                    out["best"] = B.RefreshMapPointsToMap(*args, M, ids)
                go_a.release()
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
            go_a.release()

    ts = [threading.Thread(target=thread_a, daemon=True), threading.Thread(target=thread_b, daemon=True)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a thread did not finish"
    assert not errors, errors


# ---- (6) refusals and transfer counters ----
def test_refusals_leave_the_counters_and_the_table_alone():
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    sc = _scene(ND.SEEDS[0])
    rng = np.random.default_rng(6)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, sc)
    M, set_id, others, mine, rest = _table(osa, m, rng, sc)
    n_sets, n_kf = len(sc["sizes"]), len(kfs)
    c, cr = ND.centers(sc)
    hs, hs_mono = m._kf_handles(kfs), m._kf_handles(kfs[:3])
    out = (np.zeros((n_sets, 3), f32), np.zeros(n_sets, f32), np.zeros(n_sets, f32))
    best = np.zeros(n_sets, np.int32)
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    good = dict(n_kf=n_kf, kfs=hs, c=c, cr=cr, n_sets=n_sets, sp=sc["set_ptr"], ok=sc["obs_kf"], oi=sc["obs_idx"], ro=sc["ref_obs"], pos=sc["pos"],
                map=M._h, si=set_id)

    def flat(**kw):
        a = dict(good, **kw)
        return L.orbx_keyframe_update_normal_and_depth(m._h, a["n_kf"], a["kfs"], p(a["c"]), p(a["cr"]), a["n_sets"], p(a["sp"]), p(a["ok"]), p(a["oi"]),
                                                       p(a["ro"]), p(a["pos"]), p(a.get("normal", out[0])), p(a.get("mn", out[1])), p(a.get("mx", out[2])))

    def to_map(**kw):
        a = dict(good, **kw)
        return L.orbx_keyframe_update_normal_and_depth_to_map(m._h, a["n_kf"], a["kfs"], p(a["c"]), p(a["cr"]), a["n_sets"], p(a["sp"]), p(a["ok"]),
                                                              p(a["oi"]), p(a["ro"]), a["map"], p(a["si"]), None, None, None)

    def refresh(**kw):
        a = dict(good, **kw)
        return L.orbx_keyframe_refresh_map_points_to_map(m._h, a["n_kf"], a["kfs"], p(a["c"]), p(a["cr"]), a["n_sets"], p(a["sp"]), p(a["ok"]),
                                                         p(a["oi"]), p(a["ro"]), a["map"], p(a["si"]), p(a.get("best", best)))

    assert flat() == 0 and to_map() == 0 and refresh() == 0
    M.update(m, set_id, **mine)
    M.read(m, set_id)
    counters = m.last_transfers()
    s_live = int(np.flatnonzero(np.diff(sc["set_ptr"]) > 0)[0])
    bad_idx, neg_idx, bad_kf, down = sc["obs_idx"].copy(), sc["obs_idx"].copy(), sc["obs_kf"].copy(), sc["set_ptr"].copy()
    o_mono = int(np.flatnonzero(sc["obs_kf"] == 0)[0])
    bad_idx[o_mono], neg_idx[o_mono], bad_kf[3] = ND.MONO_N[0], -1, n_kf
    down[5], down[6] = down[6], down[5]
    ref_hi, ref_neg = sc["ref_obs"].copy(), sc["ref_obs"].copy()
    ref_hi[s_live], ref_neg[s_live] = sc["sizes"][s_live], -1
    dup, far = set_id.copy(), set_id.copy()
    dup[1] = dup[0]
    far[2] = 1024
    M_small = osa.DeviceMap(16)
    every = [dict(oi=bad_idx), dict(oi=neg_idx), dict(ok=bad_kf), dict(sp=down), dict(sp=None), dict(ok=None), dict(oi=None), dict(kfs=None),
             dict(c=None), dict(cr=None), dict(ro=None), dict(ro=ref_hi), dict(ro=ref_neg), dict(n_kf=0, kfs=None), dict(n_sets=-1)]
    refusals = []
    for kw in every:
        refusals += [flat(**kw), to_map(**kw), refresh(**kw)]
    refusals += [flat(pos=None), flat(normal=None), flat(mn=None), flat(mx=None), refresh(best=None)]
    for kw in (dict(si=None), dict(si=dup), dict(si=far), dict(map=None), dict(map=M_small._h)):   # (M_small: no slot of it is live)
        refusals += [to_map(**kw), refresh(**kw)]
    assert all(r == BAD for r in refusals), refusals
    # centers_right may be NULL only without rigs in kfs
    assert flat(n_kf=3, kfs=hs_mono, cr=None) == BAD    # (the sets still name key frames 3 and 4)
    assert m.last_transfers() == counters
    assert L.orbx_map_erase(M._h, 1, set_id[4:5].ctypes.data) == 0
    assert [to_map(), refresh()] == [BAD, BAD]           # a slot that is not live
    assert m.last_transfers() == counters
    assert [flat(n_sets=0), to_map(n_sets=0), refresh(n_sets=0)] == [0, 0, 0] and m.last_transfers() == counters
    keep = np.delete(set_id, 4)
    assert _same_records(M.read(m, keep), {k: np.delete(mine[k], 4, axis=0) for k in FIELDS}) and _same_records(M.read(m, others), rest)
    # monocular key frames alone need no right centres
    only = np.flatnonzero(np.array([set(sc["obs_kf"][b:e]) <= {0, 1, 2} for b, e in zip(sc["set_ptr"][:-1], sc["set_ptr"][1:])]))
    sub_ptr = np.concatenate([[0], np.cumsum(np.diff(sc["set_ptr"])[only])]).astype(np.int32)
    sel = np.concatenate([np.arange(sc["set_ptr"][s], sc["set_ptr"][s + 1]) for s in only]).astype(np.int64)
    got = m.UpdateNormalAndDepthKeyFrames(kfs[:3], c[:3], None, sub_ptr, sc["obs_kf"][sel], sc["obs_idx"][sel], sc["ref_obs"][only], sc["pos"][only])
    _assert_results(got, [w[only] for w in sc["want"]], np.diff(sub_ptr) > 0)


def test_cost_shape_does_not_depend_on_the_number_of_key_frames():
    """The same sets (they name key frames 0 .. 4) with K = 5 and K = 40 key frames in the call, and with one key frame and sets that name it alone
    (K = 1): equal submission counts; one 64-byte record per key frame goes up."""
    import orb_slam3_amd as osa
    sc = _scene(ND.SEEDS[0])
    rng = np.random.default_rng(7)
    m = osa.ORBmatcher(0.6, True)
    kfs = ND.device_key_frames(osa, m, sc)
    extra = [kfs[k % 5] for k in range(35)]
    c, cr = ND.centers(sc)
    c40, cr40 = np.concatenate([c, c[np.arange(35) % 5]]), np.concatenate([cr, cr[np.arange(35) % 5]])
    M, set_id, others, mine, rest = _table(osa, m, rng, sc)
    live = np.diff(sc["set_ptr"]) > 0
    t = {}
    for K, (hk, ck, crk) in ((5, (kfs, c, cr)), (40, (kfs + extra, c40, cr40))):
        got = m.UpdateNormalAndDepthKeyFrames(hk, ck, crk, sc["set_ptr"], sc["obs_kf"], sc["obs_idx"], sc["ref_obs"], sc["pos"])
        _assert_results(got, sc["want"], live)
        t[K] = m.last_transfers()
        m.RefreshMapPointsToMap(hk, ck, crk, sc["set_ptr"], sc["obs_kf"], sc["obs_idx"], sc["ref_obs"], M, set_id)
        t["refresh", K] = m.last_transfers()
    one_ptr = np.array([0, 3, 3, 70], np.int32)
    idx = rng.integers(0, ND.MONO_N[0], 70).astype(np.int32)
    m.UpdateNormalAndDepthKeyFrames(kfs[:1], c[:1], None, one_ptr, np.zeros(70, np.int32), idx, np.array([2, 0, 66], np.int32), sc["pos"][:3])
    t[1] = m.last_transfers()
    for key in ("uploads", "downloads", "dma_submissions", "xfer_launches"):
        assert t[1][key] == t[5][key] == t[40][key] == t["refresh", 5][key] == t["refresh", 40][key], (key, t)
    assert t[5]["uploads"] == 1 and t[5]["downloads"] == 1 and t[5]["dma_submissions"] == 0
    for a in (t, {5: t["refresh", 5], 40: t["refresh", 40]}):
        assert a[40]["upload_bytes"] - a[5]["upload_bytes"] == _pad(64 * 40) - _pad(64 * 5) + (_pad(32 * 40) - _pad(32 * 5) if a is not t else 0), t
        assert a[40]["download_bytes"] == a[5]["download_bytes"]
