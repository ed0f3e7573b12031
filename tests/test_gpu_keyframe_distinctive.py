"""MapPoint::ComputeDistinctiveDescriptors on resident key frames (orbx_keyframe_distinctive_descriptors): the observations are
named as (key frame, feature index), the device gathers the rows where the key frames keep them.  The reference everywhere is
oracle.distinctive_descriptors on the rows gathered on the host from the key frames' host arrays in the reference's numbering;
orbx_distinctive_descriptors on the same gathered rows must agree."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

import distinctive_sets as DS

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 640.0, 480.0
SF = (f32(1.2) ** np.arange(8)).astype(f32)
BAD, TOO_LARGE = -2, -7


def _mono(osa, m, rng, desc):
    return osa.DeviceKeyFrame.from_host(m, osa.FrameView(DS.random_keypoints(rng, len(desc)), desc, 0.0, W, 0.0, H, SF), None)


def _check(oracle, osa, m, kfs, kf_desc, set_ptr, obs_kf, obs_idx):
    """The call with and without best_desc against the oracle and the host-gather route; returns best_obs."""
    rows = DS.gather(kf_desc, obs_kf[:set_ptr[-1]], obs_idx[:set_ptr[-1]])
    want = oracle.distinctive_descriptors(rows, set_ptr)
    got, desc = m.DistinctiveDescriptorsKeyFrames(kfs, set_ptr, obs_kf, obs_idx)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.array_equal(m.DistinctiveDescriptors(rows, set_ptr), want)
    for s in range(len(set_ptr) - 1):
        expect = rows[set_ptr[s] + want[s]] if want[s] >= 0 else np.zeros(32, np.uint8)
        assert np.array_equal(desc[s], expect), s
    only, none = m.DistinctiveDescriptorsKeyFrames(kfs, set_ptr, obs_kf, obs_idx, want_desc=False)
    assert none is None and np.array_equal(only, want)
    return got


# ---- (1) boundaries of the set size ----
def test_set_size_boundaries(oracle):
    """Sizes 0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 128, 129, 300 and 200 random sizes in 1..40, the rows dealt to three monocular key frames of
    unequal N (each row belongs to one observation, so the key frames hold about 1000 / 1700 / 2400 rows)."""
    import orb_slam3_amd as osa
    S = DS.boundary_sets()
    assert len({len(d) for d in S["kf_desc"]}) == 3
    assert np.array_equal(DS.gather(S["kf_desc"], S["obs_kf"], S["obs_idx"]), S["rows"])
    m = osa.ORBmatcher(0.6, True)
    rng = np.random.default_rng(1)
    kfs = [_mono(osa, m, rng, d) for d in S["kf_desc"]]
    got = _check(oracle, osa, m, kfs, S["kf_desc"], S["set_ptr"], S["obs_kf"], S["obs_idx"])
    assert got[0] == -1 and (got[1:] >= 0).all()
    t = m.last_transfers()
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["dma_submissions"] == 0 and t["xfer_launches"] == 2, t


# ---- (2) ties: the first wins ----
def test_ties_go_to_the_first(oracle):
    import orb_slam3_amd as osa
    rng = np.random.default_rng(2)
    kf_desc = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (150, 257, 400)]
    kf_desc[0][4] = kf_desc[0][3] ^ np.packbits(np.arange(256) < 10, bitorder="little")   # Y = X with ten bits flipped
    for k in (1, 2):
        kf_desc[k][:10] = kf_desc[0][:10]                                                 # rows 0..9 are the same in all three
    sets = [[(0, 5), (1, 70), (0, 5)],                        # the same (key frame, index) twice
            [(1, 70), (0, 5), (2, 90), (0, 5), (1, 70)],
            [(0, 2), (1, 2), (2, 2)],                          # identical rows from different key frames
            [(2, 7), (0, 7)],
            [(2, 100), (0, 3), (1, 3), (0, 4), (2, 4)],       # Z, X, X, Y, Y: X and Y both have the median d(X, Y) = 10, Z's is far above
            [(2, 100), (1, 4), (2, 3), (0, 4), (1, 3)]]       # Z, Y, X, Y, X
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    obs_kf = np.array([k for s in sets for k, _ in s], np.int32)
    obs_idx = np.array([i for s in sets for _, i in s], np.int32)
    m = osa.ORBmatcher(0.6, True)
    kfs = [_mono(osa, m, rng, d) for d in kf_desc]
    got = _check(oracle, osa, m, kfs, kf_desc, set_ptr, obs_kf, obs_idx)
    assert list(got[2:]) == [0, 0, 1, 1], got


# ---- (3), (4) rig key frames; counts still on the device ----
@pytest.fixture(scope="module")
def batch():
    """Two 320 x 240 stereo pairs through the fisheye stereo stage: frame handles loaded from the batch keep their counts on the device, and a key
    frame made from one has room for the handle's capacity, so its right rows do not start at N_left."""
    import orb_slam3_amd as osa
    from test_gpu_frame_fisheye import _extract_pairs
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    w, h, nf = 320, 240, 500
    left, right = _extract_pairs(w, h, 2, nf)
    exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
    exl.extract_batch_device(left.data_ptr(), 2, w, h, w, w * h, (0, 0))
    exr.extract_batch_device(right.data_ptr(), 2, w, h, w, w * h, (0, 0))
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    sf = exl.GetScaleFactors().astype(f32)
    bounds = (0.0, float(w), 0.0, float(h))
    m = osa.ORBmatcher(0.6, True)
    capl, capr = exl.batch_view().cap, exr.batch_view().cap
    rig_handles = [osa.DeviceFrame(m, capl + capr).load_stereo_fisheye_batch(exl, exr, t, bounds=bounds, scale_factors=sf) for t in (0, 1)]
    mono_handle = osa.DeviceFrame(m, capl + 37).load_batch(exl, 1, bounds=bounds, scale_factors=sf)
    exl.sync(); exr.sync()
    host = []
    for t in (0, 1):
        (_, kl, dl), (_, kr, dr) = exl.download(t), exr.download(t)
        host.append((len(kl), len(kr), np.concatenate([dl, dr]).reshape(-1, 32)))
    assert all(min(nl, nr) >= 50 and nl < capl for nl, nr, _ in host)
    return dict(m=m, rig_handles=rig_handles, mono_handle=mono_handle, host=host, keep=(exl, exr, left, right))


def _rig_sets(rng, host, mono_n):
    """Key frame 0 is monocular, 1 and 2 are the rigs of host[0], host[1]: sets that hold left and right indices of the same key frame, the indices
    N_left - 1, N_left and N - 1 among them."""
    sets = []
    for k, (nl, nr, _) in enumerate(host, start=1):
        sets.append([(k, nl - 1), (k, nl), (k, nl + nr - 1), (0, 0), (k, 0)])
        sets.append([(k, nl), (k, nl - 1)])
        sets.append([(k, nl + nr - 1)])
    for n in [3, 7, 20, 64, 65, 90] + [int(x) for x in rng.integers(2, 30, 40)]:
        s = []
        while len(s) < n:   # a rig observation lists leftIndex, then rightIndex, where both exist
            k = int(rng.integers(0, 3))
            if k == 0:
                s.append((0, int(rng.integers(0, mono_n))))
            else:
                nl, nr, _ = host[k - 1]
                s.append((k, int(rng.integers(0, nl))))
                if rng.random() < 0.6:
                    s.append((k, nl + int(rng.integers(0, nr))))
        sets.append(s[:n])
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    return set_ptr, np.array([k for s in sets for k, _ in s], np.int32), np.array([i for s in sets for _, i in s], np.int32)


def test_rig_key_frames_with_right_rows_behind_a_gap(oracle, batch):
    """K = 3: a monocular key frame and two fisheye-stereo key frames made from batch-loaded handles and counted first -- the host knows N_left and
    N_right, the right camera's rows start at the handle's left capacity, not at N_left: a wrong translation reads another row."""
    import orb_slam3_amd as osa
    m, host = batch["m"], batch["host"]
    rng = np.random.default_rng(3)
    mono_desc = rng.integers(0, 256, (211, 32), dtype=np.uint8)
    rigs = [osa.DeviceKeyFrame.from_frame_fisheye(m, D, None) for D in batch["rig_handles"]]
    assert [kf.counts() for kf in rigs] == [(nl, nr) for nl, nr, _ in host]
    kfs = [_mono(osa, m, rng, mono_desc)] + rigs
    set_ptr, obs_kf, obs_idx = _rig_sets(rng, host, len(mono_desc))
    _check(oracle, osa, m, kfs, [mono_desc, host[0][2], host[1][2]], set_ptr, obs_kf, obs_idx)
    for k, (nl, nr, _) in enumerate(host, start=1):   # N is the first index that names no row
        with pytest.raises(osa.OrbxError) as e:
            m.DistinctiveDescriptorsKeyFrames(kfs, [0, 2], [k, k], [0, nl + nr])
        assert e.value.status == BAD


def test_pending_counts_come_home_with_the_results(oracle, batch):
    """A monocular and a rig key frame made from batch-loaded handles, before any call that learns their counts: the results equal the oracle on the
    downloaded rows, the counts come home inside the call's one download run (no submission of their own), and are known afterwards.  An index equal
    to N of such a key frame is found by the kernel."""
    import orb_slam3_amd as osa
    m, host = batch["m"], batch["host"]
    rng = np.random.default_rng(4)
    nl, nr, rig_desc = host[0]
    nm, mono_desc = host[1][0], host[1][2][:host[1][0]]   # the monocular handle holds the left camera's frame 1

    def fresh():
        return [osa.DeviceKeyFrame.from_frame(m, batch["mono_handle"], None), osa.DeviceKeyFrame.from_frame_fisheye(m, batch["rig_handles"][0], None)]

    kf_desc = [mono_desc, rig_desc]
    sets = [[(1, nl - 1), (1, nl), (1, nl + nr - 1), (0, nm - 1), (0, 0)], [(0, nm - 1)], [(1, nl + nr - 1), (1, 0)]]
    for n in [5, 30, 64, 70] + [int(x) for x in rng.integers(2, 30, 30)]:
        sets.append([(0, int(rng.integers(0, nm))) if rng.random() < 0.5 else (1, int(rng.integers(0, nl + nr))) for _ in range(n)])
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    obs_kf = np.array([k for s in sets for k, _ in s], np.int32)
    obs_idx = np.array([i for s in sets for _, i in s], np.int32)
    rows = DS.gather(kf_desc, obs_kf, obs_idx)
    want = oracle.distinctive_descriptors(rows, set_ptr)

    pending = fresh()
    got, desc = m.DistinctiveDescriptorsKeyFrames(pending, set_ptr, obs_kf, obs_idx)
    t_pending = m.last_transfers()
    assert np.array_equal(got, want) and np.array_equal(desc, rows[set_ptr[:-1] + want])
    assert t_pending["uploads"] == 1 and t_pending["downloads"] == 1 and t_pending["dma_submissions"] == 0 and t_pending["xfer_launches"] == 2, t_pending
    assert [kf.counts() for kf in pending] == [(nm, -1), (nl, nr)] and [kf.count() for kf in pending] == [nm, nl + nr]
    assert m.last_transfers() == t_pending                        # the counts were at home: nothing was fetched for them
    got2, _ = m.DistinctiveDescriptorsKeyFrames(pending, set_ptr, obs_kf, obs_idx)
    t_known = m.last_transfers()
    assert np.array_equal(got2, want)
    assert t_known["downloads"] == 1 and 0 < t_pending["download_bytes"] - t_known["download_bytes"] <= 512, (t_pending, t_known)   # two counts per key frame

    for k, n in ((0, nm), (1, nl + nr)):   # index N on a key frame whose count only the device knows
        again = fresh()
        with pytest.raises(osa.OrbxError) as e:
            m.DistinctiveDescriptorsKeyFrames(again, [0, 3], [k, k, k], [0, n, 1])
        assert e.value.status == BAD
        got3, desc3 = m.DistinctiveDescriptorsKeyFrames(again, set_ptr, obs_kf, obs_idx)   # the context and the key frames go on working
        assert np.array_equal(got3, want) and np.array_equal(desc3, desc)
        assert [kf.count() for kf in again] == [nm, nl + nr]


# ---- (5) contract ----
def test_contract(oracle):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    m = osa.ORBmatcher(0.6, True)
    kf_desc = [rng.integers(0, 256, (50 + k, 32), dtype=np.uint8) for k in range(40)]
    kfs = [_mono(osa, m, rng, d) for d in kf_desc]
    sizes = [4, 0, 9, 70, 1]
    set_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    T = int(set_ptr[-1])
    obs_kf, obs_idx = np.zeros(T, np.int32), rng.integers(0, 50, T).astype(np.int32)
    want = oracle.distinctive_descriptors(DS.gather(kf_desc, obs_kf, obs_idx), set_ptr)
    t = {}
    for K in (1, 40):   # the same sets (they name key frame 0 only): the cost shape does not grow with n_kf
        got, _ = m.DistinctiveDescriptorsKeyFrames(kfs[:K], set_ptr, obs_kf, obs_idx)
        assert np.array_equal(got, want)
        t[K] = m.last_transfers()
    for key in ("uploads", "downloads", "dma_submissions", "xfer_launches"):
        assert t[1][key] == t[40][key], (key, t)
    assert t[1]["uploads"] == 1 and t[1]["downloads"] == 1
    assert t[40]["upload_bytes"] - t[1]["upload_bytes"] <= 39 * 32 + 256, t   # one 32-byte record per key frame

    hs = m._kf_handles(kfs)
    best, desc = np.zeros(len(sizes), np.int32), np.zeros((len(sizes), 32), np.uint8)
    p = lambda a: a.ctypes.data   # noqa: E731

    def call(n_kf, handles, n_sets, sp, ok, oi, bo, bd):
        return L.orbx_keyframe_distinctive_descriptors(m._h, n_kf, handles, n_sets, sp, ok, oi, bo, bd)

    good = (p(set_ptr), p(obs_kf), p(obs_idx), p(best), p(desc))
    assert call(40, hs, len(sizes), *good) == 0 and np.array_equal(best, want)
    before = m.last_transfers()
    bad_idx, bad_kf, down = obs_idx.copy(), obs_kf.copy(), set_ptr.copy()
    bad_idx[T - 1] = 50                      # key frame 0 holds 50 rows
    bad_kf[3] = 40
    down[2], down[3] = down[3], down[2]
    neg = obs_idx.copy(); neg[0] = -1
    for args in [(p(set_ptr), p(obs_kf), p(bad_idx), p(best), p(desc)), (p(set_ptr), p(obs_kf), p(neg), p(best), p(desc)),
                 (p(set_ptr), p(bad_kf), p(obs_idx), p(best), p(desc)), (p(down), p(obs_kf), p(obs_idx), p(best), p(desc)),
                 (None, p(obs_kf), p(obs_idx), p(best), p(desc)), (p(set_ptr), None, p(obs_idx), p(best), p(desc)),
                 (p(set_ptr), p(obs_kf), None, p(best), p(desc)), (p(set_ptr), p(obs_kf), p(obs_idx), None, p(desc))]:
        assert call(40, hs, len(sizes), *args) == BAD
    assert call(40, None, len(sizes), *good) == BAD
    assert call(0, None, len(sizes), *good) == BAD                         # observations, but no key frame they could name
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() > 1:       # a key frame of another device (a one-GPU box has none)
        other = osa.ORBmatcher(0.6, True, device=1)
        far = _mono(osa, other, rng, kf_desc[0])
        assert call(1, m._kf_handles([far]), len(sizes), *good) == BAD
    nmax = _lib.MAX_DISTINCTIVE_KEYFRAMES
    assert nmax >= 1024
    many = (C.c_void_p * (nmax + 1))(*[kfs[0]._h.value if isinstance(kfs[0]._h, C.c_void_p) else kfs[0]._h] * (nmax + 1))
    assert call(nmax + 1, many, len(sizes), *good) == TOO_LARGE
    assert call(40, hs, 0, None, None, None, None, None) == 0              # n_sets = 0: nothing to do
    assert call(0, None, 0, None, None, None, None, None) == 0
    empty_ptr = np.zeros(4, np.int32)
    best3 = np.full(3, 7, np.int32); desc3 = np.full((3, 32), 7, np.uint8)
    assert call(0, None, 3, p(empty_ptr), None, None, p(best3), p(desc3)) == 0 and (best3 == -1).all() and not desc3.any()   # empty sets, no key frame
    assert m.last_transfers() == before                                    # none of them enqueued anything
    assert call(nmax, many, len(sizes), *good) == 0 and np.array_equal(best, want)   # the limit itself is fine
    assert call(40, hs, len(sizes), p(set_ptr), p(obs_kf), p(obs_idx), p(best), None) == 0 and np.array_equal(best, want)


# ---- (6) key frames shared between contexts and threads ----
def test_key_frames_shared_between_two_contexts_on_two_threads(oracle):
    import orb_slam3_amd as osa
    S = DS.boundary_sets(seed=66)
    want = oracle.distinctive_descriptors(S["rows"], S["set_ptr"])
    A = osa.ORBmatcher(0.6, True)
    rng = np.random.default_rng(6)
    kfs = [_mono(osa, A, rng, d) for d in S["kf_desc"]]   # enqueued by A, handed over without a synchronisation
    errors = []
    # (the CPU emulator runs a kernel's lanes as fibers of the calling thread and is not re-entrant: there the two threads take turns)
    turn = threading.Lock() if os.environ.get("ORBX_TEST_EMULATOR") else contextlib.nullcontext()

    def worker(name, m):
        try:
            for it in range(4):
                with turn:
                    got, desc = m.DistinctiveDescriptorsKeyFrames(kfs, S["set_ptr"], S["obs_kf"], S["obs_idx"])
                assert np.array_equal(got, want), (name, it)
                assert np.array_equal(desc[1:], S["rows"][S["set_ptr"][1:-1] + want[1:]]), (name, it)
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    t = threading.Thread(target=worker, args=("B", osa.ORBmatcher(0.6, True)), daemon=True)
    t.start()
    worker("A", A)
    t.join(timeout=300)
    assert not t.is_alive(), "the second thread did not finish"
    assert not errors, errors
