"""The BowVector of resident handles and the key-frame database (orbx_frame_bow_vector, orbx_keyframe_bow_vector, orbx_keyframe_database_*) against the
restatement of DBoW2's transform / L1Scoring::score and of KeyFrameDatabase's candidate queries in tests/bow_database_scene.py.  Everything is
compared as integers or as the BITS of doubles: the device keeps the reference's order of additions.  PARITY UNPINNED: the restatement is the
reference.  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bow_database_scene as B

pytestmark = pytest.mark.gpu

EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))
BAD, TOO_LARGE = -2, -7


def _same_vec(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(B.bits(got[1]), B.bits(want[1])), (what, int((B.bits(got[1]) != B.bits(want[1])).sum()), len(want[1]))


def _same_query(got, want, what="", cap=None):
    assert got["max_common"] == want["max_common"] and got["n_cand"] == want["n_cand"], (what, got["max_common"], want["max_common"], got["n_cand"], want["n_cand"])
    if got["n_common"] is not None:
        assert np.array_equal(got["n_common"], want["n_common"]), (what, got["n_common"], want["n_common"])
        assert np.array_equal(B.bits(got["score"]), B.bits(want["score"])), (what, np.nonzero(B.bits(got["score"]) != B.bits(want["score"]))[0])
    k = want["n_cand"] if cap is None else min(cap, want["n_cand"])
    assert len(got["cand_slot"]) == k
    assert np.array_equal(got["cand_slot"], want["cand_slot"][:k]) and np.array_equal(got["cand_common"], want["cand_common"][:k]), what
    assert np.array_equal(B.bits(got["cand_score"]), B.bits(want["cand_score"][:k])), what


class Ctx:
    """One scene on the device: the vocabulary, the query frame with BoW, every designed key frame with BoW, the database of 37 slots."""

    def __init__(self, oracle, seed, dense):
        import orb_slam3_amd as osa
        self.ds = ds = B.DatabaseScene(oracle, seed, dense)
        self.m = m = osa.ORBmatcher(0.75, True)
        self.voc = B.device_vocabulary(ds.sc)
        self.F = osa.DeviceFrame(m, B.N_QUERY + 50).load(ds.sc.F)
        self.F.compute_bow(self.voc, B.LEVELSUP, download=False)
        self.kf = {}
        for j, (name, d) in enumerate(ds.kfs):
            self.kf[name] = kf = osa.DeviceKeyFrame.from_host(m, B.frame_view(ds.sc, d, j), None)
            kf.compute_bow(m, self.voc, B.LEVELSUP, download=False)
        self.db = osa.DeviceKeyFrameDatabase(ds.n_slots, B.N_QUERY)
        for name, _ in ds.kfs:
            self.db.add(m, ds.slot[name], self.kf[name])


@pytest.fixture(scope="module")
def ctxs(oracle):
    made = {}

    def get(seed, dense):
        if (seed, dense) not in made:
            made[(seed, dense)] = Ctx(oracle, seed, dense)
        return made[(seed, dense)]
    yield get
    made.clear()


CASES = [(s, d) for s in B.SEEDS for d in (True, False)]


@pytest.mark.parametrize("seed,dense", CASES)
def test_bow_vectors_of_frames_and_key_frames(ctxs, seed, dense):
    import orb_slam3_amd as osa
    c = ctxs(seed, dense)
    ds, m = c.ds, c.m
    _same_vec(c.F.bow_vector(), ds.q_vec, "query frame")
    if dense:
        assert (np.diff(ds.q_vec[0]) > 0).all() and len(ds.q_vec[0]) <= 64
    for name, d in ds.kfs:
        _same_vec(c.kf[name].bow_vector(m), ds.vec[name], name)
    # a key frame made from the frame, its BoW copied: the frame's vector; and frames of 0 and 1 features
    kf = osa.DeviceKeyFrame.from_frame(m, c.F, None).bow_from_frame(m, c.F)
    _same_vec(kf.bow_vector(m), ds.q_vec, "key frame from the frame")
    for name in ("zero", "one"):
        d = dict(ds.kfs)[name]
        Fs = osa.DeviceFrame(m, 8).load(B.frame_view(ds.sc, d))
        Fs.compute_bow(c.voc, B.LEVELSUP, download=False)
        _same_vec(Fs.bow_vector(), ds.vec[name], "frame " + name)


def test_bow_vector_of_a_fisheye_stereo_frame_and_key_frame(oracle):
    """The rows of both cameras form ONE vector over all N rows (Frame::ComputeBoW of a rig)."""
    import orb_slam3_amd as osa
    from test_gpu_frame_fisheye import _kps, _left_view
    ds = B.DatabaseScene(oracle, B.SEEDS[0], False)
    sc, m = ds.sc, osa.ORBmatcher(0.75, True)
    voc = B.device_vocabulary(sc)
    nl = 520
    rng = np.random.default_rng(3)
    kl, kr = _kps(rng, nl), _kps(rng, B.N_QUERY - nl)
    none_l, none_r = np.full(nl, -1, np.int32), np.full(B.N_QUERY - nl, -1, np.int32)
    D = osa.DeviceFrame(m, B.N_QUERY + 100).load_fisheye(_left_view(kl, sc.d), kr, none_l, none_r)
    D.compute_bow_fisheye(voc, B.LEVELSUP, download=False)
    _same_vec(D.bow_vector(), ds.q_vec, "rig frame")
    kf = osa.DeviceKeyFrame.from_frame_fisheye(m, D, None).bow_from_frame_fisheye(m, D)
    _same_vec(kf.bow_vector(m), ds.q_vec, "rig key frame from the frame")
    kh = osa.DeviceKeyFrame.from_host_fisheye(m, _left_view(kl, sc.d), kr, None)
    kh.compute_bow_fisheye(m, voc, B.LEVELSUP, download=False)
    _same_vec(kh.bow_vector(m), ds.q_vec, "rig key frame from host arrays")
    db = osa.DeviceKeyFrameDatabase(5, B.N_QUERY + 100).add(m, 3, kf).add(m, 1, kh)
    want = B.query(ds.q_vec, {1: ds.q_vec, 3: ds.q_vec}, 5)
    _same_query(db.query_frame(m, D), want, "rig frame")
    _same_query(db.query_keyframe(m, kh), want, "rig key frame")


def test_bow_vector_and_database_with_the_count_pending(oracle):
    """A batch-loaded frame whose N never reaches the host: the vector, the key frame made from it, add (bound: the capacity) and both queries."""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from test_gpu_frame_bow import _noisy
    from test_gpu_matcher import _random_vocabulary
    W, H = 320, 240
    ex = osa.ORBextractor(500, 1.2, 8, 20, 7)
    m = osa.ORBmatcher(0.75, True)
    frames = torch.from_numpy(np.stack([synth.make_test_image(5 + t, W, H) for t in range(2)])).cuda()
    ex.extract_batch_device(frames.data_ptr(), 2, W, H, W, W * H, (0, 1000))
    outs = [ex.download(t) for t in range(2)]
    rng = np.random.default_rng(7)
    cp, ci, nd, wi = _random_vocabulary(rng, 6, 3)
    pool = np.concatenate([o[2] for o in outs])
    nd = _noisy(rng, pool[rng.integers(0, len(pool), len(nd))], 0.03)
    weights = rng.uniform(0.1, 1.0, int(wi.max()) + 1)
    weights[rng.random(len(weights)) < 0.1] = 0.0
    voc = osa.ORBVocabulary(3, cp, ci, nd, wi).set_word_weights(weights)
    vecs = [B.bow_vector(oracle.bow_transform(cp, ci, nd, wi, 3, 2, o[2])[0], weights) for o in outs]
    cap = ex.batch_view().cap
    D = osa.DeviceFrame(m, cap)
    db = osa.DeviceKeyFrameDatabase(5, cap)
    kfs = []
    for t in (0, 1):
        D.load_batch(ex, t)
        D.compute_bow(voc, 2, download=False)
        kfs.append(osa.DeviceKeyFrame.from_frame(m, D, None).bow_from_frame(m, D))
        db.add(m, 1 + 2 * t, kfs[-1])                                   # N pending: the row bound is the capacity
    assert cap > len(outs[1][1]) > 50
    small = osa.DeviceKeyFrameDatabase(2, cap - 1)
    assert m._L.orbx_keyframe_database_add(m._h, small._h, 0, kfs[0]._h) == TOO_LARGE
    _same_vec(D.bow_vector(), vecs[1], "frame, count pending")          # D still holds frame 1, its count on the device only
    want = B.query(vecs[1], {1: vecs[0], 3: vecs[1]}, 5)
    _same_query(db.query_frame(m, D), want, "frame, count pending")
    _same_query(db.query_keyframe(m, kfs[1]), want, "key frame, count pending")
    _same_vec(kfs[0].bow_vector(m, cap=cap), vecs[0], "key frame, count pending")
    assert kfs[0].count() == len(outs[0][1])
    _same_vec(kfs[0].bow_vector(m), vecs[0], "key frame, count known")
    assert m._L.orbx_keyframe_database_add(m._h, small._h, 0, kfs[0]._h) == 0      # N is known now and fits


@pytest.mark.parametrize("seed,dense", CASES)
def test_slots_candidates_and_counters(ctxs, seed, dense):
    c = ctxs(seed, dense)
    ds, m = c.ds, c.m
    for ratio in (B.MIN_RATIO, np.float32(0.0)):
        want = B.query(ds.q_vec, ds.slots(), ds.n_slots, min_ratio=ratio)
        got = c.db.query_frame(m, c.F, min_ratio=ratio)
        _same_query(got, want, ("frame", float(ratio)))
        t = m.last_transfers()
        assert t["uploads"] == 0 and t["downloads"] == 1, t                     # no exclude list: nothing goes up; one run comes down
        _same_query(c.db.query_keyframe(m, c.kf["equal"], min_ratio=ratio), want, ("key frame in the database", float(ratio)))
        _same_query(c.db.query_frame(m, c.F, min_ratio=ratio, full=False), want, "without the full arrays")
    full = B.query(ds.q_vec, ds.slots(), ds.n_slots)
    assert full["max_common"] == ds.W and full["n_cand"] >= 1
    if not dense:
        got = c.db.query_frame(m, c.F)
        assert got["n_common"][ds.slot["t"]] == ds.t and ds.slot["t"] not in got["cand_slot"] and ds.slot["t+1"] in got["cand_slot"]
        assert int(B.bits(got["score"][ds.slot["disjoint"]])[0]) == B.NEG_ZERO_BITS and got["n_common"][ds.slot["disjoint"]] == 0
        assert int(B.bits(got["score"][ds.slot["stopped"]])[0]) == B.NEG_ZERO_BITS and int(B.bits(got["score"][0])[0]) == 0 and got["n_common"][0] == -1


@pytest.mark.parametrize("seed", B.SEEDS)
def test_truncated_list_and_exclusion(ctxs, seed):
    c = ctxs(seed, False)
    ds, m = c.ds, c.m
    zero = np.float32(0.0)
    want = B.query(ds.q_vec, ds.slots(), ds.n_slots, min_ratio=zero)
    assert want["n_cand"] > 5
    for cap in (0, 1, 5, want["n_cand"], want["n_cand"] + 1):
        _same_query(c.db.query_frame(m, c.F, min_ratio=zero, cand_cap=cap), want, ("cap", cap), cap=cap)
    ex = [ds.slot["equal"], ds.slot["related1"], 0]                            # (slot 0 is empty anyway)
    want_ex = B.query(ds.q_vec, ds.slots(), ds.n_slots, exclude=set(ex))
    got = c.db.query_frame(m, c.F, exclude=ex)
    _same_query(got, want_ex, "excluded")
    t = m.last_transfers()
    assert t["uploads"] == 1 and t["downloads"] == 1 and t["upload_bytes"] <= 256, t
    assert got["max_common"] < ds.W and got["n_common"][ds.slot["equal"]] == -1
    _same_query(c.db.query_keyframe(m, c.kf["equal"], exclude=ex), want_ex, "excluded, by key frame")


def test_erase_re_add_clear_and_small_databases(ctxs, oracle):
    import orb_slam3_amd as osa
    c = ctxs(B.SEEDS[0], False)
    ds, m = c.ds, c.m
    # 5 slots (not a multiple of the waves of a workgroup): equal, t and t+1 at 0, 2, 4
    db = osa.DeviceKeyFrameDatabase(5, B.N_QUERY)
    at = {"equal": 0, "t": 2, "t+1": 4}
    for n, s in at.items():
        db.add(m, s, c.kf[n])
    slots = {s: ds.vec[n] for n, s in at.items()}
    _same_query(db.query_frame(m, c.F), B.query(ds.q_vec, slots, 5), "5 slots")
    db.erase(m, 0).erase(m, 1)                                                  # (slot 1 was empty)
    del slots[0]
    got = db.query_frame(m, c.F)
    _same_query(got, B.query(ds.q_vec, slots, 5), "erased")
    assert got["n_common"][0] == -1 and got["max_common"] == ds.t + 1
    db.add(m, 0, c.kf["equal"]).add(m, 2, c.kf["one"])                          # re-added; a slot overwritten by a shorter vector
    slots[0], slots[2] = ds.vec["equal"], ds.vec["one"]
    _same_query(db.query_frame(m, c.F), B.query(ds.q_vec, slots, 5), "re-added")
    db.clear(m)
    got = db.query_frame(m, c.F)
    assert got["n_cand"] == 0 and got["max_common"] == 0 and (got["n_common"] == -1).all()
    # one slot whose row is exactly full: 65 features, 65 words, words_cap 65
    one = osa.DeviceKeyFrameDatabase(1, 65)
    assert len(ds.vec["common65"][0]) == 65
    assert m._L.orbx_keyframe_database_add(m._h, one._h, 0, c.kf["equal"]._h) == TOO_LARGE
    one.add(m, 0, c.kf["common65"])
    _same_query(one.query_frame(m, c.F), B.query(ds.q_vec, {0: ds.vec["common65"]}, 1), "full row")
    # the query key frame need not be in the database
    _same_query(one.query_keyframe(m, c.kf["related0"]), B.query(ds.vec["related0"], {0: ds.vec["common65"]}, 1), "foreign query")
    # queries with the empty and the one-word vector
    want = B.query(ds.vec["zero"], ds.slots(), ds.n_slots)
    assert want["n_cand"] == 0 and want["max_common"] == 0
    _same_query(c.db.query_keyframe(m, c.kf["zero"]), want, "empty query")
    _same_query(c.db.query_keyframe(m, c.kf["stopped"]), want, "stopped query")
    _same_query(c.db.query_keyframe(m, c.kf["one"]), B.query(ds.vec["one"], ds.slots(), ds.n_slots), "one-word query")


def test_a_key_frame_destroyed_after_add_still_answers(ctxs):
    import orb_slam3_amd as osa
    c = ctxs(B.SEEDS[1], False)
    ds, m = c.ds, c.m
    db = osa.DeviceKeyFrameDatabase(3, B.N_QUERY)
    d = dict(ds.kfs)["related2"]
    kf = osa.DeviceKeyFrame.from_host(m, B.frame_view(ds.sc, d), None)
    kf.compute_bow(m, c.voc, B.LEVELSUP, download=False)
    db.add(m, 1, kf)
    kf.close()
    _same_query(db.query_frame(m, c.F), B.query(ds.q_vec, {1: ds.vec["related2"]}, 3), "after the key frame's destruction")


def test_a_query_longer_than_the_staging_and_the_norm_tile(oracle):
    """16000 features, more than 8192 distinct words: the largest sort, three norm tiles, the query read through L2."""
    import orb_slam3_amd as osa
    bs = B.BigScene(oracle)
    B.check_conditions_big(bs)
    m = osa.ORBmatcher(0.75, True)
    voc = B.device_vocabulary(bs.sc)
    F = osa.DeviceFrame(m, 16000).load(B.frame_view(bs.sc, bs.d))
    F.compute_bow(voc, B.LEVELSUP, download=False)
    _same_vec(F.bow_vector(), bs.q_vec, "big frame")
    db = osa.DeviceKeyFrameDatabase(bs.n_slots, 700)
    for j, (name, d) in enumerate(bs.kfs):
        kf = osa.DeviceKeyFrame.from_host(m, B.frame_view(bs.sc, d, j), None)
        kf.compute_bow(m, voc, B.LEVELSUP, download=False)
        db.add(m, bs.slot[name], kf)
    _same_query(db.query_frame(m, F), B.query(bs.q_vec, bs.slots(), bs.n_slots), "big query")


def test_two_contexts_on_two_threads_query_one_database(ctxs):
    import orb_slam3_amd as osa
    c = ctxs(B.SEEDS[0], False)
    ds, A = c.ds, c.m
    want = B.query(ds.vec["related0"], ds.slots(), ds.n_slots)
    errors = []
    turn = threading.Lock() if EMULATOR else contextlib.nullcontext()   # (the emulator runs a kernel's lanes as fibers of the calling thread)

    def worker(name, m):
        try:
            for it in range(3):
                with turn:
                    got = c.db.query_keyframe(m, c.kf["related0"])
                _same_query(got, want, (name, it))
        except BaseException as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    t = threading.Thread(target=worker, args=("B", osa.ORBmatcher(0.6, True)), daemon=True)
    t.start()
    worker("A", A)
    t.join(timeout=300)
    assert not t.is_alive(), "the second thread did not finish"
    assert not errors, errors


def test_refusals_leave_the_context_alone(ctxs, oracle):
    import torch
    import orb_slam3_amd as osa
    c = ctxs(B.SEEDS[0], False)
    ds, m = c.ds, c.m
    L = m._L
    want = B.query(ds.q_vec, ds.slots(), ds.n_slots)
    _same_query(c.db.query_frame(m, c.F), want)
    before = m.last_transfers()
    d = dict(ds.kfs)["related0"]
    plain = osa.DeviceKeyFrame.from_host(m, B.frame_view(ds.sc, d), None)                       # no BoW
    sc = ds.sc
    bare = osa.ORBVocabulary(sc.L, sc.cp, sc.ci, sc.nd, sc.wi)                                   # no weights
    kf_bare = osa.DeviceKeyFrame.from_host(m, B.frame_view(sc, d), None)
    kf_bare.compute_bow(m, bare, B.LEVELSUP, download=False)
    other = B.device_vocabulary(sc)                                                              # another vocabulary object
    kf_other = osa.DeviceKeyFrame.from_host(m, B.frame_view(sc, d), None)
    kf_other.compute_bow(m, other, B.LEVELSUP, download=False)
    kf_level = osa.DeviceKeyFrame.from_host(m, B.frame_view(sc, d), None)                        # another levelsup
    kf_level.compute_bow(m, c.voc, B.LEVELSUP + 1, download=False)
    F_bare = osa.DeviceFrame(m, 400).load(B.frame_view(sc, d))
    F_nobow = osa.DeviceFrame(m, 400).load(B.frame_view(sc, d))
    F_bare.compute_bow(bare, B.LEVELSUP, download=False)
    before = m.last_transfers()
    w, v, n = np.full(B.N_QUERY, 77, np.int32), np.full(B.N_QUERY, 7.0), C.c_int(-5)
    out = dict(nc=np.full(ds.n_slots, 77, np.int32), sc=np.full(ds.n_slots, 7.0), cs=np.full(8, 77, np.int32), cc=np.full(8, 77, np.int32),
               csc=np.full(8, 7.0), n_cand=C.c_int(-5), mx=C.c_int(-5))
    P = _lib_ptr()

    def q_frame(f=c.F._h, db=c.db._h, ex=None, n_ex=0, ratio=0.8, mm=m._h):
        return L.orbx_keyframe_database_query_frame(mm, db, f, ex, n_ex, ratio, P(out["nc"]), P(out["sc"]), P(out["cs"]), P(out["cc"]), P(out["csc"]), 8,
                                                    C.byref(out["n_cand"]), C.byref(out["mx"]))

    def q_kf(kf, ex=None, n_ex=0):
        return L.orbx_keyframe_database_query_keyframe(m._h, c.db._h, kf, ex, n_ex, 0.8, P(out["nc"]), P(out["sc"]), P(out["cs"]), P(out["cc"]), P(out["csc"]),
                                                       8, C.byref(out["n_cand"]), C.byref(out["mx"]))
    high, low = np.array([3, ds.n_slots], np.int32), np.array([-1], np.int32)
    refused = [
        L.orbx_keyframe_database_add(m._h, c.db._h, 0, plain._h), L.orbx_keyframe_database_add(m._h, c.db._h, 0, kf_bare._h),
        L.orbx_keyframe_database_add(m._h, c.db._h, 0, kf_other._h), L.orbx_keyframe_database_add(m._h, c.db._h, 0, kf_level._h),
        L.orbx_keyframe_database_add(m._h, c.db._h, -1, c.kf["one"]._h), L.orbx_keyframe_database_add(m._h, c.db._h, ds.n_slots, c.kf["one"]._h),
        L.orbx_keyframe_database_add(m._h, None, 0, c.kf["one"]._h), L.orbx_keyframe_database_add(m._h, c.db._h, 0, None),
        L.orbx_keyframe_database_erase(m._h, c.db._h, ds.n_slots), L.orbx_keyframe_database_erase(m._h, c.db._h, -1),
        L.orbx_keyframe_database_clear(m._h, None),
        q_frame(f=F_nobow._h), q_frame(f=F_bare._h), q_frame(db=None), q_frame(ex=P(high), n_ex=2), q_frame(ex=P(low), n_ex=1), q_frame(n_ex=1),
        q_frame(ratio=1.5), q_frame(ratio=-0.1), q_frame(ratio=float("nan")), q_frame(f=None), q_frame(mm=None),
        q_kf(plain._h), q_kf(kf_bare._h), q_kf(kf_other._h), q_kf(kf_level._h), q_kf(None), q_kf(c.kf["one"]._h, P(high), 2),
        L.orbx_frame_bow_vector(m._h, F_nobow._h, P(w), P(v), C.byref(n)), L.orbx_frame_bow_vector(m._h, F_bare._h, P(w), P(v), C.byref(n)),
        L.orbx_frame_bow_vector(m._h, c.F._h, None, P(v), C.byref(n)), L.orbx_frame_bow_vector(m._h, c.F._h, P(w), P(v), None),
        L.orbx_keyframe_bow_vector(m._h, plain._h, P(w), P(v), C.byref(n)), L.orbx_keyframe_bow_vector(m._h, kf_bare._h, P(w), P(v), C.byref(n)),
    ]
    other_m = osa.ORBmatcher(0.6, True)
    refused += [L.orbx_frame_bow_vector(other_m._h, c.F._h, P(w), P(v), C.byref(n)), q_frame(mm=other_m._h)]   # a handle of another matcher
    if torch.cuda.device_count() > 1 and not EMULATOR:                                                        # another device
        m1 = osa.ORBmatcher(0.6, True, device=1)
        db1 = osa.DeviceKeyFrameDatabase(3, B.N_QUERY, device=1)
        refused += [L.orbx_keyframe_database_add(m._h, db1._h, 0, c.kf["one"]._h), L.orbx_keyframe_database_add(m1._h, c.db._h, 0, c.kf["one"]._h),
                    q_frame(db=db1._h), L.orbx_keyframe_database_erase(m1._h, c.db._h, 0), L.orbx_keyframe_bow_vector(m1._h, c.kf["one"]._h, P(w), P(v), C.byref(n))]
    assert refused == [BAD] * len(refused), refused
    assert m.last_transfers() == before
    assert (w == 77).all() and (v == 7.0).all() and n.value == -5 and (out["nc"] == 77).all() and (out["sc"] == 7.0).all() and (out["cs"] == 77).all()
    assert (out["cc"] == 77).all() and (out["csc"] == 7.0).all() and out["n_cand"].value == -5 and out["mx"].value == -5
    hd = C.c_void_p(5)
    assert L.orbx_keyframe_database_create(0, 0, 10, C.byref(hd)) == BAD and hd.value is None
    assert L.orbx_keyframe_database_create(0, 4, 0, C.byref(hd)) == BAD and L.orbx_keyframe_database_create(0, 4, 16385, C.byref(hd)) == TOO_LARGE
    assert L.orbx_keyframe_database_create(0, (1 << 20) + 1, 4, C.byref(hd)) == TOO_LARGE
    _same_query(c.db.query_frame(m, c.F), want, "after the refusals")


def _lib_ptr():
    from orb_slam3_amd._lib import ptr
    return ptr
