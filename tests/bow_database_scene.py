"""The reference and the scenes of tests/test_gpu_keyframe_database.py: DBoW2's BowVector (TF_IDF, L1_NORM), L1Scoring::score and the first halves of
KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates restated in plain Python float loops (IEEE double, sequential, in the
reference's order; include/orbx.h cites them), on word ids from the CPU oracle's bow_transform and the weights of test_gpu_frame_bow.Scene.  PARITY
UNPINNED: no DBoW2 is compiled here; the device is compared with this restatement, bit for bit.  No device code runs in this module.

Key frames are DESIGNED from subsets of the query's own descriptor rows, chosen by word, so that their common-word counts are exact."""
import contextlib

import numpy as np

from test_gpu_frame_bow import Scene, _noisy

LEVELSUP = 2
DENSE, SPARSE = (4, 3), (8, 4)          # Scene(seed, 900, k=4, L=3): a few dozen words, each many times; Scene(seed, 900, 8, 4): thousands, sparse
SEEDS = (11, 17)                        # check_conditions() holds for these (tests/test_keyframe_database_abi.py asserts it without a GPU)
BIG_SEED = 31
N_QUERY = 900
MIN_RATIO = np.float32(0.8)
NEG_ZERO_BITS = 0x8000000000000000


def bits(x):
    """the bit patterns of doubles, as uint64"""
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- the reference ----
def bow_vector(words, weights):
    """TemplatedVocabulary::transform's BowVector: addWeight per occurrence (`vit->second += w`, starting from w), then normalize(L1) over the
    std::map in ascending word id.  Returns (ids int32 ascending, values float64)."""
    v = {}
    for w in words:
        w = int(w)
        wt = float(weights[w])
        if wt > 0:
            v[w] = v[w] + wt if w in v else wt
    ids = sorted(v)
    norm = 0.0
    for i in ids:
        norm += abs(v[i])
    vals = [v[i] / norm for i in ids] if norm > 0.0 else [v[i] for i in ids]
    return np.array(ids, np.int32), np.array(vals, np.float64)


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2) and the number of common words: the merge of the two maps in ascending id."""
    a = dict(zip(v1[0].tolist(), v1[1].tolist()))
    score, common = 0.0, 0
    for i, wi in zip(v2[0].tolist(), v2[1].tolist()):
        if i in a:
            vi = a[i]
            score += abs(vi - wi) - abs(vi) - abs(wi)
            common += 1
    return common, -score / 2.0


def query(q_vec, slots, n_slots, exclude=(), min_ratio=MIN_RATIO):
    """slots: {slot: BowVector}.  Returns dict(n_common [n_slots], score [n_slots], max_common, cand_slot, cand_common, cand_score)."""
    n_common, score = np.full(n_slots, -1, np.int32), np.zeros(n_slots, np.float64)
    for s, vec in slots.items():
        if s in exclude:
            continue
        n_common[s], score[s] = l1_score(q_vec, vec)
    max_common = int(max(0, n_common.max()))
    min_common = int(np.float32(max_common) * np.float32(min_ratio))     # int minCommonWords = maxCommonWords * 0.8f
    cand = [s for s in range(n_slots) if n_common[s] > 0 and n_common[s] > min_common]
    return dict(n_common=n_common, score=score, max_common=max_common, n_cand=len(cand), cand_slot=np.array(cand, np.int32),
                cand_common=n_common[cand], cand_score=score[cand])


# ---- what an order-blind implementation would compute (check_conditions) ----
def _tree64(terms):
    """64 strided partial sums, combined as a wave's butterfly combines them"""
    p = [0.0] * 64
    for i, t in enumerate(terms):
        p[i % 64] += t
    s = 32
    while s:
        p = [p[l] + p[l ^ s] for l in range(64)]
        s >>= 1
    return p[0]


def _unnormalised(words, weights):
    v, cnt = {}, {}
    for w in words:
        w = int(w)
        wt = float(weights[w])
        if wt > 0:
            v[w] = v[w] + wt if w in v else wt
            cnt[w] = cnt.get(w, 0) + 1
    return v, cnt


def _strided_score(v1, v2):
    a = dict(zip(v1[0].tolist(), v1[1].tolist()))
    return -_tree64([abs(a[i] - wi) - abs(a[i]) - abs(wi) for i, wi in zip(v2[0].tolist(), v2[1].tolist()) if i in a]) / 2.0


# ---- scenes ----
class _HostVocabulary:
    def __init__(self, *a, **k):
        pass

    def set_word_weights(self, w):
        return self


@contextlib.contextmanager
def _no_device_vocabulary():
    import orb_slam3_amd as osa
    keep = osa.ORBVocabulary
    osa.ORBVocabulary = _HostVocabulary
    try:
        yield
    finally:
        osa.ORBVocabulary = keep


def host_scene(seed, n, k, L, **kw):
    """test_gpu_frame_bow.Scene with its arrays only: the device vocabulary is made by device_vocabulary() where a device is there"""
    with _no_device_vocabulary():
        return Scene(seed, n, k, L, **kw)


def device_vocabulary(sc):
    import orb_slam3_amd as osa
    return osa.ORBVocabulary(sc.L, sc.cp, sc.ci, sc.nd, sc.wi).set_word_weights(sc.weights)


def _words(oracle, sc, desc):
    if len(desc) == 0:
        return np.zeros(0, np.int32)
    return sc.transform(oracle, desc, LEVELSUP)[0]


class DatabaseScene:
    """A query frame of N_QUERY features and designed key frames: kfs = [(name, descriptors)], slots[name] = its slot (gaps between them)."""

    def __init__(self, oracle, seed, dense):
        k, L = DENSE if dense else SPARSE
        self.dense, self.seed = dense, seed
        self.sc = sc = host_scene(seed, N_QUERY, k, L)
        rng = np.random.default_rng(1000 + seed)
        self.q_words = qw = _words(oracle, sc, sc.d)
        self.q_vec = bow_vector(qw, sc.weights)
        self.W = W = len(self.q_vec[0])
        rows_of = {int(w): np.nonzero(qw == w)[0] for w in self.q_vec[0]}
        order = [int(w) for w in rng.permutation(self.q_vec[0])]

        def common(c, all_rows=False):           # rows of the query that give exactly c common words
            idx = [rows_of[w] if all_rows else rows_of[w][:1] for w in order[:c]]
            return sc.d[np.concatenate(idx)] if idx else np.zeros((0, 32), np.uint8)

        kfs = [("equal", sc.d.copy())]
        for j in range(3):                       # related key frames: noisy copies of a part of the query
            src = rng.integers(0, N_QUERY, int(rng.integers(150, 400)))
            kfs.append((f"related{j}", _noisy(rng, sc.d[src], 0.04)))
        stopped = np.nonzero(sc.weights[qw] <= 0)[0]
        kfs += [("stopped", sc.d[stopped]), ("zero", np.zeros((0, 32), np.uint8)), ("one", common(1))]
        self.t = t = int(np.float32(W) * MIN_RATIO)
        if not dense:
            kfs += [("t", common(t, True)), ("t+1", common(t + 1, True))]
            kfs += [(f"common{c}", common(c)) for c in (63, 64, 65)]
            # words the query does not hold, with positive weight: random descriptors, kept by their word
            pool = rng.integers(0, 256, (6000, 32), dtype=np.uint8)
            pw = _words(oracle, sc, pool)
            ok = np.array([sc.weights[w] > 0 and int(w) not in rows_of for w in pw])
            _, first = np.unique(pw[ok], return_index=True)
            self.foreign = foreign = pool[ok][first]          # one row per foreign word
            kfs += [(f"stored{s}", np.concatenate([common(20), foreign[:s - 20]])) for s in (63, 64, 65)]
            kfs.append(("disjoint", foreign[50:50 + 120]))
        self.kfs = kfs
        self.words = {name: _words(oracle, sc, d) for name, d in kfs}
        self.vec = {name: bow_vector(self.words[name], sc.weights) for name, _ in kfs}
        self.slot = {name: 2 * j + 1 for j, (name, _) in enumerate(kfs)}
        self.n_slots = 37
        assert max(self.slot.values()) < self.n_slots

    def slots(self, names=None):
        return {self.slot[n]: self.vec[n] for n in (names or self.slot)}


def check_conditions(ds):
    """What the tests demand of a scene, asserted on the reference alone."""
    sc, W, t = ds.sc, ds.W, ds.t
    common = {n: l1_score(ds.q_vec, v)[0] for n, v in ds.vec.items()}
    assert common["equal"] == W and common["one"] == 1 and common["zero"] == 0 and common["stopped"] == 0
    assert len(ds.kfs[4][1]) > 0 and len(ds.vec["stopped"][0]) == 0            # features, but only stopped words: an empty vector
    assert (sc.weights[ds.q_words] <= 0).any() and (sc.weights == 0).any() and (sc.weights < 0).any()
    full = query(ds.q_vec, ds.slots(), ds.n_slots)
    assert full["max_common"] == W and ds.slot["equal"] in full["cand_slot"]
    if ds.dense:
        raw, cnt = _unnormalised(ds.q_words, sc.weights)
        assert W <= 64 and max(cnt.values()) >= 6
        assert any(c >= 6 and raw[w] != c * float(sc.weights[w]) for w, c in cnt.items()), "no word whose sequential value differs from count * w"
        ids = sorted(raw)
        norm = 0.0
        for i in ids:
            norm += abs(raw[i])
        assert norm != _tree64([abs(raw[i]) for i in ids]), "the ordered norm equals the strided one"
        assert any(l1_score(ds.q_vec, v)[1] != _strided_score(ds.q_vec, v) for v in ds.vec.values()), "every ordered score equals the strided one"
        return
    assert W > 130 and t + 1 < W and 65 < t
    assert common["t"] == t and common["t+1"] == t + 1
    assert ds.slot["t"] not in full["cand_slot"] and ds.slot["t+1"] in full["cand_slot"]          # strict > at the threshold
    for c in (63, 64, 65):
        assert common[f"common{c}"] == c and len(ds.vec[f"common{c}"][0]) == c and len(ds.kfs[[n for n, _ in ds.kfs].index(f"common{c}")][1]) == c
        assert common[f"stored{c}"] == 20 and len(ds.vec[f"stored{c}"][0]) == c
    assert common["disjoint"] == 0 and len(ds.vec["disjoint"][0]) == 120
    assert int(bits(full["score"][ds.slot["disjoint"]])[0]) == NEG_ZERO_BITS and int(bits(full["score"][ds.slot["stopped"]])[0]) == NEG_ZERO_BITS
    ex = query(ds.q_vec, ds.slots(), ds.n_slots, exclude={ds.slot["equal"]})
    assert ex["max_common"] < W and not np.array_equal(ex["cand_slot"], full["cand_slot"])       # the maximum and the list change with the exclusion
    assert any(l1_score(ds.q_vec, v)[1] != _strided_score(ds.q_vec, v) for v in ds.vec.values())
    zero = query(ds.q_vec, ds.slots(), ds.n_slots, min_ratio=np.float32(0.0))
    assert zero["n_cand"] > full["n_cand"] and zero["n_cand"] == sum(1 for c in common.values() if c > 0)


class BigScene:
    """A query of 16000 features over 12^4 words: more distinct words than two norm tiles of k_bow_vector and than the query staging of k_bow_score
    hold, and the largest sort."""

    def __init__(self, oracle, seed=BIG_SEED):
        self.sc = sc = host_scene(seed, 3000, 12, 4, ragged=False)
        rng = np.random.default_rng(2000 + seed)
        self.d = rng.integers(0, 256, (16000, 32), dtype=np.uint8)
        self.q_words = _words(oracle, sc, self.d)
        self.q_vec = bow_vector(self.q_words, sc.weights)
        self.kfs = [("part", self.d[rng.permutation(16000)[:700]]), ("noisy", _noisy(rng, self.d[:400], 0.03)), ("head", self.d[:70])]
        self.vec = {n: bow_vector(_words(oracle, sc, d), sc.weights) for n, d in self.kfs}
        self.slot = {"part": 0, "noisy": 2, "head": 3}
        self.n_slots = 5

    def slots(self):
        return {self.slot[n]: v for n, v in self.vec.items()}


def check_conditions_big(bs):
    assert len(bs.q_vec[0]) > 2 * 4096 + 64, len(bs.q_vec[0])
    got = query(bs.q_vec, bs.slots(), bs.n_slots)
    assert got["max_common"] > 300 and got["n_common"][bs.slot["head"]] > 40


def frame_view(sc, desc, seed=0):
    """a FrameView of `desc` with key points of the scene's kind"""
    import orb_slam3_amd as osa
    from test_gpu_frame_bow import H, SF, W, _keypoints
    return osa.FrameView(_keypoints(np.random.default_rng(500 + seed), len(desc)), np.ascontiguousarray(desc), 0.0, float(W), 0.0, float(H), SF)
