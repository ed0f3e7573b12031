"""Inputs of the ComputeDistinctiveDescriptors tests on resident key frames (tests/test_gpu_keyframe_distinctive.py, and the oracle-only check of
tests/test_keyframe_distinctive_abi.py): observation sets whose rows are spread over K = 3 key frames of unequal N."""
import numpy as np

EDGE_SIZES = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 128, 129, 300]   # the register form holds up to 64 rows; the median index changes with N's parity
N_RANDOM = 200
SHARE = (0.2, 0.33)   # of all rows: key frame 0, key frame 1; key frame 2 takes the rest


def noisy_copy(rng, desc, p):
    flip = np.packbits(rng.random((len(desc), 256)) < p, axis=1, bitorder="little")
    return np.ascontiguousarray(desc ^ flip)


def random_keypoints(rng, n, w=640.0, h=480.0):
    from orb_slam3_amd import KP_DTYPE
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = rng.uniform(1, w - 1, n), rng.uniform(1, h - 1, n)
    k["octave"] = rng.integers(0, 8, n)
    k["size"], k["class_id"] = 31.0, -1
    return k


def boundary_sets(seed=61):
    """The set sizes of EDGE_SIZES plus N_RANDOM sizes in 1..40; the rows of a set are noisy copies of one base row (as
    tests/test_gpu_matcher.py::test_distinctive_descriptors builds them), so the medians of a set differ and the winner is not row 0.  Every row
    belongs to one observation; the rows are dealt to three key frames in a random order.
    Returns dict(sizes, set_ptr, rows [T, 32] in observation order, kf_desc: three arrays, obs_kf [T], obs_idx [T])."""
    rng = np.random.default_rng(seed)
    sizes = EDGE_SIZES + [int(n) for n in rng.integers(1, 41, N_RANDOM)]
    set_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    base = rng.integers(0, 256, (len(sizes), 32), dtype=np.uint8)
    rows = np.concatenate([noisy_copy(rng, np.repeat(base[i:i + 1], n, axis=0), 0.08) for i, n in enumerate(sizes) if n > 0])
    T = len(rows)
    n0, n1 = int(T * SHARE[0]), int(T * SHARE[1])
    perm = rng.permutation(T)                       # perm[j] = the observation whose row is slot j of the concatenated key frames
    start = np.array([0, n0, n0 + n1, T])
    obs_kf, obs_idx = np.zeros(T, np.int32), np.zeros(T, np.int32)
    slot_kf = np.searchsorted(start, np.arange(T), side="right") - 1
    obs_kf[perm] = slot_kf
    obs_idx[perm] = np.arange(T) - start[slot_kf]
    kf_desc = [np.ascontiguousarray(rows[perm[start[k]:start[k + 1]]]) for k in range(3)]
    return dict(sizes=sizes, set_ptr=set_ptr, rows=rows, kf_desc=kf_desc, obs_kf=obs_kf, obs_idx=obs_idx)


def gather(kf_desc, obs_kf, obs_idx):
    """mDescriptors.row(idx) of every observation, from the key frames' host arrays (the reference's numbering)."""
    if len(obs_kf) == 0:
        return np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(np.stack([kf_desc[k][i] for k, i in zip(obs_kf, obs_idx)]))
