"""One frame handle (orbx_frame) loaded again and again, across both kinds and all four loaders: every load must leave the handle exactly as a fresh
handle given the same load -- the loaders share one tail that writes all of the handle's bookkeeping (frame_loaded, orbx_matcher.hip)."""
import numpy as np
import pytest

from test_gpu_frame_fisheye import _extract_pairs, _noisy

pytestmark = pytest.mark.gpu

W, H, NF, N_MP = 320, 240, 500, 300


def _local_map(rng, kps, desc_rows, f, n_mp):
    """n_mp map points in front of a camera at the origin that project onto features of the frame (pinhole or KannalaBrandt8 without distortion, focal
    length f, centre of the image), seen head-on, their descriptors a noisy copy of the feature's."""
    i = rng.integers(0, len(kps), n_mp)
    a = np.stack([(kps["x"][i] - W / 2) / f, (kps["y"][i] - H / 2) / f], 1).astype(np.float64)
    return i, a, _noisy(rng, desc_rows[i], 0.05)


def test_one_handle_reloaded_across_kinds_equals_fresh_handles():
    """320 x 240 frames, 500 features, 300 map points, one handle of rig capacity loaded in turn: monocular from host arrays, fisheye-stereo from host
    arrays, monocular from a batch (count pending), fisheye-stereo from a stereo stage (counts pending, the right rows at the left extractor's capacity:
    a gap behind N_left), monocular from host arrays again.  After each load that kind's SearchLocalPoints and its ComputeBoW ids equal, entry for
    entry, those of a fresh handle given the same load."""
    import orb_slam3_amd as osa
    from test_gpu_matcher import _random_vocabulary
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    nb, fr = 2, 1
    left, right = _extract_pairs(W, H, nb, NF)
    exm, exl, exr = (osa.ORBextractor(NF, 1.2, 8, 20, 7) for _ in range(3))
    for ex, img in ((exm, left), (exl, left), (exr, right)):
        ex.extract_batch_device(img.data_ptr(), nb, W, H, W, W * H, (0, 0))
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    sf = exl.GetScaleFactors().astype(np.float32)
    bounds = (0.0, float(W), 0.0, float(H))
    (_, km, dm), (_, kl, dl), (_, kr, dr) = exm.download(fr), exl.download(fr), exr.download(fr)
    _, _, l2r, r2l, _, _ = exl.stereo_fisheye_download(fr)
    dm = dm.reshape(-1, 32)
    desc = np.concatenate([dl, dr]).reshape(-1, 32)
    nl, nr, capl = len(kl), len(kr), exl.batch_view().cap
    cap = capl + exr.batch_view().cap + 37
    assert len(km) > 100 and 100 < nl < capl and nr > 100   # roff = capl lies above N_left after the batch load

    rng = np.random.default_rng(91)
    m = osa.ORBmatcher(0.8, True)
    cp, ci, nd, wi = _random_vocabulary(rng, 4, 2, ragged=False)
    voc = osa.ORBVocabulary(2, cp, ci, _noisy(rng, desc[rng.integers(0, nl + nr, len(nd))], 0.03), wi)
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    lsf = np.float32(np.log(np.float32(1.2)))

    # monocular: a pinhole camera without distortion (fx = fy = 200), depth along the ray
    i, a, mp_desc_m = _local_map(rng, km, dm, 200.0, N_MP)
    ray = np.concatenate([a, np.ones((N_MP, 1))], 1)
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    d = rng.uniform(2.0, 12.0, N_MP)
    mono = dict(pos=(ray * d[:, None]).astype(np.float32), normal=ray.astype(np.float32), mx=(d * sf[km["octave"][i]] * 1.05).astype(np.float32),
                mn=(0.2 * d).astype(np.float32), desc=mp_desc_m)
    cam10 = (200.0, 200.0, W / 2, H / 2, 0, 0, 0, 0, 0, 40.0)

    # fisheye-stereo: KannalaBrandt8 without distortion (fx = fy = 100) for both cameras, 2 cm apart; the points lie on the left camera's features
    i, a, mp_desc_s = _local_map(rng, kl, desc[:nl], 100.0, N_MP)
    theta = np.linalg.norm(a, axis=1)
    s = np.where(theta > 1e-6, np.sin(theta) / np.maximum(theta, 1e-6), 1.0)
    ray = np.stack([s * a[:, 0], s * a[:, 1], np.cos(theta)], 1)
    d = rng.uniform(2.0, 12.0, N_MP)
    rig = dict(pos=(ray * d[:, None]).astype(np.float32), normal=ray.astype(np.float32), mx=(d * sf[kl["octave"][i]] * 1.05).astype(np.float32),
               mn=(0.2 * d).astype(np.float32), desc=mp_desc_s)
    kb8 = np.array([100.0, 100.0, W / 2, H / 2, 0, 0, 0, 0], np.float32)
    views = [(eye.ravel(), zero, zero, kb8), (eye.ravel(), np.array([-0.02, 0, 0], np.float32), np.array([0.02, 0, 0], np.float32), kb8)]

    def mono_calls(D):
        n, fm, iv = m.SearchLocalPoints(D, cam10, (eye, zero, zero), lsf, 0.5, mono["pos"], mono["normal"], mono["mn"], mono["mx"], mono["desc"], th=3.0)
        return [np.int64(n), fm, iv, *D.compute_bow(voc, 1), np.array(D.counts())]

    def rig_calls(D):
        n, fm, iv = m.SearchLocalPointsFisheye(D, views, lsf, 0.5, rig["pos"], rig["normal"], rig["mn"], rig["mx"], rig["desc"], th=3.0)
        return [np.int64(n), fm, iv, *D.compute_bow_fisheye(voc, 1), np.array(D.counts())]

    mono_view = osa.FrameView(km, dm, *bounds, sf)
    rig_view = osa.FrameView(kl, desc, *bounds, sf)
    loads = [("monocular, host arrays", lambda D: D.load(mono_view), mono_calls, (len(km), -1)),
             ("fisheye-stereo, host arrays", lambda D: D.load_fisheye(rig_view, kr, l2r, r2l), rig_calls, (nl, nr)),
             ("monocular, batch", lambda D: D.load_batch(exm, fr, bounds=bounds, scale_factors=sf), mono_calls, (len(km), -1)),
             ("fisheye-stereo, stereo stage", lambda D: D.load_stereo_fisheye_batch(exl, exr, fr, bounds=bounds, scale_factors=sf), rig_calls, (nl, nr)),
             ("monocular, host arrays again", lambda D: D.load(mono_view), mono_calls, (len(km), -1))]
    handle = osa.DeviceFrame(m, cap)
    for name, load, calls, counts in loads:
        got = calls(load(handle))
        want = calls(load(osa.DeviceFrame(m, cap)))
        assert len(got) == len(want) == 6
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.shape(x) == np.shape(y) and np.array_equal(x, y), (name, k)
        assert tuple(got[5]) == counts and len(got[1]) == len(got[3]) == len(got[4]) == counts[0] + max(counts[1], 0), name
        assert got[0] > 20 and got[2].any(), (name, got[0])   # the search did match: the points were made from the frame's features
