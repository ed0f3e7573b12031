"""The three synchronous whole-batch downloads (orbx_batch_download_all, orbx_stereo_batch_download_all, orbx_stereo_fisheye_batch_download_all) with
every output alone, the rest NULL: each single output equals the same output of the full call.  The outputs of one call
share one pinned staging block: an output laid over another's place in it would show here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B, NF = 320, 240, 3, 500
BF, BASELINE = 40.0, 0.1


@pytest.fixture(scope="module")
def rig():
    """A left / right pair of extractors with three 320 x 240 frames resident and both stereo stages run on them."""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from test_gpu_stereo_fisheye import _rig_for_shifted_images
    canvas = synth.make_canvas(11, size=1024, n_shapes=700)
    pairs = [synth.make_stereo_pair(11, t, W, H, canvas) for t in range(B)]
    left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    exl, exr = osa.ORBextractor(NF, 1.2, 8, 20, 7), osa.ORBextractor(NF, 1.2, 8, 20, 7)
    exl.extract_batch_device(left.data_ptr(), B, W, H, W, W * H, (0, W))
    exr.extract_batch_device(right.data_ptr(), B, W, H, W, W * H, (0, W))
    exl.stereo_batch_device(exr, BF, BASELINE)
    exl.stereo_fisheye_batch_device(exr, _rig_for_shifted_images())
    yield exl, exr
    del left, right


def _each_alone(call, full):
    """call(*outputs) with one output at a time (a sentinel-filled array of the full one's shape), None for the rest."""
    for k, want in enumerate(full):
        got = np.frombuffer(bytes([0x5A]) * want.nbytes, want.dtype).reshape(want.shape).copy()
        call(*[got if j == k else None for j in range(len(full))])
        assert got.tobytes() == want.tobytes(), f"output {k} alone differs from the full call"


def test_batch_download_all_each_output_alone(rig):
    from orb_slam3_amd._lib import check, ptr
    exl, _ = rig
    full = exl.download_all()   # kps, desc, counts, mono
    assert full[2].min() > 100

    def call(kps, desc, counts, mono):
        check(exl._L.orbx_batch_download_all(exl._h, ptr(kps), ptr(desc), ptr(counts), ptr(mono)), "orbx_batch_download_all")
    _each_alone(call, full)


def test_stereo_batch_download_all_each_output_alone(rig):
    exl, _ = rig
    cap = exl.batch_view().cap
    full = (np.zeros((B, cap), np.float32), np.zeros((B, cap), np.float32), np.zeros(B, np.int32))   # u_right, depth, n_matches
    exl.stereo_download_all(*[a.ctypes.data for a in full])
    assert full[2].min() > 0

    def call(*outs):
        exl.stereo_download_all(*[0 if a is None else a.ctypes.data for a in outs])
    _each_alone(call, full)


def test_stereo_fisheye_batch_download_all_each_output_alone(rig):
    from orb_slam3_amd._lib import check, ptr
    exl, _ = rig
    n_matches, desc_matches, l2r, r2l, depth, p3d = exl.stereo_fisheye_download_all()
    assert desc_matches.min() > 0
    full = (l2r, r2l, depth, p3d, n_matches, desc_matches)   # the order of the C arguments

    def call(*outs):
        check(exl._L.orbx_stereo_fisheye_batch_download_all(exl._h, *[ptr(a) for a in outs]), "orbx_stereo_fisheye_batch_download_all")
    _each_alone(call, full)
