"""BoW on resident fisheye-stereo key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_rig_key_frame_bow_calls_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/keyframe_bow_fisheye_check.cpp: the rig key frame of one 320 x 240 frame made from host arrays, from a host-loaded handle and twice
    from a batch-loaded handle of a capacity above N (both counts pending, a gap of rows behind the left camera's; BoW computed on the key frame or
    copied from the handle), a fresh set per call, through the five entry points: the ids with both buffers and with one, the frame form with K = 2
    and rows of the handle's capacity, the key-frame form with the key frame first and among kfs2, the triangulation gated and coarse with the key
    frame on either side.  Equal results from all four, the extractor's counts afterwards, the caller's arrays (heap blocks of exactly the needed
    size, filled with a sentinel) untouched beyond the rows in use.  A stand-alone program under the sanitizers
    (test_simt_emulation._stand_alone_under_sanitizers): a copy past the caller's array or a kernel writing past a row ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "keyframe_bow_fisheye_check")
    assert r.returncode == 0 and "keyframe bow fisheye ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
