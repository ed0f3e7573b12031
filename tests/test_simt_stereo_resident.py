"""Rectified-stereo / RGB-D depth on resident frames and key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan
(no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_stereo_resident_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/stereo_resident_check.cpp: orbx_rgbd_batch_device on an extracted batch of two 320 x 240 frames with a distorting camera (a pitch
    above the row, holes of 0, negative and NaN depth), orbx_frame_load_stereo_batch with the count pending and orbx_frame_load_host_stereo from the
    downloaded arrays, orbx_frame_unproject_stereo on both into arrays of exactly N rows; then orbx_keyframe_create_host_stereo and
    orbx_keyframe_triangulate_pairs_stereo over 1, 63, 64, 65 and all designed pairs and orbx_keyframe_search_and_triangulate_stereo behind the
    BoW search -- against Frame::ComputeStereoFromRGBD, Frame::UnprojectStereo and the member's loop with its stereo branches written out in C++:
    equal bits, equal status, the rows of rejected pairs untouched; a key frame without depth leaves its stereo observations to the host; refusals
    and the empty call leave the counters alone.  A stand-alone program under the sanitizers (test_simt_emulation._stand_alone_under_sanitizers):
    a row copied past the handle's buffers, a status written past the arena's row or a copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "stereo_resident_check")
    assert r.returncode == 0 and "stereo resident ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
