"""The extractor's synchronous downloads and the stages behind an extraction as a stand-alone program on the SIMT emulator, under AddressSanitizer
and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_staged_downloads_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/staged_download_check.cpp: three 320 x 240 frames per side, one of them flat, on one extractor and on a left / right pair.
    orbx_batch_download per frame == that frame's rows of orbx_batch_download_all, one row short it returns ORBX_E_CAPACITY and still reports the
    count, the flat frame reports 0 and writes nothing; orbx_batch_download_keypoints_un == the raw key points without a camera; each of
    orbx_batch_download_all, orbx_stereo_batch_download_all and orbx_stereo_fisheye_batch_download_all with every output alone == that output of the
    full call, and the full call == the per-frame downloads row for row; the RGB-D stage on float and on 16-bit depth (integers, factor 1) gives equal
    results and counts, also on a second batch extracted while the first results leave through orbx_stereo_batch_download_async; orbx_get_level for
    level 0 and the last level into a destination whose stride is the padded width; orbx_debug_level_keypoints returns the same count without a
    buffer and with one of exactly that many entries.  Every caller buffer is a heap block of exactly the bytes the call may write, filled with a
    sentinel: a copy of the capacity where the count is due ends the run, an output that landed in another's place fails an equality."""
    r = _stand_alone_under_sanitizers(tmp_path, "staged_download_check")
    assert r.returncode == 0 and "staged downloads ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
