"""LocalMapping::CreateNewMapPoints' triangulation on resident key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and
UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_new_points_pairs_and_fused_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/new_points_check.cpp: orbx_keyframe_triangulate_pairs[_fisheye] over 1, 63, 64, 65 and all designed pairs and
    orbx_keyframe_search_and_triangulate[_fisheye] behind the BoW search, on a monocular pair of key frames (unequal N, pyramids 8 x 1.2 and 5 x 1.1,
    some features with mvuRight) and a fisheye-stereo pair, against the member's loop written out in C++: equal status, equal bits where a pair is
    accepted, the rows of rejected pairs untouched, the fused row equal to the search's; refusals and the empty call leave the counters alone.  The
    caller's arrays are heap blocks of exactly the needed size.  A stand-alone program under the sanitizers
    (test_simt_emulation._stand_alone_under_sanitizers): a status written past the arena's row or a copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "new_points_check")
    assert r.returncode == 0 and "new points ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
