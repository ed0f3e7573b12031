"""MapPoint::UpdateNormalAndDepth on resident key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_normal_depth_flat_and_refresh_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/normal_depth_check.cpp: orbx_keyframe_update_normal_and_depth (flat) and orbx_keyframe_refresh_map_points_to_map over K = 3 key frames
    (two monocular ones with different pyramids, one rig) and sets of 0, 1, 2, 17, 64, 65 and 130 observations, against MapPoint.cc's loop written
    out in C++: equal bits, an empty set's entries and slot untouched, pos kept, the winning rows in the slots, the table's last slot among them;
    refusals that leave the counters and the table alone.  The caller's arrays are heap blocks of exactly the needed size.  A stand-alone program
    under the sanitizers (test_simt_emulation._stand_alone_under_sanitizers): a record scattered outside the table's allocation, a row written past
    the arena or a copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "normal_depth_check")
    assert r.returncode == 0 and "normal depth ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
