"""The shared gates of the map-point projection kernels as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_projection_gates_of_every_entry_point_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/project_gates_check.cpp: 257 map points (two blocks, the second with one live lane) of ten classes whose verdict is known by
    construction -- accepted, skipped, behind the camera, outside the image on each side, outside either distance bound, seen from behind the normal;
    two of the accepted ones clamp their predicted level at 0 and at nlevels - 1 -- through orbx_is_in_frustum, orbx_is_in_frustum_checks,
    orbx_keyframe_fuse_map_points[_fisheye] (two key frames of different bounds and levels, a skip row each),
    orbx_keyframe_search_by_projection_sim3[_fisheye] (K = 2 and K = 1, both projection forms) and
    orbx_frame_search_by_projection_keyframe[_fisheye]_map: in_view / projected equal the designed verdict for every pair, at least 20 pairs per class
    and call, and isInFrustum, the Sim3 search and Relocalization's search agree on (u, v) bit for bit wherever all three accept (the pinhole trio and
    the KannalaBrandt8 trio) -- the contract of the helpers the kernels share.  The caller's arrays are heap blocks of exactly the needed size.  A
    stand-alone program under the sanitizers (test_simt_emulation._stand_alone_under_sanitizers): a skip row read for the wrong key frame, a query
    row written past the arena or a copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "project_gates_check")
    assert r.returncode == 0 and "project gates ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
