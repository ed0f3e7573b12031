"""The device-resident map-point table as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_map_table_and_map_forms_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/map_check.cpp: orbx_map_create / update (whole, in pieces that straddle the kernels' 64-point blocks, through two contexts) / partial
    update / erase / read, orbx_frame_search_local_points_map and orbx_keyframe_fuse_map_points_map (K = 2, skip, projected) against the flat calls
    on the same rows: equal return values and output arrays, the upload 60 bytes per point smaller, refusals that leave the counters and the table
    alone.  The caller's arrays are heap blocks of exactly the needed size.  A stand-alone program under the sanitizers
    (test_simt_emulation._stand_alone_under_sanitizers): a record scattered or gathered outside the table's allocation, a row written past the arena
    or a copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "map_check")
    assert r.returncode == 0 and "map ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
