"""The Tracking searches that run from map ids as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_track_map_forms_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/track_map_check.cpp: orbx_frame_track_last_frame_map (level modes 0, 1, 2, mvuRight, has_obs, an occupancy mask) and
    orbx_frame_search_by_projection_keyframe_map against the flat handle forms fed with queries projected on the host as the adapters project them:
    equal return values, match rows mapped back to source features, projected and proj_u / proj_v bit for bit, one upload run smaller than the
    flat form's, refusals that leave the counters alone.  601 source features: three blocks of k_track_project, the last one partial.  The
    caller's arrays are heap blocks of exactly the needed size.  A stand-alone program under the sanitizers
    (test_simt_emulation._stand_alone_under_sanitizers): a record read outside the table's allocation, a query row written past the arena or a
    copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "track_map_check")
    assert r.returncode == 0 and "track map ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
