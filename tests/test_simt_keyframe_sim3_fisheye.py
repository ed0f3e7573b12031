"""LoopClosing's Sim3 searches on fisheye-stereo resident key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan
(no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_sim3_fisheye_key_frame_calls_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/keyframe_sim3_fisheye_check.cpp: orbx_keyframe_search_by_projection_sim3_fisheye (both projection forms) and
    orbx_keyframe_fuse_map_points_sim3_fisheye with K = 2 rig key frames of unequal N_left / N_right and 300 map points, with and without skip /
    occupied / projected and the projections, on a fresh matcher context and twice more on one context that served a call three times as large first:
    equal results, the caller's arrays (heap blocks of exactly the needed size -- match and occupied rows of N_left + N_right entries -- filled with a
    sentinel) written only where a result belongs, match rows -1 from N_left on, Fuse indices below N_left; a refused call of each kind and an empty
    one leave the transfer counters alone.  A stand-alone program under the sanitizers (test_simt_emulation._stand_alone_under_sanitizers): a copy
    past the caller's array, an upload staged past the pinned mirror or a kernel writing past the arena ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "keyframe_sim3_fisheye_check")
    assert r.returncode == 0 and "keyframe sim3 fisheye ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
