"""LoopClosing's Sim3 searches on resident key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_sim3_key_frame_calls_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/keyframe_sim3_check.cpp: orbx_keyframe_search_by_projection_sim3 (both projection forms) and orbx_keyframe_fuse_map_points_sim3 with
    K = 2 key frames of unequal N and 300 map points, with and without skip / occupied / projected and the projections, on a fresh matcher context and
    twice more on one context that served a call three times as large first: equal results, the caller's arrays (heap blocks of exactly the needed
    size, filled with a sentinel) written only where a result belongs, a refused call and an empty one leave the transfer counters alone.  A
    stand-alone program under the sanitizers (test_simt_emulation._stand_alone_under_sanitizers): a copy past the caller's array, an upload staged
    past the pinned mirror or a kernel writing past the arena ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "keyframe_sim3_check")
    assert r.returncode == 0 and "keyframe sim3 ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
