"""ComputeDistinctiveDescriptors on resident key frames as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_distinctive_key_frame_call_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/keyframe_distinctive_check.cpp: orbx_keyframe_distinctive_descriptors with K = 3 key frames (one of them a rig) and sets of 0, 1, 2,
    17, 64, 65 and 130 observations, on a fresh matcher context and twice more on one context that served a call three times as large first: equal
    results, equal to the reference loop written out in the program; the caller's arrays are heap blocks of exactly the needed size, filled with a
    sentinel; a refused call and an empty one leave the transfer counters alone.  A stand-alone program under the sanitizers
    (test_simt_emulation._stand_alone_under_sanitizers): a copy past the caller's array, an upload staged past the pinned mirror, a row gathered
    from outside a key frame's allocation or a kernel writing past the arena ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "keyframe_distinctive_check")
    assert r.returncode == 0 and "keyframe distinctive ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
