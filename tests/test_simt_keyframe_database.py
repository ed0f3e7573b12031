"""The BowVector and the key-frame database as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_keyframe_database_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/keyframe_database_check.cpp: two vocabularies (27 words, every word many times; 512 words, rows of several 64-word chunks), a
    monocular query frame, monocular key frames, an empty one and a fisheye-stereo one; orbx_frame_bow_vector / orbx_keyframe_bow_vector into arrays
    of exactly the vector's length, orbx_keyframe_database_add into slots with gaps, both query forms with and without an exclude list at ratios
    0.8, 0 and 1 and candidate capacities of all slots, 2 and 0, erase, re-add over a longer row, clear, and queries after the key frames are
    destroyed -- against BowVector::addWeight / normalize(L1), L1Scoring::score and the candidate threshold written out in C++ with
    std::map<unsigned, double>: equal bits, nothing written behind a cut list; refusals leave the outputs and the transfer counters alone.  A
    stand-alone program under the sanitizers (test_simt_emulation._stand_alone_under_sanitizers): a word written past a database row, a candidate
    past the arena's list or a copy past the caller's array ends the run."""
    r = _stand_alone_under_sanitizers(tmp_path, "keyframe_database_check")
    assert r.returncode == 0 and "keyframe database ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
