"""The BowVector and the key-frame database through every layer, without a GPU: the nine entry points are exported by liborbx.so, declared in
include/orbx.h, registered by the ctypes loader with as many argument types as the header declares parameters, named by the Python wrappers and wrapped
in C++, where the wrappers compile and link in a translation unit of their own.  One reference-only test asserts what
tests/test_gpu_keyframe_database.py demands of its scenes, for every seed it uses."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_frame_bow_vector", "orbx_keyframe_bow_vector", "orbx_keyframe_database_create", "orbx_keyframe_database_destroy",
           "orbx_keyframe_database_add", "orbx_keyframe_database_erase", "orbx_keyframe_database_clear", "orbx_keyframe_database_query_frame",
           "orbx_keyframe_database_query_keyframe"]
PY_NAMES = [("DeviceFrame", "bow_vector"), ("DeviceKeyFrame", "bow_vector"), ("DeviceKeyFrameDatabase", "add"), ("DeviceKeyFrameDatabase", "erase"),
            ("DeviceKeyFrameDatabase", "clear"), ("DeviceKeyFrameDatabase", "query_frame"), ("DeviceKeyFrameDatabase", "query_keyframe"),
            ("DeviceKeyFrameDatabase", "close")]
QUERY_TAIL = ("const int32_t *exclude, int n_exclude, float min_ratio, int32_t *n_common, double *score, int32_t *cand_slot, int32_t *cand_common, "
              "double *cand_score, int cand_cap, int *n_cand, int *max_common")


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + ["orbx_vocabulary_set_word_weights", "orbx_frame_compute_bow", "orbx_keyframe_compute_bow", "orbx_map_create"]:   # the others stay
        assert s in exported, s


def _declaration(h, symbol):
    m = re.search(r"\b(?:int|void)\s+%s\(([^;]*)\);" % symbol, h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert _declaration(h, SYMBOLS[0]) == "orbx_matcher *m, orbx_frame *f, int32_t *word_id, double *value, int *n_words"
    assert _declaration(h, SYMBOLS[1]) == "orbx_matcher *m, orbx_keyframe *kf, int32_t *word_id, double *value, int *n_words"
    assert _declaration(h, SYMBOLS[2]) == "int device, int n_slots, int words_cap, orbx_keyframe_database **out"
    assert _declaration(h, SYMBOLS[3]) == "orbx_keyframe_database *db"
    assert _declaration(h, SYMBOLS[4]) == "orbx_matcher *m, orbx_keyframe_database *db, int slot, orbx_keyframe *kf"
    assert _declaration(h, SYMBOLS[5]) == "orbx_matcher *m, orbx_keyframe_database *db, int slot"
    assert _declaration(h, SYMBOLS[6]) == "orbx_matcher *m, orbx_keyframe_database *db"
    assert _declaration(h, SYMBOLS[7]) == "orbx_matcher *m, orbx_keyframe_database *db, orbx_frame *f, " + QUERY_TAIL
    assert _declaration(h, SYMBOLS[8]) == "orbx_matcher *m, orbx_keyframe_database *db, orbx_keyframe *kf, " + QUERY_TAIL
    assert _declaration(h, "orbx_vocabulary_set_word_weights") == "orbx_vocabulary *voc, const double *weight, int n_words"   # keeps its declaration
    for text in ("PARITY UNPINNED", "vit->second += w", "norm += fabs(value)", "score += fabs(vi - wi) - fabs(vi) - fabs(wi)", "return -score / 2.0",
                 "int minCommonWords = maxCommonWords * 0.8f", "spConnectedKF", "GetBestCovisibilityKeyFrames", "KeyFrameDatabase::mMutex",
                 "k_bow_vector", "k_bow_score", "k_bow_select", "ORBX_MAX_DATABASE_SLOTS"):
        assert text in h, text


def test_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    py = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert s in py, s
    import orb_slam3_amd as osa
    for cls, name in PY_NAMES:
        assert callable(getattr(getattr(osa, cls), name)), (cls, name)


def test_argument_counts_match_the_header():
    from orb_slam3_amd import _lib
    h = (ROOT / "include" / "orbx.h").read_text()
    L = _lib.lib()
    for s in SYMBOLS:
        assert len(getattr(L, s).argtypes) == _declaration(h, s).count(",") + 1, s


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in SYMBOLS[:7]:
        assert s + "(" in h, s
    for s in SYMBOLS[7:]:                       # the two queries go through one driver, which is handed the entry point
        assert "return query(" + s + "," in h, s
    for name in ("class DeviceKeyFrameDatabase", "void BowVector(", "void add(", "void erase(", "void clear(", "Candidates queryFrame(", "Candidates queryKeyFrame("):
        assert name in h, name


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that calls the wrappers links against liborbx.so."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, const FrameView &V, const ORBVocabularyDevice &voc) {\n"
                   "    DeviceFrame F(m, 2000);\n"
                   "    F.load(V);\n"
                   "    F.ComputeBoW(m, voc);\n"
                   "    std::vector<int32_t> ids;\n"
                   "    std::vector<double> values;\n"
                   "    F.BowVector(m, ids, values);\n"
                   "    DeviceKeyFrame kf(m, F, nullptr);\n"
                   "    kf.BowFromFrame(m, F);\n"
                   "    kf.BowVector(m, ids, values);\n"
                   "    DeviceKeyFrameDatabase db(100, 2000);\n"
                   "    db.add(m, 3, kf);\n"
                   "    DeviceKeyFrameDatabase::Candidates a = db.queryFrame(m, F), b = db.queryKeyFrame(m, kf, {3}, 0.8f, 10, true);\n"
                   "    db.erase(m, 3);\n"
                   "    db.clear(m);\n"
                   "    return a.nCandidates + b.maxCommonWords + (int)b.slot.size() + (int)b.nCommon.size() + (int)ids.size();\n"
                   "}\n"
                   "int main(int argc, char **) { return argc > 100 ? (int)(size_t)&f : 0; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", str(src), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()


def test_scene_conditions_hold_for_the_reference_alone(oracle):
    """What tests/test_gpu_keyframe_database.py demands of its scenes, asserted on the plain-Python restatement (no device code runs), for every seed
    and both vocabularies: exact common counts of the designed key frames, strict `>` at the threshold, chunk edges, -0.0, the exclusion that moves
    the maximum -- and, on the dense vocabulary, that an order-blind implementation WOULD differ: a word whose sequential value is not count * w, a
    norm and a score that a 64-lane partial sum gets wrong."""
    import bow_database_scene as B
    for seed in B.SEEDS:
        for dense in (True, False):
            B.check_conditions(B.DatabaseScene(oracle, seed, dense))
    B.check_conditions_big(B.BigScene(oracle))
