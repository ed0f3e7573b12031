"""BoW and the relocalization window search on fisheye-stereo frame handles through every layer, without a GPU: every new entry point is exported
by liborbx.so, declared in include/orbx.h, registered by the ctypes loader, and named by the Python and the C++ wrappers."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BOW_FISHEYE_SYMBOLS = ["orbx_frame_compute_bow_fisheye", "orbx_frame_search_by_bow_fisheye", "orbx_frame_search_by_projection_window_fisheye"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_bow_fisheye_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in BOW_FISHEYE_SYMBOLS if s not in exported]


def test_bow_fisheye_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    for s in BOW_FISHEYE_SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, h), s
    assert "BoW on a fisheye handle is not there yet" not in (ROOT / "INTEGRATION.md").read_text()


def test_bow_fisheye_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in BOW_FISHEYE_SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert s in m, s
    import orb_slam3_amd as osa
    from orb_slam3_amd.matcher import ORBmatcher
    assert callable(osa.DeviceFrame.compute_bow_fisheye)
    assert callable(ORBmatcher.SearchByBoWDeviceFisheye) and callable(ORBmatcher.SearchByProjectionWindowFisheye)


def test_bow_fisheye_argtypes_match_the_monocular_forms():
    """Same C signatures as orbx_frame_compute_bow / orbx_frame_search_by_bow / orbx_frame_search_by_projection_window (the loader is built without
    opening liborbx.so's GPU side: ctypes only resolves the symbols)."""
    from orb_slam3_amd import _lib
    L = _lib.lib()
    for mono, fish in zip(["orbx_frame_compute_bow", "orbx_frame_search_by_bow", "orbx_frame_search_by_projection_window"], BOW_FISHEYE_SYMBOLS):
        assert getattr(L, fish).argtypes == getattr(L, mono).argtypes, fish


def test_bow_fisheye_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in ("ComputeBoWFisheye(", "SearchByBoWFisheye(DeviceFrame &", "SearchByProjectionWindowFisheye(DeviceFrame &"):
        assert s in h, s
    for s in BOW_FISHEYE_SYMBOLS:
        assert s in h, s
    inl = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher_slam.inl").read_text()
    for s in ("SearchByBoWFisheye(const std::vector<KeyFrame *> &vpKFs, Frame &F, DeviceFrame &DF", "SearchByBoWFisheye(KeyFrame *pKF, Frame &F, DeviceFrame &DF",
              "SearchByProjectionFisheye(Frame &CurrentFrame, DeviceFrame &DF, KeyFrame *pKF"):
        assert s in inl, s


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_bow_fisheye_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "int f(ORB_SLAM3::ORBmatcher &m, const ORB_SLAM3::ORBVocabularyDevice &voc, orbx_extractor *l, orbx_extractor *r) {\n"
                   "    ORB_SLAM3::DeviceFrame F(m, 4000);\n"
                   "    F.loadStereoFisheyeBatch(l, r, 0);\n"
                   "    F.ComputeBoWFisheye(m, voc, 4);\n"
                   "    std::vector<int32_t> wid, nid, match, nm;\n"
                   "    F.ComputeBoWFisheye(m, voc, 2, &wid, &nid);\n"
                   "    std::vector<orbx_bow_keyframe> kfs;\n"
                   "    std::vector<std::vector<int32_t>> rows;\n"
                   "    ORB_SLAM3::ORBmatcher::WindowQueries q;\n"
                   "    return m.SearchByBoWFisheye(F, kfs, nm, rows) + m.SearchByProjectionWindowFisheye(F, {}, q, 100.f, true, match);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
