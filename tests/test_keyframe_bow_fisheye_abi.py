"""BoW on device-resident FISHEYE-STEREO key frames through every layer, without a GPU: the five entry points are exported by liborbx.so, declared
in include/orbx.h, registered by the ctypes loader with argument types, and named by the Python wrapper, the C++ wrapper and the reference-signature
adapter; the C++ wrapper and the adapter compile with the rig forms instantiated (the adapter against oracle/mock_slam)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_keyframe_abi import _dbow2_include

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_keyframe_compute_bow_fisheye", "orbx_keyframe_bow_from_frame_fisheye", "orbx_frame_search_by_bow_resident_fisheye",
           "orbx_keyframe_search_by_bow_fisheye", "orbx_keyframe_search_for_triangulation_fisheye"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in SYMBOLS if s not in exported]


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert "typedef struct orbx_keyframe_kb8_gate {" in h
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, h), s
    # what the user has to know is stated where it is read: the numbering, the refusals of the other kind, the reference lines
    for text in ("FISHEYE-STEREO key frames", "feature numbering", "refuse a monocular one", "ORBmatcher.cc:283-392", ":800-802, :820-822", ":1036-1072",
                 "row extent"):
        assert text in h, text


def test_symbols_are_bound_in_python():
    import ctypes as C
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
    # orbx_keyframe_kb8_gate: two pointers, nlevels, cam1[2][8], cam2[2][8], R12[4][9], t12[4][3], coarse (+ padding to the pointers' alignment)
    G = _lib.KeyFrameKb8Gate
    assert G.nlevels.offset == 2 * C.sizeof(C.c_void_p) and G.cam1.offset == G.nlevels.offset + 4 and G.coarse.offset == G.cam1.offset + 4 * (16 + 16 + 36 + 12)
    assert C.sizeof(G) == (G.coarse.offset + 4 + 7) // 8 * 8
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SYMBOLS:
        assert s in m, s
    import orb_slam3_amd as osa
    for name in ("compute_bow_fisheye", "bow_from_frame_fisheye"):
        assert callable(getattr(osa.DeviceKeyFrame, name)), name
    for name in ("SearchByBoWResidentFisheye", "SearchByBoWKeyFramesResidentFisheye", "SearchForTriangulationResidentKB8"):
        assert callable(getattr(osa.ORBmatcher, name)), name


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in SYMBOLS:
        assert s in h, s
    assert "bool fisheye() const" in h and "static bool allFisheye(" in h
    inl = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher_slam.inl").read_text()
    assert "orbx_keyframe_kb8_gate g;" in inl and "all fisheye-stereo or none" in inl
    assert "resident key frames are monocular / rectified" not in inl      # the three overloads take rig key frames now
    assert "have NOT been run against the compiled reference" in inl       # the text says what these overloads were checked against


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, DeviceFrame &F, const FrameView &V, const std::vector<orbx_keypoint> &kr, const float *isg,\n"
                   "      const ORBVocabularyDevice &voc, const orbx_keyframe_kb8_gate &g) {\n"
                   "    DeviceKeyFrame a(DeviceKeyFrame::Fisheye(), m, F, isg), b(m, V, kr, isg);\n"
                   "    if (!a.fisheye() || !b.fisheye()) return -1;\n"
                   "    std::vector<int32_t> w, nd, nm;\n"
                   "    a.BowFromFrame(m, F);\n"
                   "    b.ComputeBoW(m, voc);\n"
                   "    b.ComputeBoW(m, voc, 4, &w, &nd);\n"
                   "    std::vector<DeviceKeyFrame *> kfs{&a, &b};\n"
                   "    std::vector<std::vector<uint8_t>> valid(2);\n"
                   "    std::vector<std::vector<int32_t>> rows;\n"
                   "    int n = m.SearchByBoW(F, kfs, valid, nm, rows);\n"
                   "    n += m.SearchByBoW(a, valid[0], kfs, {}, nm, rows);\n"
                   "    std::vector<std::pair<size_t, size_t>> pairs;\n"
                   "    return n + m.SearchForTriangulation(a, b, valid[0], valid[1], g, pairs);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_adapter_compiles_with_slam_types(tmp_path):
    """-DORBX_WITH_SLAM_TYPES against oracle/mock_slam: the three reference-typed overloads that take a DeviceKeyFrame* beside each KeyFrame*, with
    the fisheye-stereo branch of each (GetRightPose, mpCamera2, getParameter) instantiated -- compiled, not run: the mock types have no behaviour."""
    inc = _dbow2_include(tmp_path)
    src = tmp_path / "a.cpp"
    src.write_text('#include "oracle/adapter_slam/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, std::vector<KeyFrame *> &kfs, DeviceFrame &DF, Frame &F, const FrameView &V, const std::vector<orbx_keypoint> &kr,\n"
                   "      const float *isg) {\n"
                   "    DeviceKeyFrame a(DeviceKeyFrame::Fisheye(), m, DF, isg), b(m, V, kr, isg);\n"
                   "    std::vector<DeviceKeyFrame *> dev{&a, &b};\n"
                   "    std::vector<std::vector<MapPoint *>> rows;\n"
                   "    std::vector<MapPoint *> row;\n"
                   "    std::vector<int> nm;\n"
                   "    m.SearchByBoW(kfs, dev, F, DF, rows, nm);\n"
                   "    int n = m.SearchByBoW(kfs[0], dev[0], F, DF, row);\n"
                   "    m.SearchByBoW(kfs[0], dev[0], kfs, dev, rows, nm);\n"
                   "    std::vector<std::pair<size_t, size_t>> pairs;\n"
                   "    return n + m.SearchForTriangulation(kfs[0], dev[0], kfs[1], dev[1], pairs, false, false);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DORBX_WITH_SLAM_TYPES", f"-I{ROOT}", f"-I{ROOT / 'oracle' / 'ocv_shim'}",
                        f"-I{ROOT / 'oracle' / 'mock_slam'}", f"-I{inc}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
