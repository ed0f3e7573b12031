"""Fisheye-stereo resident key frames (orbx_keyframe_*_fisheye) and their one-call Fuse through every layer, without a GPU: the five entry points
are exported by liborbx.so, declared in include/orbx.h, registered by the ctypes loader with argument types, and named by the Python wrapper, the C++
wrapper and the reference-signature adapter; the adapter still compiles with the SLAM types of oracle/mock_slam."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_keyframe_abi import _dbow2_include

ROOT = Path(__file__).resolve().parent.parent
FISHEYE_SYMBOLS = ["orbx_keyframe_from_frame_fisheye", "orbx_keyframe_create_host_fisheye", "orbx_keyframe_counts",
                   "orbx_keyframe_fuse_search_fisheye", "orbx_keyframe_fuse_map_points_fisheye"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_fisheye_keyframe_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in FISHEYE_SYMBOLS if s not in exported]


def test_fisheye_keyframe_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    for s in FISHEYE_SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, h), s
    # what the object holds and leaves out, the numbering and the reference lines are stated where the user reads them
    for text in ("mvKeysRight", "mvLeftToRightMatch / mvRightToLeftMatch", "N_left + j", "ORBmatcher.cc:1296", "GetRightPose()", "GetRightCameraCenter()",
                 "strict on the max side", "Not covered"):
        assert text in h, text


def test_fisheye_keyframe_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in FISHEYE_SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert s in m, s
    import orb_slam3_amd as osa
    for name in ("from_frame_fisheye", "from_host_fisheye", "counts"):
        assert callable(getattr(osa.DeviceKeyFrame, name)), name
    assert callable(osa.ORBmatcher.FuseSearchKeyFramesFisheye) and callable(osa.ORBmatcher.FuseMapPointsFisheye)
    from orb_slam3_amd import synth
    assert callable(synth.make_fisheye_fuse_scene)


def test_fisheye_keyframe_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    assert "void FuseSearchKeyFramesFisheye(" in h and "void FuseMapPointsFisheye(" in h
    for s in FISHEYE_SYMBOLS:
        assert s in h, s
    inl = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher_slam.inl").read_text()
    assert "FuseSearchKeyFramesFisheye(vpDeviceKFs" in inl and "GetRightPose()" in inl and "targets in one list" in inl


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, DeviceFrame &F, const FrameView &left, const std::vector<orbx_keypoint> &kr, const float *isg) {\n"
                   "    DeviceKeyFrame a(DeviceKeyFrame::Fisheye{}, m, F, isg), b(m, left, kr, isg);\n"
                   "    std::vector<DeviceKeyFrame *> kfs{&a, &b};\n"
                   "    std::vector<ORBmatcher::FuseQueries> q(4);\n"
                   "    std::vector<std::vector<int32_t>> bi, bd;\n"
                   "    m.FuseSearchKeyFramesFisheye(kfs, q, true, bi, bd);\n"
                   "    ORBmatcher::FuseMapPointSet mps;\n"
                   "    std::vector<orbx_fisheye_view> views(4);\n"
                   "    std::vector<int32_t> i3, d3; std::vector<uint8_t> pr;\n"
                   "    m.FuseMapPointsFisheye(kfs, views, mps, {}, 3.0f, 0.18f, i3, d3, &pr);\n"
                   "    int nl = 0, nr = 0;\n"
                   "    a.counts(nl, nr);\n"
                   "    return nl + nr + b.count();\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_adapter_compiles_with_slam_types(tmp_path):
    """-DORBX_WITH_SLAM_TYPES against oracle/mock_slam: the fisheye DeviceKeyFrame constructors, the two C++ members and the reference-typed
    Fuse(vpTargetKFs, vpDeviceKFs, vpMapPoints, th), which takes all-fisheye targets, are instantiated."""
    inc = _dbow2_include(tmp_path)
    src = tmp_path / "a.cpp"
    src.write_text('#include "oracle/adapter_slam/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "std::vector<int> f(ORBmatcher &m, DeviceFrame &F, const FrameView &left, const std::vector<orbx_keypoint> &kr, KeyFrame *pKF,\n"
                   "                   std::vector<MapPoint *> &mps) {\n"
                   "    DeviceKeyFrame a(DeviceKeyFrame::Fisheye{}, m, F, pKF->mvInvLevelSigma2.data()), b(m, left, kr, pKF->mvInvLevelSigma2.data());\n"
                   "    std::vector<DeviceKeyFrame *> dev{&a, &b};\n"
                   "    std::vector<KeyFrame *> kfs{pKF, pKF};\n"
                   "    std::vector<ORBmatcher::FuseQueries> q(4);\n"
                   "    std::vector<std::vector<int32_t>> bi, bd;\n"
                   "    m.FuseSearchKeyFramesFisheye(dev, q, true, bi, bd);\n"
                   "    ORBmatcher::FuseMapPointSet flat;\n"
                   "    std::vector<orbx_fisheye_view> views(4);\n"
                   "    std::vector<int32_t> i3, d3;\n"
                   "    m.FuseMapPointsFisheye(dev, views, flat, {}, 3.0f, 0.18f, i3, d3);\n"
                   "    return m.Fuse(kfs, dev, mps, 3.0f);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DORBX_WITH_SLAM_TYPES", f"-I{ROOT}", f"-I{ROOT / 'oracle' / 'ocv_shim'}",
                        f"-I{ROOT / 'oracle' / 'mock_slam'}", f"-I{inc}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
