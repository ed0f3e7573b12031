"""LoopClosing's Sim3 projection searches on resident key frames through every layer, without a GPU: both entry points are exported by liborbx.so,
declared in include/orbx.h with the reference lines they replace, registered by the ctypes loader with argument types, and named by the Python
wrapper, the C++ wrapper and the reference-signature adapter, which still compiles with the SLAM types of oracle/mock_slam.  One oracle-only test
asserts what the GPU tests demand of their inputs."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_keyframe_abi import _dbow2_include

ROOT = Path(__file__).resolve().parent.parent
SIM3_SYMBOLS = ["orbx_keyframe_search_by_projection_sim3", "orbx_keyframe_fuse_map_points_sim3"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_sim3_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in SIM3_SYMBOLS if s not in exported]


def test_sim3_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    for s in SIM3_SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, h), s
    assert re.search(r"#define\s+ORBX_SIM3_PROJECT_CAMERA\s+0\b", h) and re.search(r"#define\s+ORBX_SIM3_PROJECT_INVZ\s+1\b", h)
    # the reference lines each entry point replaces, the callers, and the equal-bounds limit are stated where the user reads them
    for text in ("ORBmatcher.cc:427-532", ":534-646", "ORBmatcher.cc:1339-1455", ":573-578", "LoopClosing::SearchAndFuse", "LoopClosing.cc:755,777,964",
                 "bit-equal image bounds", "strict on the max side", "ORBX_MAX_FRAME_FEATURES"):
        assert text in h, text


def test_sim3_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    for s in SIM3_SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
    assert (_lib.SIM3_PROJECT_CAMERA, _lib.SIM3_PROJECT_INVZ) == (0, 1)
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SIM3_SYMBOLS:
        assert s in m, s
    import orb_slam3_amd as osa
    assert callable(osa.ORBmatcher.SearchByProjectionSim3KeyFrames) and callable(osa.ORBmatcher.FuseMapPointsSim3)


def test_sim3_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    assert "void SearchByProjectionSim3KeyFrames(" in h and "void FuseMapPointsSim3(" in h
    for s in SIM3_SYMBOLS:
        assert s in h, s
    inl = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher_slam.inl").read_text()
    assert re.search(r"int SearchByProjection\(KeyFrame \*pKF, DeviceKeyFrame \*pDeviceKF, Sophus::Sim3f &Scw,", inl)
    assert re.search(r"int SearchByProjection\(KeyFrame \*pKF, DeviceKeyFrame \*pDeviceKF, Sophus::Sim3<float> &Scw,", inl)
    assert re.search(r"std::vector<int> Fuse\(const std::vector<KeyFrame \*> &vpKFs, const std::vector<DeviceKeyFrame \*> &vpDeviceKFs, "
                     r"std::vector<Sophus::Sim3f> &vScw,", inl)
    assert "ORBX_SIM3_PROJECT_CAMERA" in inl and "ORBX_SIM3_PROJECT_INVZ" in inl and "FuseMapPointsSim3(vpDeviceKFs" in inl


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, const FrameView &V) {\n"
                   "    DeviceKeyFrame a(m, V, nullptr), b(m, V, nullptr);\n"
                   "    std::vector<DeviceKeyFrame *> kfs{&a, &b};\n"
                   "    ORBmatcher::FuseMapPointSet mps;\n"
                   "    std::vector<orbx_camera> cams(2); std::vector<orbx_frame_pose> poses(2);\n"
                   "    std::vector<std::vector<int32_t>> match; std::vector<int> nm; std::vector<uint8_t> pr;\n"
                   "    m.SearchByProjectionSim3KeyFrames(kfs, cams, poses, mps, {}, {}, 8.0f, 1.5f, 0.18f, ORBX_SIM3_PROJECT_INVZ, match, nm, &pr);\n"
                   "    std::vector<int32_t> bi, bd;\n"
                   "    m.FuseMapPointsSim3(kfs, cams, poses, mps, {}, 4.0f, 0.18f, bi, bd, &pr);\n"
                   "    return nm[0] + bi[0];\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_adapter_compiles_with_slam_types(tmp_path):
    """-DORBX_WITH_SLAM_TYPES against oracle/mock_slam: the three reference-typed overloads on resident key frames are instantiated.  They are not run
    against the compiled reference (the stand-in MapPoint has no unscaled distance getters: the overloads would throw)."""
    inc = _dbow2_include(tmp_path)
    src = tmp_path / "a.cpp"
    src.write_text('#include "oracle/adapter_slam/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, KeyFrame *kf, DeviceKeyFrame *dev, Sophus::Sim3f &S, std::vector<MapPoint *> &pts, std::vector<KeyFrame *> &ptKFs,\n"
                   "      std::vector<MapPoint *> &matched, std::vector<KeyFrame *> &matchedKF) {\n"
                   "    return m.SearchByProjection(kf, dev, S, pts, matched, 8, 1.5f) + m.SearchByProjection(kf, dev, S, pts, ptKFs, matched, matchedKF, 3, 1.5f);\n"
                   "}\n"
                   "std::vector<int> g(ORBmatcher &m, std::vector<KeyFrame *> &kfs, std::vector<DeviceKeyFrame *> &dev, std::vector<Sophus::Sim3f> &vS,\n"
                   "                   std::vector<MapPoint *> &pts, std::vector<std::vector<MapPoint *>> &rep) {\n"
                   "    return m.Fuse(kfs, dev, vS, pts, 4.0f, rep);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DORBX_WITH_SLAM_TYPES", f"-I{ROOT}", f"-I{ROOT / 'oracle' / 'ocv_shim'}",
                        f"-I{ROOT / 'oracle' / 'mock_slam'}", f"-I{inc}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_scene_conditions_hold_for_the_oracle_alone(oracle):
    """What tests/test_gpu_keyframe_sim3.py demands of its inputs, asserted on the composed reference (no device code runs): per seed at least half of
    the pairs pass the gates, a fifth is matched, 8 queries lose their independent best feature to an earlier query, every gate removes 1 % of the
    pairs, the exact-mnMaxX points and the 12 / 12 angle points exist, and 20 pairs per key frame project to different bits in the two forms."""
    import sim3_scene as S
    for seed, K in S.SEEDS.items():
        fig = S.check_conditions(oracle, S.make_scene(seed, K), range(K))
        assert fig["stolen"] >= 8 and min(fig["uv_differ"]) >= 20, (seed, fig)
