"""LoopClosing's Sim3 projection searches on fisheye-stereo resident key frames through every layer, without a GPU: both entry points are exported by
liborbx.so, declared in include/orbx.h with what they restate, registered by the ctypes loader with argument types that match the declarations, and
named by the Python wrapper, the C++ wrapper and the reference-signature adapter, which still compiles with the SLAM types of oracle/mock_slam and
refuses a list of mixed kinds.  One oracle-only test asserts what the GPU tests demand of their inputs."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_keyframe_abi import _dbow2_include

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_keyframe_search_by_projection_sim3_fisheye", "orbx_keyframe_fuse_map_points_sim3_fisheye"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in SYMBOLS if s not in exported]


def _declaration(name):
    h = (ROOT / "include" / "orbx.h").read_text()
    m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, h)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    for s in SYMBOLS:
        _declaration(s)
    # what the calls restate, and their limits, are stated where the user reads them
    for text in ("bRight = false", "KannalaBrandt8::project", "one per key frame, not two", "N_left + N_right", "i >= N_left", ":573-578",
                 "best_idx always below N_left", "a monocular key frame"):
        assert text in h, text


def test_ctypes_signatures_match_the_header():
    """Every argument of the two declarations against the registered ctypes type: pointers (to anything) are pointer-sized types, int is c_int32,
    float is c_float, and the counts agree."""
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    want = {"int": C.c_int32, "float": C.c_float}
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        block = re.search(r"L\.%s\.argtypes = \[(.*?)\]\n" % s, src, re.S)
        assert block, s
        ns = dict(vp=C.c_void_p, i32=C.c_int32, f32=C.c_float, C=C)
        types = eval("[" + block.group(1) + "]", ns)   # noqa: S307 (the loader's own list expression)
        args = _declaration(s)
        assert len(types) == len(args), (s, len(types), len(args))
        for a, t in zip(args, types):
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (s, a, t)
            else:
                assert t is want[a.split()[0]], (s, a, t)
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SYMBOLS:
        assert s in m, s
    import orb_slam3_amd as osa
    assert callable(osa.ORBmatcher.SearchByProjectionSim3KeyFramesFisheye) and callable(osa.ORBmatcher.FuseMapPointsSim3Fisheye)


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    assert "void SearchByProjectionSim3KeyFramesFisheye(" in h and "void FuseMapPointsSim3Fisheye(" in h
    for s in SYMBOLS:
        assert s in h, s
    inl = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher_slam.inl").read_text()
    assert "SearchByProjectionSim3KeyFramesFisheye({pDeviceKF}" in inl and "FuseMapPointsSim3Fisheye(vpDeviceKFs" in inl
    assert "pKF->NLeft != -1" in inl and "GeometricCamera::CAM_FISHEYE" in inl


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, std::vector<DeviceKeyFrame *> &kfs) {\n"
                   "    ORBmatcher::FuseMapPointSet mps;\n"
                   "    std::vector<orbx_fisheye_view> views(kfs.size());\n"
                   "    std::vector<std::vector<int32_t>> match; std::vector<int> nm; std::vector<uint8_t> pr;\n"
                   "    m.SearchByProjectionSim3KeyFramesFisheye(kfs, views, mps, {}, {}, 8.0f, 1.5f, 0.18f, ORBX_SIM3_PROJECT_INVZ, match, nm, &pr);\n"
                   "    std::vector<int32_t> bi, bd;\n"
                   "    m.FuseMapPointsSim3Fisheye(kfs, views, mps, {}, 4.0f, 0.18f, bi, bd, &pr);\n"
                   "    return nm[0] + bi[0];\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _slam_flags(tmp_path):
    inc = _dbow2_include(tmp_path)
    return ["-std=c++17", "-DORBX_WITH_SLAM_TYPES", f"-I{ROOT}", f"-I{ROOT / 'oracle' / 'ocv_shim'}", f"-I{ROOT / 'oracle' / 'mock_slam'}", f"-I{inc}"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_adapter_compiles_with_slam_types(tmp_path):
    """-DORBX_WITH_SLAM_TYPES against oracle/mock_slam: the three reference-typed overloads on resident key frames, which now route a fisheye-stereo
    key frame (NLeft != -1) to the _fisheye calls, are instantiated, and so are the rule and the two calls they route to (`h`: names this adapter did
    not have before).  Compiling shows that the overloads and their targets fit the SLAM types; THAT a rig key frame takes the _fisheye branch is read
    from the source by test_symbols_are_wrapped_in_cpp alone.  They are not run against the compiled reference."""
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
                   "}\n"
                   "int h(ORBmatcher &m, std::vector<KeyFrame *> &kfs, std::vector<DeviceKeyFrame *> &dev) {\n"
                   "    if (!ORBmatcher::sim3_rig_list(kfs)) return 0;\n"
                   "    ORBmatcher::FuseMapPointSet mps;\n"
                   "    std::vector<orbx_fisheye_view> views(dev.size());\n"
                   "    std::vector<std::vector<int32_t>> match; std::vector<int> nm; std::vector<int32_t> bi, bd;\n"
                   "    m.SearchByProjectionSim3KeyFramesFisheye(dev, views, mps, {}, {}, 8.0f, 1.5f, 0.18f, ORBX_SIM3_PROJECT_CAMERA, match, nm);\n"
                   "    m.FuseMapPointsSim3Fisheye(dev, views, mps, {}, 4.0f, 0.18f, bi, bd);\n"
                   "    return nm[0] + bi[0];\n"
                   "}\n")
    r = subprocess.run(["g++", "-fsyntax-only", *_slam_flags(tmp_path), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_a_mixed_list_throws(tmp_path):
    """The rule the resident Fuse(vpKFs, vpDeviceKFs, vScw, ...) applies before it touches the device (ORBmatcher::sim3_rig_list), run on the stand-in
    KeyFrame: all monocular -> false, all fisheye-stereo -> true, an empty list -> false, a mixed list -> std::invalid_argument."""
    oracle_lib = ROOT / "oracle" / "liborb_oracle.so"
    assert oracle_lib.exists(), "build the oracle first (__graft_entry__.build())"
    src = tmp_path / "m.cpp"
    src.write_text('#include "oracle/adapter_slam/ORBmatcher.h"\n'
                   "#include <cstdio>\n"
                   "using namespace ORB_SLAM3;\n"
                   "int main() {\n"
                   "    KeyFrame a, b, c;\n"
                   "    b.NLeft = 100; c.NLeft = 80;\n"
                   "    std::vector<KeyFrame *> mono{&a, &a}, rig{&b, &c}, mixed{&b, &a}, mixed2{&a, &a, &c}, none;\n"
                   "    if (ORBmatcher::sim3_rig_list(mono) || !ORBmatcher::sim3_rig_list(rig) || ORBmatcher::sim3_rig_list(none)) return 1;\n"
                   "    int thrown = 0;\n"
                   "    for (auto *l : {&mixed, &mixed2}) {\n"
                   "        try { ORBmatcher::sim3_rig_list(*l); } catch (const std::invalid_argument &) { thrown++; }\n"
                   "    }\n"
                   '    if (thrown != 2) return 2;\n'
                   '    printf("mixed lists throw\\n");\n'
                   "    return 0;\n"
                   "}\n")
    exe = tmp_path / "mixed"
    r = subprocess.run(["g++", "-O0", *_slam_flags(tmp_path), str(src), "-o", str(exe), f"-L{oracle_lib.parent}", "-lorb_oracle",
                        f"-Wl,-rpath,{oracle_lib.parent}", "-Wl,--unresolved-symbols=ignore-all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "mixed lists throw" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_scene_conditions_hold_for_the_oracle_alone(oracle):
    """What tests/test_gpu_keyframe_sim3_fisheye.py demands of its inputs, asserted on the composed reference (no device code runs), with the search
    form's equal bounds and with per-key-frame bounds: per seed at least half of the pairs pass the gates, a fifth is matched, 8 queries lose their
    independent best feature to an earlier query, every gate removes 1 % of the pairs, the left camera's exact-mnMaxX point and its 6 / 6 angle points
    exist, and per key frame the invz form decides 20 pairs differently from the camera form and still matches 20 features."""
    import sim3_fisheye_scene as SF
    import test_gpu_keyframe_fisheye as TF
    for seed, K in SF.SEEDS.items():
        for bounds in (SF.EQUAL, TF.BOUNDS[:K]):
            sc = SF.make_scene(oracle, seed, K, bounds=bounds)
            fig = SF.check_conditions(oracle, sc, range(K))
            assert fig["stolen"] >= 8 and min(fig["invz_differ"]) >= 20 and min(fig["invz_matches"]) >= 20, (seed, fig)
            for kf in sc["key_frames"]:
                assert 150 <= len(kf["kps_left"]) <= 300 and 100 <= len(kf["kps_right"]) <= 250
