"""MapPoint::UpdateNormalAndDepth on resident key frames through every layer, without a GPU: the three entry points are exported by liborbx.so,
declared in include/orbx.h, registered by the ctypes loader with as many argument types as the header declares parameters, named by the Python
wrapper and wrapped in C++, where the wrappers compile and link in a translation unit of their own.  One reference-only test asserts what
tests/test_gpu_normal_depth.py demands of its scenes."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_keyframe_update_normal_and_depth", "orbx_keyframe_update_normal_and_depth_to_map", "orbx_keyframe_refresh_map_points_to_map"]
PY_METHODS = ["UpdateNormalAndDepthKeyFrames", "UpdateNormalAndDepthKeyFramesToMap", "RefreshMapPointsToMap"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + ["orbx_keyframe_distinctive_descriptors", "orbx_keyframe_distinctive_descriptors_to_map", "orbx_map_update"]:   # the others stay
        assert s in exported, s


def _declaration(h, symbol):
    m = re.search(r"\bint\s+%s\(([^;]*)\);" % symbol, h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    lists = "int n_sets, const int32_t *set_ptr, const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *ref_obs"
    head = "orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers, const float *centers_right, " + lists
    assert _declaration(h, SYMBOLS[0]) == head + ", const float *pos, float *normal, float *min_dist, float *max_dist"
    assert _declaration(h, SYMBOLS[1]) == head + ", orbx_map *map, const int32_t *set_id, float *normal, float *min_dist, float *max_dist"
    assert _declaration(h, SYMBOLS[2]) == head + ", orbx_map *map, const int32_t *set_id, int32_t *best_obs"
    # the member, its callers and the contract are stated where the user reads them
    for text in ("MapPoint::UpdateNormalAndDepth", "LocalMapping::ProcessNewKeyFrame", "Tracking::CreateNewKeyFrame", "GetRightCameraCenter()",
                 "ALWAYS the left centre", "Eigen-internal, unpinned", "UNSCALED", "0 / 0 = NaN", "k_normal_depth_kf", "k_map_scatter_refresh",
                 "one 64-byte record per key frame", "before anything is enqueued or a transfer counter moves", "SetWorldPos"):
        assert text in h, text


def test_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    py = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert f"_L.{s}(" in py, s
    import orb_slam3_amd as osa
    for name in PY_METHODS:
        assert callable(getattr(osa.ORBmatcher, name)), name


def test_argument_counts_match_the_header():
    """ctypes checks nothing against the header: the number of registered argument types equals the number of declared parameters."""
    h = (ROOT / "include" / "orbx.h").read_text()
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    vp = i32 = f32 = 1   # noqa: F841  (one parameter each)

    class C:   # noqa: N801
        POINTER = staticmethod(lambda t: 1)
    for s in SYMBOLS:
        expr = re.search(r"L\.%s\.argtypes = (\[.*?\])\n    L\." % s, src, re.S).group(1)
        n = len(eval(expr.replace("\n", " ")))   # the lists hold only vp / i32 / C.POINTER(...)
        assert n == _declaration(h, s).count(",") + 1, (s, n)


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in SYMBOLS:
        assert s + "(" in h, s
    assert len(re.findall(r"void UpdateNormalAndDepth\(const std::vector<DeviceKeyFrame \*> &vpKFs", h)) == 2
    assert "void RefreshMapPoints(const std::vector<DeviceKeyFrame *> &vpKFs" in h


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that calls the three wrappers links against liborbx.so; tests/cpp/adapter_demo.cpp builds as before."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, const FrameView &V) {\n"
                   "    DeviceMap map(64);\n"
                   "    DeviceKeyFrame a(m, V, nullptr), b(m, V, nullptr);\n"
                   "    std::vector<DeviceKeyFrame *> kfs{&a, &b};\n"
                   "    std::vector<int32_t> setPtr{0, 2, 2}, obsKf{0, 1}, obsIdx{0, 0}, refObs{1, 0}, setId{3, 7}, bestObs;\n"
                   "    std::vector<float> centers(6), none, pos(6), normal, mn, mx;\n"
                   "    m.UpdateNormalAndDepth(kfs, centers, none, setPtr, obsKf, obsIdx, refObs, pos, normal, mn, mx);\n"
                   "    m.UpdateNormalAndDepth(kfs, centers, none, setPtr, obsKf, obsIdx, refObs, map, setId);\n"
                   "    m.UpdateNormalAndDepth(kfs, centers, centers, setPtr, obsKf, obsIdx, refObs, map, setId, &normal, &mn, &mx);\n"
                   "    m.RefreshMapPoints(kfs, centers, none, setPtr, obsKf, obsIdx, refObs, map, setId, bestObs);\n"
                   "    m.ComputeDistinctiveDescriptors(kfs, setPtr, obsKf, obsIdx, map, setId, bestObs);\n"
                   "    return bestObs[0] + (int)normal[0] + (int)mn[0] + (int)mx[0];\n"
                   "}\n"
                   "int main(int argc, char **) { return argc > 100 ? (int)(size_t)&f : 0; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", str(src), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
    demo = tmp_path / "adapter_demo"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", str(ROOT / "tests/cpp/adapter_demo.cpp"), "-o", str(demo), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_scene_conditions_hold_for_the_reference_alone():
    """What tests/test_gpu_normal_depth.py demands of its scenes, asserted on the float32 reference (no device code runs), for every seed it uses:
    the order of the sum shows in at least 10 sets of 8 or more observations, at least 5 reference observations are right-camera rows without a left
    one, at least 5 are not in the set's first key frame, both ends of both pyramids occur as reference levels, the rig indices N_left - 1, N_left and
    N - 1 are named, and the only NaN is in the set built for it."""
    import orb_slam3_amd as osa
    assert all(hasattr(osa.ORBmatcher, name) for name in PY_METHODS)   # (these are their inputs)
    import normal_depth_scene as ND
    import test_gpu_normal_depth as TG
    assert len({s for s in ND.SEEDS}) == 3
    for seed in ND.SEEDS:
        sc = ND.make_scene(seed)
        assert set(ND.EDGE_SIZES) <= set(sc["sizes"]) and len(sc["sizes"]) == len(ND.EDGE_SIZES) + ND.N_RANDOM
        ND.check_conditions(sc)
    blocks = ND.make_scene(TG.BLOCK_SEED, n_sets=258)
    assert len(blocks["sizes"]) == 258 and blocks["sizes"][0] == 0 and blocks["sizes"][1] > 0
    ND.check_conditions(blocks)
