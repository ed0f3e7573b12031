"""The device-resident map-point table and the `_map` forms through every layer, without a GPU: each entry point is exported by liborbx.so,
declared in include/orbx.h, registered by the ctypes loader with argument types, named by the Python wrapper and wrapped in C++, where the wrappers
compile and link in a translation unit of their own.  The oracle-only tests assert what tests/test_gpu_map.py demands of its scenes."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
TABLE = ["orbx_map_create", "orbx_map_destroy", "orbx_map_update", "orbx_map_erase", "orbx_map_read"]
FLAT = ["orbx_frame_search_local_points", "orbx_frame_search_local_points_fisheye", "orbx_keyframe_fuse_map_points",
        "orbx_keyframe_fuse_map_points_fisheye", "orbx_keyframe_fuse_map_points_sim3", "orbx_keyframe_fuse_map_points_sim3_fisheye",
        "orbx_keyframe_search_by_projection_sim3", "orbx_keyframe_search_by_projection_sim3_fisheye"]
SEARCHES = [s + "_map" for s in FLAT]
SYMBOLS = TABLE + SEARCHES + ["orbx_keyframe_distinctive_descriptors_to_map"]
PY_METHODS = ["SearchLocalPointsMap", "SearchLocalPointsFisheyeMap", "FuseMapPointsMap", "FuseMapPointsFisheyeMap", "FuseMapPointsSim3Map",
              "FuseMapPointsSim3FisheyeMap", "SearchByProjectionSim3KeyFramesMap", "SearchByProjectionSim3KeyFramesFisheyeMap",
              "DistinctiveDescriptorsKeyFramesToMap"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + FLAT + ["orbx_keyframe_distinctive_descriptors"]:   # the flat calls stay
        assert s in exported, s


def _declaration(h, symbol):
    m = re.search(r"\b(?:int|void)\s+%s\(([^;]*)\);" % symbol, h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert "typedef struct orbx_map orbx_map;" in h
    limit = re.search(r"#define\s+ORBX_MAX_MAP_POINTS\s+\(1 << (\d+)\)", h)
    assert limit and int(limit.group(1)) == 24
    for s in SYMBOLS:
        _declaration(h, s)
    five = "const float *pos, const float *normal, const float *min_dist, const float *max_dist, const uint8_t *mp_desc"
    for flat in FLAT:   # a `_map` form is its flat form with the five arrays replaced by (map, ids)
        want = _declaration(h, flat)
        assert five in want, flat
        want = re.sub(r"\borbx_frame \*\w+", "orbx_frame *", want.replace(five, "orbx_map *map, const int32_t *ids"))
        assert re.sub(r"\borbx_frame \*\w+", "orbx_frame *", _declaration(h, flat + "_map")) == want, flat
    assert _declaration(h, "orbx_keyframe_distinctive_descriptors_to_map") == _declaration(h, "orbx_keyframe_distinctive_descriptors").replace(
        "int32_t *best_obs, uint8_t *best_desc", "orbx_map *map, const int32_t *set_id, int32_t *best_obs")
    # the contract is stated where the user reads it
    for text in ("Map::mMutexMapUpdate", "SetBadFlag", "`written`", "ORBX_E_TOO_LARGE beyond", "k_map_gather", "k_map_scatter", "k_map_scatter_desc",
                 "BEFORE anything is enqueued", "never ids", "orbx_map_destroy waits"):
        assert text in h, text


def test_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    py = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert f"_L.{s}(" in py, s
    h = (ROOT / "include" / "orbx.h").read_text()
    assert _lib.MAX_MAP_POINTS == 1 << int(re.search(r"#define\s+ORBX_MAX_MAP_POINTS\s+\(1 << (\d+)\)", h).group(1))
    import orb_slam3_amd as osa
    for name in ("update", "erase", "read", "close"):
        assert callable(getattr(osa.DeviceMap, name))
    for name in PY_METHODS:
        assert callable(getattr(osa.ORBmatcher, name)), name


def test_argument_counts_match_the_header():
    """ctypes checks nothing against the header: the number of registered argument types equals the number of declared parameters."""
    h = (ROOT / "include" / "orbx.h").read_text()
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    vp = i32 = f32 = 1   # noqa: F841  (one parameter each)

    class C:   # noqa: N801
        POINTER = staticmethod(lambda t: 1)
    Camera = FramePose = 1   # noqa: F841, N806
    for s in SYMBOLS:
        expr = re.search(r"L\.%s\.argtypes = (\[.*?\])\n    L\." % s, src, re.S).group(1)
        n = len(eval(expr.replace("\n", " ")))   # the lists hold only vp / i32 / f32 / C.POINTER(...) and arithmetic on lists of them
        assert n == _declaration(h, s).count(",") + 1, (s, n)


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in SYMBOLS:
        assert s + "(" in h, s
    assert "class DeviceMap {" in h and "const DeviceMap &map, const std::vector<int32_t> &ids" in h


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that calls every new wrapper links against liborbx.so; tests/cpp/adapter_demo.cpp builds as before."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, const FrameView &V, DeviceFrame &F, DeviceFrame &R) {\n"
                   "    DeviceMap map(1024);\n"
                   "    std::vector<int32_t> ids{3, 7}, bestIdx, bestDist, bestObs, vpMatch, setPtr{0, 1, 2}, obsKf{0, 0}, obsIdx{0, 1};\n"
                   "    std::vector<float> pos(6), normal(6), mn(2), mx(2);\n"
                   "    std::vector<uint8_t> desc(64), none, inView, projected;\n"
                   "    map.update(m, ids, pos.data(), normal.data(), mn.data(), mx.data(), desc.data());\n"
                   "    map.update(m, ids, nullptr, nullptr, nullptr, nullptr, desc.data());\n"
                   "    map.read(m, ids, pos.data(), normal.data(), mn.data(), mx.data(), desc.data());\n"
                   "    DeviceKeyFrame a(m, V, nullptr), b(m, V, std::vector<orbx_keypoint>(), nullptr);\n"
                   "    std::vector<DeviceKeyFrame *> kfs{&a}, rigs{&b};\n"
                   "    std::vector<orbx_camera> cams(1);\n"
                   "    std::vector<orbx_frame_pose> poses(1);\n"
                   "    std::vector<orbx_fisheye_view> views(2), left(1), noViews;\n"
                   "    std::vector<std::vector<uint8_t>> occupied;\n"
                   "    std::vector<std::vector<int32_t>> rows;\n"
                   "    std::vector<int> nm;\n"
                   "    int n = m.SearchLocalPoints(F, none, cams[0], poses[0], 0.18f, 0.5f, map, ids, none, none, 3.f, false, 0.f, inView, vpMatch);\n"
                   "    n += m.SearchLocalPointsFisheye(R, none, views.data(), 0.18f, 0.5f, map, ids, none, none, std::vector<float>(), 3.f, false, 0.f, inView,\n"
                   "                                    vpMatch);\n"
                   "    m.FuseMapPoints(kfs, cams, poses, map, ids, none, 3.f, 0.18f, bestIdx, bestDist, &projected);\n"
                   "    m.FuseMapPointsFisheye(rigs, views, map, ids, none, 3.f, 0.18f, bestIdx, bestDist);\n"
                   "    m.FuseMapPointsSim3(kfs, cams, poses, map, ids, none, 3.f, 0.18f, bestIdx, bestDist);\n"
                   "    m.FuseMapPointsSim3Fisheye(rigs, left, map, ids, none, 3.f, 0.18f, bestIdx, bestDist);\n"
                   "    m.SearchByProjectionSim3KeyFrames(kfs, cams, poses, noViews, map, ids, none, occupied, 8.f, 1.5f, 0.18f, ORBX_SIM3_PROJECT_CAMERA, rows, nm);\n"
                   "    m.SearchByProjectionSim3KeyFrames(rigs, {}, {}, left, map, ids, none, occupied, 8.f, 1.5f, 0.18f, ORBX_SIM3_PROJECT_INVZ, rows, nm);\n"
                   "    m.ComputeDistinctiveDescriptors(kfs, setPtr, obsKf, obsIdx, map, ids, bestObs);\n"
                   "    map.erase(ids);\n"
                   "    return n + bestObs[0] + bestIdx[0] + nm[0];\n"
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


def test_sim3_scenes_meet_the_gpu_tests_conditions_on_the_oracle_alone(oracle):
    """The scenes test_gpu_map.py hands to the six key-frame `_map` calls (seed 5, K = 3, 300 map points), on the reference alone: at least one
    accepted and one rejected pair per gate family -- check_conditions asserts every gate removes pairs, the edge and angle points fall on their
    sides, and half or more of the pairs pass -- and matches are found."""
    import orb_slam3_amd as osa
    assert hasattr(osa.ORBmatcher, "SearchByProjectionSim3KeyFramesMap")   # (these are its inputs)
    import sim3_fisheye_scene as SF
    import sim3_scene as S
    for fig in (S.check_conditions(oracle, S.make_scene(5, 3), range(3)), SF.check_conditions(oracle, SF.make_scene(oracle, 5, 3), range(3))):
        assert fig["projected"] >= 0.5 and fig["matched"] >= 0.2
        for gate in ("behind", "image", "below", "above", "angle"):
            assert 0.0 < fig[gate] < 1.0 - fig["projected"] + 1e-9, (gate, fig)


def test_fuse_and_distinctive_inputs_on_the_oracle_alone(oracle):
    """Fuse proper on the same scenes (the chi2 gate and mvuRight; a rig: both cameras): the existing tests' references accept and reject pairs,
    and the distinctive sets hold one empty set and winners other than row 0."""
    import orb_slam3_amd as osa
    assert hasattr(osa.ORBmatcher, "FuseMapPointsMap") and hasattr(osa.ORBmatcher, "DistinctiveDescriptorsKeyFramesToMap")
    import distinctive_sets as DS
    import sim3_fisheye_scene as SF
    import sim3_scene as S
    import test_gpu_keyframe as T
    import test_gpu_keyframe_fisheye as TF
    for mod, sc in ((T, S.make_scene(5, 3)), (TF, SF.make_scene(oracle, 5, 3))):
        bi, bd, pr = mod._reference(oracle, sc, range(3))[:3]
        assert 0.25 * pr.size <= pr.sum() < pr.size
        assert ((bd <= mod.TH_LOW) & (pr == 1)).sum() >= 100 and ((bd > mod.TH_LOW) & (pr == 1)).sum() >= 1
    D = DS.boundary_sets()
    want = oracle.distinctive_descriptors(D["rows"], D["set_ptr"])
    assert (want < 0).sum() == 1 and (want > 0).sum() >= 50
