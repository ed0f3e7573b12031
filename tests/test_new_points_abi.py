"""LocalMapping::CreateNewMapPoints' triangulation on resident key frames through every layer, without a GPU: the four entry points are exported by
liborbx.so, declared in include/orbx.h, registered by the ctypes loader with as many argument types as the header declares parameters, named by the
Python wrapper and wrapped in C++, where the wrappers compile and link in a translation unit of their own; the ORBX_NEWPT_* values are the header's
in every layer.  One reference-only test asserts what tests/test_gpu_new_points.py demands of its scenes, for every seed it uses."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_keyframe_triangulate_pairs", "orbx_keyframe_triangulate_pairs_fisheye", "orbx_keyframe_search_and_triangulate",
           "orbx_keyframe_search_and_triangulate_fisheye"]
PY_METHODS = ["TriangulatePairsKeyFrames", "TriangulatePairsKeyFramesKB8", "SearchAndTriangulateResident", "SearchAndTriangulateResidentKB8"]
STATUS = ["OK", "NO_MATCH", "LOW_PARALLAX", "TRIANGULATE_FAILED", "BEHIND_1", "BEHIND_2", "REPROJ_1", "REPROJ_2", "ZERO_DIST", "FAR", "SCALE_RATIO",
          "STEREO_LEFT_TO_HOST"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + ["orbx_keyframe_search_for_triangulation", "orbx_keyframe_search_for_triangulation_fisheye", "orbx_map_update"]:   # the others stay
        assert s in exported, s


def _declaration(h, symbol):
    m = re.search(r"\bint\s+%s\(([^;]*)\);" % symbol, h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    tail = "const orbx_new_points_params *par, int n_pairs, const int32_t *idx1, const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted"
    assert _declaration(h, SYMBOLS[0]) == ("orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_new_points_view *view1, "
                                           "const orbx_new_points_view *view2, " + tail)
    assert _declaration(h, SYMBOLS[1]) == ("orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_fisheye_view *views1, "
                                           "const orbx_fisheye_view *views2, " + tail)
    head = "orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2, int check_orientation, "
    tail = "const orbx_new_points_params *par, int32_t *matches12, float *pos, uint8_t *status, int *n_accepted"
    assert _declaration(h, SYMBOLS[2]) == (head + "const orbx_keyframe_gate *gate, const orbx_new_points_view *view1, const orbx_new_points_view *view2, "
                                           + tail)
    assert _declaration(h, SYMBOLS[3]) == (head + "const orbx_keyframe_kb8_gate *gate, const orbx_fisheye_view *views1, const orbx_fisheye_view *views2, "
                                           + tail)
    # the search calls this one runs behind keep their declarations
    assert _declaration(h, "orbx_keyframe_search_for_triangulation") == head + "const orbx_keyframe_gate *gate, int32_t *matches12"
    # the member, its contract and what is left out are stated where the user reads them
    for text in ("LocalMapping::CreateNewMapPoints", "GeometricTools::Triangulate", "PARITY UNPINNED", "cosParallaxStereo = cosParallaxRays + 1",
                 "mbInertial ? 0.9996 : 0.9998", "x3Dh(3) == 0", "5.991 * mvLevelSigma2_1[kp1.octave]", "ratioFactor = 1.5f * KF1.mfScaleFactor",
                 "ORBX_NEWPT_STEREO_LEFT_TO_HOST", "mvDepth", "k_new_points", "before anything is enqueued or a transfer counter moves", "`_to_map` form",
                 "orbx_map_update", "there is no batched form"):
        assert text in h, text


def test_status_values_are_the_headers_in_every_layer():
    h = (ROOT / "include" / "orbx.h").read_text()
    from orb_slam3_amd import _lib
    import new_points_scene as S
    for value, name in enumerate(STATUS):
        m = re.search(r"\bORBX_NEWPT_%s = (\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
        assert getattr(_lib, "NEWPT_" + name) == value and _lib.NEWPT_STATUS[value] == name
        assert getattr(S, name) == value and S.STATUS[value] == name
    assert len(_lib.NEWPT_STATUS) == len(S.STATUS) == len(STATUS) == len(re.findall(r"\bORBX_NEWPT_[A-Z_0-9]+ = \d+", h))


def test_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    py = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert f'"{s}"' in py, s
    import orb_slam3_amd as osa
    for name in PY_METHODS:
        assert callable(getattr(osa.ORBmatcher, name)), name


def test_argument_counts_and_struct_sizes_match_the_header():
    """ctypes checks nothing against the header: the number of registered argument types equals the number of declared parameters, and the two
    structures have the size the C compiler gives them (19 floats; 4 + 4 + 4 + 4 + 4 + 4 + 8 + 8 bytes)."""
    import ctypes as C
    from orb_slam3_amd import _lib
    h = (ROOT / "include" / "orbx.h").read_text()
    L = _lib.lib()
    for s in SYMBOLS:
        assert len(getattr(L, s).argtypes) == _declaration(h, s).count(",") + 1, s
    assert C.sizeof(_lib.NewPointsView) == 19 * 4 and C.sizeof(_lib.NewPointsParams) == 40
    fields = re.search(r"typedef struct orbx_new_points_params \{(.*?)\} orbx_new_points_params;", h, re.S).group(1)
    names = [n for decl in re.findall(r"(?:float|int|const float \*)\s*([^;]+);", fields) for n in re.split(r",\s*\*?", decl.strip().lstrip("*"))]
    assert names == [f[0] for f in _lib.NewPointsParams._fields_], names


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in SYMBOLS:
        assert s + "(" in h, s
    assert len(re.findall(r"int TriangulatePairs\(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2", h)) == 2
    assert len(re.findall(r"int SearchAndTriangulate\(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2", h)) == 2
    inl = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher_slam.inl").read_text()
    assert "TriangulatePairs" not in inl and "SearchAndTriangulate" not in inl      # no reference-typed overload (the mock KeyFrame has no poses)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that calls the four wrappers links against liborbx.so; tests/cpp/adapter_demo.cpp builds as before."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, const FrameView &V) {\n"
                   "    DeviceKeyFrame a(m, V, nullptr), b(m, V, nullptr);\n"
                   "    orbx_new_points_view v1{}, v2{};\n"
                   "    orbx_fisheye_view r1[2] = {}, r2[2] = {};\n"
                   "    float sigma[8] = {1, 1, 1, 1, 1, 1, 1, 1};\n"
                   "    orbx_new_points_params par{1.8f, 0, 0, 0.f, 8, 8, sigma, sigma};\n"
                   "    orbx_keyframe_gate g{};\n"
                   "    orbx_keyframe_kb8_gate gk{};\n"
                   "    std::vector<int32_t> i1{0, 1}, i2{1, -1};\n"
                   "    std::vector<float> pos;\n"
                   "    std::vector<uint8_t> status, none;\n"
                   "    std::vector<std::pair<size_t, size_t>> pairs;\n"
                   "    int acc = m.TriangulatePairs(a, b, v1, v2, par, i1, i2, pos, status);\n"
                   "    acc += m.TriangulatePairs(a, b, r1, r2, par, i1, i2, pos, status);\n"
                   "    int nacc = 0;\n"
                   "    acc += m.SearchAndTriangulate(a, b, none, none, g, v1, v2, par, pairs, pos, status, nacc);\n"
                   "    acc += m.SearchAndTriangulate(a, b, none, none, gk, r1, r2, par, pairs, pos, status, nacc);\n"
                   "    return acc + nacc + (int)pos[0] + status[0] + (status[1] == ORBX_NEWPT_NO_MATCH);\n"
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
    """What tests/test_gpu_new_points.py demands of its scenes, asserted on the float32 reference (no device code runs), for every seed it uses and
    both kinds: every status but TRIANGULATE_FAILED at least three times over the scene's parameter variants (the rig has no stereo pairs), at least
    30 % accepted, ten accepted pairs with different octaves, five accepted pairs in each camera combination of the rig, the indices N_left - 1 and
    N_left on both sides, three pairs with mvuRight >= 0 on one side only, no NaN among the accepted positions -- and TRIANGULATE_FAILED itself under
    the degenerate pose, which is how it reaches the tests through the entry point."""
    import orb_slam3_amd as osa
    assert all(hasattr(osa.ORBmatcher, name) for name in PY_METHODS)   # (these are their inputs)
    import new_points_scene as S
    assert len(set(S.SEEDS)) == 2
    for seed in S.SEEDS:
        for rig in (False, True):
            sc = S.make_scene(seed, rig)
            counts = S.check_conditions(sc)
            assert counts[S.TRIANGULATE_FAILED] >= 3 and (S.reference(sc, "degenerate")[0] == S.TRIANGULATE_FAILED).sum() >= 3
            assert len(sc["idx1"]) >= max(S.PAIR_COUNTS)
