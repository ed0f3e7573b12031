"""Rectified-stereo / RGB-D depth on resident frames and key frames through every layer, without a GPU: the seven entry points are exported by
liborbx.so, declared in include/orbx.h, registered by the ctypes loader with as many argument types as the header declares parameters, named by the
Python wrappers and wrapped in C++, where the wrappers compile and link in a translation unit of their own; status 12 is the header's in every
layer.  One reference-only test asserts what tests/test_gpu_stereo_resident.py demands of its key-frame scenes, for every seed it uses."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_rgbd_batch_device", "orbx_frame_load_stereo_batch", "orbx_frame_load_host_stereo", "orbx_frame_unproject_stereo",
           "orbx_keyframe_create_host_stereo", "orbx_keyframe_triangulate_pairs_stereo", "orbx_keyframe_search_and_triangulate_stereo"]
PY_NAMES = [("ORBextractor", "RGBDBatch"), ("DeviceFrame", "load_stereo_batch"), ("DeviceFrame", "load_host_stereo"), ("ORBmatcher", "UnprojectStereo"),
            ("DeviceKeyFrame", "create_host_stereo"), ("ORBmatcher", "TriangulatePairsKeyFramesStereo"), ("ORBmatcher", "SearchAndTriangulateResidentStereo")]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + ["orbx_stereo_batch_device", "orbx_frame_load_batch", "orbx_keyframe_triangulate_pairs"]:   # the others stay
        assert s in exported, s


def _declaration(h, symbol):
    m = re.search(r"\bint\s+%s\(([^;]*)\);" % symbol, h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert _declaration(h, SYMBOLS[0]) == "orbx_extractor *ex, const float *d_depth, size_t pitch_bytes, size_t frame_stride_bytes, float bf"
    assert _declaration(h, SYMBOLS[1]) == "orbx_frame *f, orbx_extractor *left, int frame, const float *bounds4, const float *scale_factors, int nlevels"
    assert _declaration(h, SYMBOLS[2]) == "orbx_frame *f, const orbx_frame_desc *desc, const float *depth, const float *keys_xy"
    assert _declaration(h, SYMBOLS[3]) == ("orbx_matcher *m, orbx_frame *f, const orbx_new_points_view *view, float *u_right, float *depth, float *pos, "
                                           "int *n_with_depth")
    assert _declaration(h, SYMBOLS[4]) == ("orbx_matcher *m, const orbx_frame_desc *desc, const float *depth, const float *keys_xy, "
                                           "const float *inv_level_sigma2, orbx_keyframe **out")
    # the `_stereo` forms: every argument of the existing forms, `st` placed after `par`
    for plain, stereo in ((("orbx_keyframe_triangulate_pairs"), SYMBOLS[5]), ("orbx_keyframe_search_and_triangulate", SYMBOLS[6])):
        want = _declaration(h, plain).replace("const orbx_new_points_params *par, ", "const orbx_new_points_params *par, const orbx_new_points_stereo *st, ")
        assert _declaration(h, stereo) == want, stereo
    assert _declaration(h, "orbx_frame_load_batch") == _declaration(h, SYMBOLS[1]).replace("*left", "*ex")     # the existing load keeps its declaration
    assert re.search(r"typedef struct orbx_new_points_stereo \{ float mb1, mbf1, mb2, mbf2; \} orbx_new_points_stereo;", h)
    for text in ("Frame::ComputeStereoFromRGBD", "converted to int by truncation", "a NaN depth therefore gives -1", "Frame::UnprojectStereo",
                 "KeyFrame::UnprojectStereo", "the RAW key point", "cos(2 * atan2(KF1.mb / 2, KF1.mvDepth[idx1]))", "7.8 * mvLevelSigma2_1[kp1.octave]",
                 "no reference tree compiles LocalMapping.cc", "ORBX_NEWPT_UNPROJECT_FAILED", "k_stereo_from_rgbd", "k_unproject_stereo", "k_new_points_stereo"):
        assert text in h, text


def test_status_12_is_the_headers_in_every_layer():
    h = (ROOT / "include" / "orbx.h").read_text()
    from orb_slam3_amd import _lib
    import stereo_resident_scene as S
    m = re.search(r"#define ORBX_NEWPT_UNPROJECT_FAILED (\d+)", h)
    assert m and int(m.group(1)) == 12
    assert _lib.NEWPT_UNPROJECT_FAILED == 12 and _lib.NEWPT_STATUS_STEREO[12] == "UNPROJECT_FAILED" and _lib.NEWPT_STATUS_STEREO[:12] == _lib.NEWPT_STATUS
    assert S.UNPROJECT_FAILED == 12 and S.STATUS[12] == "UNPROJECT_FAILED" and S.STATUS[:12] == tuple(_lib.NEWPT_STATUS)
    cpp = (ROOT / "tests" / "cpp" / "stereo_resident_check.cpp").read_text()
    assert "ORBX_NEWPT_UNPROJECT_FAILED" in cpp and "int hist[13]" in cpp          # (the C++ layer takes the value from the header)
    # the values of the existing forms are the ones they were
    assert [int(v) for v in re.findall(r"\bORBX_NEWPT_[A-Z_0-9]+ = (\d+)", h)] == list(range(12))


def test_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    py = (ROOT / "orb_slam3_amd" / "matcher.py").read_text() + (ROOT / "orb_slam3_amd" / "extractor.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert s in py, s
    import orb_slam3_amd as osa
    for cls, name in PY_NAMES:
        assert callable(getattr(getattr(osa, cls), name)), (cls, name)


def test_argument_counts_and_struct_sizes_match_the_header():
    import ctypes as C
    from orb_slam3_amd import _lib
    h = (ROOT / "include" / "orbx.h").read_text()
    L = _lib.lib()
    for s in SYMBOLS:
        assert len(getattr(L, s).argtypes) == _declaration(h, s).count(",") + 1, s
    assert C.sizeof(_lib.NewPointsStereo) == 16 and [f[0] for f in _lib.NewPointsStereo._fields_] == ["mb1", "mbf1", "mb2", "mbf2"]


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text() + (ROOT / "orb_slam3_amd" / "cpp" / "ORBextractor.h").read_text()
    for s in SYMBOLS:
        assert s + "(" in h, s
    for name in ("void RGBDBatch(", "void loadStereoBatch(", "void loadHostStereo(", "int UnprojectStereo(", "int TriangulatePairsStereo(",
                 "int SearchAndTriangulateStereo("):
        assert name in h, name


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that calls the seven wrappers links against liborbx.so."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBextractor.h"\n'
                   '#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBextractor &ex, ORBmatcher &m, const FrameView &V, const float *dDepth) {\n"
                   "    ex.RGBDBatch(dDepth, 1280, 1280 * 240, 40.f);\n"
                   "    DeviceFrame F(m, 2000);\n"
                   "    F.loadStereoBatch(ex.handle(), 0);\n"
                   "    std::vector<float> depth, xy, ur, x3D;\n"
                   "    F.loadHostStereo(V, depth, xy);\n"
                   "    orbx_new_points_view v1{}, v2{};\n"
                   "    int acc = m.UnprojectStereo(F, v1, ur, depth, x3D);\n"
                   "    DeviceKeyFrame a(m, V, depth, xy, nullptr), b(m, F, nullptr);\n"
                   "    float sigma[8] = {1, 1, 1, 1, 1, 1, 1, 1};\n"
                   "    orbx_new_points_params par{1.8f, 0, 0, 0.f, 8, 8, sigma, sigma};\n"
                   "    orbx_new_points_stereo st{0.11f, 55.f, 0.11f, 55.f};\n"
                   "    orbx_keyframe_gate g{};\n"
                   "    std::vector<int32_t> i1{0, 1}, i2{1, -1};\n"
                   "    std::vector<float> pos;\n"
                   "    std::vector<uint8_t> status, none;\n"
                   "    std::vector<std::pair<size_t, size_t>> pairs;\n"
                   "    acc += m.TriangulatePairsStereo(a, b, v1, v2, par, st, i1, i2, pos, status);\n"
                   "    int nacc = 0;\n"
                   "    acc += m.SearchAndTriangulateStereo(a, b, none, none, g, v1, v2, par, st, pairs, pos, status, nacc);\n"
                   "    return acc + nacc + (status[0] == ORBX_NEWPT_UNPROJECT_FAILED);\n"
                   "}\n"
                   "int main(int argc, char **) { return argc > 100 ? (int)(size_t)&f : 0; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", str(src), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()


def test_scene_conditions_hold_for_the_reference_alone():
    """What tests/test_gpu_stereo_resident.py demands of its key-frame scenes, asserted on the float32 reference (no device code runs), for every
    seed: the designed classes (a) .. (h) with their counts (stereo_resident_scene.check_conditions_stereo), and for class (e) -- a stereo
    observation with cosParallaxRays <= 0 -- that both verdicts occur over the seeds: left as low parallax, and unprojected."""
    import new_points_scene as N
    import stereo_resident_scene as S
    verdicts = set()
    for seed in N.SEEDS:
        sc = S.make_stereo_scene(seed)
        verdicts |= S.check_conditions_stereo(sc)
        assert len(sc["idx1"]) >= max(S.PAIR_COUNTS)
    assert N.LOW_PARALLAX in verdicts and len(verdicts - {N.LOW_PARALLAX}) >= 1, verdicts
