"""The image-preparation calls through every layer, without a GPU: the four entry points are exported by liborbx.so, declared in include/orbx.h with the
restated arithmetic beside them, registered by the ctypes loader with as many argument types as the header declares parameters, named by the Python
wrappers and wrapped in C++, where the wrappers compile and link in a translation unit of their own.  One reference-only test asserts what
tests/test_gpu_image_prep.py demands of its designed maps."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_rectifier_create", "orbx_rectifier_destroy", "orbx_rectify_batch_device", "orbx_rgbd_batch_device_u16"]
PY_NAMES = [("DeviceRectifier", "rectify_batch"), ("ORBextractor", "rgbd_batch_u16"), ("ORBextractor", "RGBDBatch")]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + ["orbx_rgbd_batch_device", "orbx_extract_batch_device"]:   # the others stay
        assert s in exported, s


def _declaration(h, symbol, ret="int"):
    m = re.search(r"\b%s\s+%s\(([^;]*)\);" % (ret, symbol), h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert "typedef struct orbx_rectifier orbx_rectifier;" in h
    assert _declaration(h, SYMBOLS[0]) == ("int device, const float *map_x, const float *map_y, int dst_width, int dst_height, size_t map_stride, "
                                           "orbx_rectifier **out")
    assert _declaration(h, SYMBOLS[1], "void") == "orbx_rectifier *r"
    assert _declaration(h, SYMBOLS[2]) == ("orbx_rectifier *r, orbx_extractor *ex, const uint8_t *d_src, int n_frames, int src_width, int src_height, "
                                           "size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst, size_t dst_row_stride, size_t dst_frame_stride")
    assert _declaration(h, SYMBOLS[3]) == ("orbx_extractor *ex, const uint16_t *d_depth, size_t pitch_bytes, size_t frame_stride_bytes, "
                                           "float depth_factor, float bf")
    assert _declaration(h, "orbx_rgbd_batch_device") == "orbx_extractor *ex, const float *d_depth, size_t pitch_bytes, size_t frame_stride_bytes, float bf"
    for text in ("System.cc:259-260", "imgwarp.cpp", "PARITY UNPINNED", "cvRound(map_x[y][x] * 32)", "ties to even", "INT_MIN", "saturate_cast<short>(sx >> 5)",
                 "(32 - a)(32 - b) * 32", "+ 16384) >> 15", "((32767 p + q + 16384) >> 15) == p", "a tap outside is 0", "BORDER_CONSTANT", "[1, 32766]",
                 "k_rectify", "k_stereo_from_rgbd_u16", "mDepthMapFactor", "one rounded float"):
        assert text in h, text


def test_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    py = (ROOT / "orb_slam3_amd" / "extractor.py").read_text()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert s in py, s
    import orb_slam3_amd as osa
    assert "DeviceRectifier" in osa.__all__
    for cls, name in PY_NAMES:
        assert callable(getattr(getattr(osa, cls), name)), (cls, name)


def test_argument_counts_match_the_header():
    from orb_slam3_amd import _lib
    h = (ROOT / "include" / "orbx.h").read_text()
    L = _lib.lib()
    for s in SYMBOLS:
        assert len(getattr(L, s).argtypes) == _declaration(h, s, "void" if s.endswith("destroy") else "int").count(",") + 1, s
    assert L.orbx_rectifier_destroy.restype is None


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBextractor.h").read_text()
    for s in SYMBOLS:
        assert s + "(" in h, s
    for name in ("class Rectifier {", "void RectifyBatch(", "void RGBDBatchU16(", "void RGBDBatch("):
        assert name in h, name


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that calls the wrappers links against liborbx.so."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBextractor.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBextractor &left, ORBextractor &right, const float *M1, const float *M2, const uint8_t *dRaw, uint8_t *dRect, const uint16_t *dDepth) {\n"
                   "    Rectifier rect(M1, M2, 752, 480, 752);\n"
                   "    rect.RectifyBatch(left, dRaw, 256, 752, 480, 752, 752 * 480, dRect, 752, 752 * 480);\n"
                   "    rect.RectifyBatch(right, dRaw, 256, 752, 480, 752, 752 * 480, dRect + 256 * 752 * 480, 752, 752 * 480);\n"
                   "    left.RGBDBatchU16(dDepth, 1280, 1280 * 480, 1.0f / 5000.0f, 40.f);\n"
                   "    return rect.width() + rect.height() + (rect.handle() != nullptr);\n"
                   "}\n"
                   "int main(int argc, char **) { return argc > 100 ? (int)(size_t)&f : 0; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", str(src), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()


def test_map_conditions_hold_for_the_reference_alone():
    """What tests/test_gpu_image_prep.py demands of its designed maps, asserted on the integer reference (no device code runs): each plausible wrong
    implementation differs from the reference on the class made for it, and the 16-bit depth values tell one rounding from a double division."""
    import image_prep_scene as S
    counts = S.check_conditions()
    assert counts["half_up"] > 400 and counts["float_bilinear"] > 400 and counts["nan_as_zero"] > 0, counts
    assert counts["clamp_below_zero"] > 400 and counts["clamp_at_the_far_edge"] > 400, counts
    assert S.check_conditions_depth() >= 1
