"""The colour, resize and CLAHE calls through every layer, without a GPU: the five entry points are exported by liborbx.so, declared in include/orbx.h
with the restated arithmetic beside them, registered by the ctypes loader with as many argument types as the header declares parameters, named by the
Python wrappers and wrapped in C++, where the wrappers compile and link in a translation unit of their own."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_gray_batch_device", "orbx_resize_batch_device", "orbx_clahe_create", "orbx_clahe_destroy", "orbx_clahe_batch_device"]
PY_NAMES = [("ORBextractor", "gray_batch"), ("ORBextractor", "resize_batch"), ("DeviceClahe", "apply_batch"), ("DeviceRectifier", "rectify_batch")]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS + ["orbx_rectify_batch_device", "orbx_extract_batch_device"]:   # the others stay
        assert s in exported, s


def _declaration(h, symbol, ret="int"):
    m = re.search(r"\b%s\s+%s\(([^;]*)\);" % (ret, symbol), h)
    assert m, symbol
    return re.sub(r"\s+", " ", m.group(1))


def test_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert "typedef struct orbx_clahe orbx_clahe;" in h
    tail = "size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst, size_t dst_row_stride, size_t dst_frame_stride"
    assert _declaration(h, SYMBOLS[0]) == "orbx_extractor *ex, const uint8_t *d_src, int n_frames, int width, int height, int channels, int rgb, " + tail
    assert _declaration(h, SYMBOLS[1]) == ("orbx_extractor *ex, const uint8_t *d_src, int n_frames, int src_width, int src_height, size_t src_row_stride, "
                                           "size_t src_frame_stride, uint8_t *d_dst, int dst_width, int dst_height, size_t dst_row_stride, size_t dst_frame_stride")
    assert _declaration(h, SYMBOLS[2]) == "int device, double clip_limit, int tiles_x, int tiles_y, orbx_clahe **out"
    assert _declaration(h, SYMBOLS[3], "void") == "orbx_clahe *c"
    assert _declaration(h, SYMBOLS[4]) == "orbx_clahe *c, orbx_extractor *ex, const uint8_t *d_src, int n_frames, int width, int height, " + tail
    for text in ("Tracking.cc:1569-1582", "needToResize()", "createCLAHE(3.0, cv::Size(8, 8))", "PARITY UNPINNED", "its code wins",
                 "(R * 9798 + G * 19235 + B * 3735 + 16384) >> 15", "(a + b + c + d + 2) >> 2", "saturate_cast<short>((1.f - f) * 2048)",
                 "BORDER_REFLECT_101", "max((int)(clip_limit * area / 256), 1)", "255.0f / area", "step = max(256 / residual, 1)",
                 "for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++", "ties to even", "THEN tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1)",
                 "every operation rounded as written", "[1, 64]", "NEVER IN FLIGHT", "k_gray", "k_resize_half", "k_clahe_lut", "k_clahe_apply"):
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
    assert "DeviceClahe" in osa.__all__ and "DeviceRectifier" in osa.__all__
    for cls, name in PY_NAMES:
        assert callable(getattr(getattr(osa, cls), name)), (cls, name)


def test_argument_counts_match_the_header():
    import ctypes as C
    from orb_slam3_amd import _lib
    h = (ROOT / "include" / "orbx.h").read_text()
    L = _lib.lib()
    for s in SYMBOLS:
        assert len(getattr(L, s).argtypes) == _declaration(h, s, "void" if s.endswith("destroy") else "int").count(",") + 1, s
    assert L.orbx_clahe_destroy.restype is None
    assert L.orbx_clahe_create.argtypes[1] is C.c_double


def test_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBextractor.h").read_text()
    for s in SYMBOLS:
        assert s + "(" in h, s
    for name in ("class Clahe {", "void ApplyBatch(", "void GrayBatch(", "void ResizeBatch(", "class Rectifier {"):
        assert name in h, name


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrappers_compile_and_link(tmp_path):
    """A translation unit of its own that chains the wrappers in the integrator's order links against liborbx.so."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBextractor.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBextractor &ex, const uint8_t *dRaw, uint8_t *dSmall, const uint8_t *dColour, uint8_t *dGray) {\n"
                   "    Clahe clahe(3.0, 8, 8);\n"
                   "    clahe.ApplyBatch(ex, dRaw, 256, 1024, 1024, 1024, 1024 * 1024, const_cast<uint8_t *>(dRaw), 1024, 1024 * 1024);\n"
                   "    ex.ResizeBatch(dRaw, 256, 1024, 1024, 1024, 1024 * 1024, dSmall, 512, 512, 512, 512 * 512);\n"
                   "    ex.GrayBatch(dColour, 256, 752, 480, 3, true, 3 * 752, 3 * 752 * 480, dGray, 752, 752 * 480);\n"
                   "    return clahe.handle() != nullptr;\n"
                   "}\n"
                   "int main(int argc, char **) { return argc > 100 ? (int)(size_t)&f : 0; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", str(src), "-o", str(exe), str(_lib.LIB_PATH),
                        "-Wl,-rpath," + str(_lib.LIB_PATH.parent), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
