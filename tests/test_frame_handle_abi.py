"""The device-resident frame handle (orbx_frame) through every layer, without a GPU: every entry point is exported by liborbx.so, declared
in include/orbx.h, registered by the ctypes loader, and named by the Python and the C++ wrappers."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FRAME_SYMBOLS = ["orbx_frame_create", "orbx_frame_destroy", "orbx_frame_load_host", "orbx_frame_load_batch", "orbx_frame_count",
                 "orbx_frame_search_by_projection_mappoints", "orbx_frame_search_by_projection_frame", "orbx_frame_search_local_points"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_frame_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in FRAME_SYMBOLS if s not in exported]


def test_frame_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert "typedef struct orbx_frame orbx_frame;" in h
    for s in FRAME_SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\(" % s, h), s


def test_frame_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    for s in FRAME_SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in ("orbx_frame_create", "orbx_frame_destroy", "orbx_frame_load_host", "orbx_frame_load_batch", "orbx_frame_count",
              "orbx_frame_search_by_projection_mappoints", "orbx_frame_search_by_projection_frame", "orbx_frame_search_local_points"):
        assert s in m, s
    import orb_slam3_amd as osa
    from orb_slam3_amd.matcher import ORBmatcher
    for name in ("load", "load_batch", "count"):
        assert callable(getattr(osa.DeviceFrame, name))
    assert callable(ORBmatcher.SearchLocalPoints)


def test_frame_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    assert "class DeviceFrame" in h and "SearchLocalPoints(DeviceFrame &" in h
    for s in FRAME_SYMBOLS:
        assert s in h, s


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "int f(ORB_SLAM3::ORBmatcher &m, orbx_extractor *ex) {\n"
                   "    ORB_SLAM3::DeviceFrame F(m, 2000);\n"
                   "    F.loadBatch(ex, 0);\n"
                   "    std::vector<int32_t> match; std::vector<uint8_t> iv;\n"
                   "    ORB_SLAM3::ORBmatcher::LocalMapPoints mps;\n"
                   "    orbx_camera cam{}; orbx_frame_pose pose{};\n"
                   "    return m.SearchLocalPoints(F, {}, cam, pose, 0.18f, 0.5f, mps, 1.f, false, 0.f, iv, match) + F.count();\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
