"""Fisheye-stereo frames on the device-resident frame handle through every layer, without a GPU: every new entry point is exported by liborbx.so,
declared in include/orbx.h, registered by the ctypes loader, and named by the Python and the C++ wrappers."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FISHEYE_FRAME_SYMBOLS = ["orbx_frame_load_host_fisheye", "orbx_frame_load_stereo_fisheye_batch", "orbx_frame_counts",
                         "orbx_frame_search_by_projection_mappoints_fisheye", "orbx_frame_search_by_projection_frame_fisheye",
                         "orbx_frame_search_local_points_fisheye"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_fisheye_frame_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in FISHEYE_FRAME_SYMBOLS if s not in exported]


def test_fisheye_frame_symbols_are_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    for s in FISHEYE_FRAME_SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, h), s
    assert "track_depth" in h   # the right-only far-point input of the one-call SearchLocalPoints


def test_fisheye_frame_symbols_are_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    m = (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    for s in FISHEYE_FRAME_SYMBOLS:
        assert s in _lib.SYMBOLS, s
        assert f"L.{s}.argtypes" in src, s
        assert s in m, s
    import orb_slam3_amd as osa
    from orb_slam3_amd.matcher import ORBmatcher
    for name in ("load_fisheye", "load_stereo_fisheye_batch", "counts"):
        assert callable(getattr(osa.DeviceFrame, name))
    assert callable(ORBmatcher.SearchLocalPointsFisheye)


def test_fisheye_frame_symbols_are_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    for s in ("loadFisheye", "loadStereoFisheyeBatch", "SearchLocalPointsFisheye(DeviceFrame &", "SearchByProjectionFisheye(DeviceFrame &"):
        assert s in h, s
    for s in FISHEYE_FRAME_SYMBOLS:
        assert s in h, s


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_fisheye_wrapper_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "int f(ORB_SLAM3::ORBmatcher &m, orbx_extractor *l, orbx_extractor *r) {\n"
                   "    ORB_SLAM3::DeviceFrame F(m, 4000);\n"
                   "    F.loadStereoFisheyeBatch(l, r, 0);\n"
                   "    std::vector<int32_t> match; std::vector<uint8_t> iv;\n"
                   "    ORB_SLAM3::ORBmatcher::LocalMapPoints mps;\n"
                   "    ORB_SLAM3::ORBmatcher::FisheyeMapPoints mp;\n"
                   "    ORB_SLAM3::ORBmatcher::ProjectedQueries q;\n"
                   "    orbx_fisheye_view views[2]{};\n"
                   "    int a = 0, b = 0; F.counts(a, b);\n"
                   "    return m.SearchLocalPointsFisheye(F, {}, views, 0.18f, 0.5f, mps, {}, 1.f, false, 0.f, iv, match) +\n"
                   "           m.SearchByProjectionFisheye(F, {}, mp, 3.f, match) + m.SearchByProjectionFisheye(F, {}, q, {}, 7.f, false, false, match);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
