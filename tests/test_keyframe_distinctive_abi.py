"""ComputeDistinctiveDescriptors on resident key frames through every layer, without a GPU: the entry point is exported by liborbx.so, declared in
include/orbx.h with the reference lines it replaces and its key-frame limit, registered by the ctypes loader with argument types, and named by the
Python wrapper and the C++ wrapper, which compiles and links in a translation unit of its own.  One oracle-only test asserts what the GPU tests
demand of their inputs."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOL = "orbx_keyframe_distinctive_descriptors"


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbol_is_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert SYMBOL in exported
    assert "orbx_distinctive_descriptors" in exported   # the host-rows call stays


def test_symbol_is_declared_in_the_header():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert re.search(r"\bint\s+%s\(orbx_matcher \*m, int n_kf, orbx_keyframe \*const \*kfs, int n_sets, const int32_t \*set_ptr," % SYMBOL, h)
    limit = re.search(r"#define\s+ORBX_MAX_DISTINCTIVE_KEYFRAMES\s+(\d+)\b", h)
    assert limit and int(limit.group(1)) >= 1024
    # the reference lines the entry point replaces, its callers and its limits are stated where the user reads them
    for text in ("MapPoint.cc:329-403", "MapPoint.cc:345-356", "LocalMapping::ProcessNewKeyFrame", "LocalMapping::SearchInNeighbors",
                 "Tracking::CreateNewKeyFrame", "(int)(0.5 * (N - 1))", "the first minimum wins", "ORBX_E_TOO_LARGE", "N_left"):
        assert text in h, text


def test_symbol_is_bound_in_python():
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    assert SYMBOL in _lib.SYMBOLS
    assert f"L.{SYMBOL}.argtypes" in src
    h = (ROOT / "include" / "orbx.h").read_text()
    assert _lib.MAX_DISTINCTIVE_KEYFRAMES == int(re.search(r"#define\s+ORBX_MAX_DISTINCTIVE_KEYFRAMES\s+(\d+)", h).group(1))
    assert SYMBOL in (ROOT / "orb_slam3_amd" / "matcher.py").read_text()
    import orb_slam3_amd as osa
    assert callable(osa.ORBmatcher.DistinctiveDescriptorsKeyFrames)


def test_symbol_is_wrapped_in_cpp():
    h = (ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h").read_text()
    assert SYMBOL in h
    assert re.search(r"void ComputeDistinctiveDescriptors\(const std::vector<DeviceKeyFrame \*> &vpKFs, const std::vector<int32_t> &setPtr, "
                     r"const std::vector<int32_t> &obsKf,\s+const std::vector<int32_t> &obsIdx, std::vector<int32_t> &bestObs, "
                     r"std::vector<uint8_t> \*bestDesc = nullptr\)", h)
    # the host-rows overload is still there
    assert "void ComputeDistinctiveDescriptors(const std::vector<uint8_t> &descriptors, const std::vector<int32_t> &setPtr, std::vector<int32_t> &bestIdx)" in h


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles_and_links(tmp_path):
    """A translation unit of its own that calls the new overload (and the old one beside it) links against liborbx.so; tests/cpp/adapter_demo.cpp
    builds as before."""
    from orb_slam3_amd import _lib
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int f(ORBmatcher &m, const FrameView &V) {\n"
                   "    DeviceKeyFrame a(m, V, nullptr), b(m, V, nullptr);\n"
                   "    std::vector<DeviceKeyFrame *> kfs{&a, &b};\n"
                   "    std::vector<int32_t> setPtr{0, 2, 2}, obsKf{0, 1}, obsIdx{0, 0}, bestObs, bestIdx;\n"
                   "    std::vector<uint8_t> bestDesc, rows(64);\n"
                   "    m.ComputeDistinctiveDescriptors(kfs, setPtr, obsKf, obsIdx, bestObs, &bestDesc);\n"
                   "    m.ComputeDistinctiveDescriptors(kfs, setPtr, obsKf, obsIdx, bestObs);\n"
                   "    m.ComputeDistinctiveDescriptors(rows, setPtr, bestIdx);\n"
                   "    return bestObs[0] + bestIdx[0] + bestDesc[0];\n"
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


def test_set_conditions_hold_for_the_oracle_alone(oracle):
    """What tests/test_gpu_keyframe_distinctive.py demands of the sets of its first test, asserted on the oracle (no device code runs): the key frames
    have unequal N and hold every observation's row, the boundary sizes are all there, every median index (int)(0.5 * (N - 1)) of N = 1..5 occurs,
    and the winners are not all row 0 -- at least a quarter of the sets of three or more rows pick another row."""
    import orb_slam3_amd as osa
    assert hasattr(osa.ORBmatcher, "DistinctiveDescriptorsKeyFrames")   # (these are its inputs)
    import distinctive_sets as DS
    S = DS.boundary_sets()
    sizes = np.array(S["sizes"])
    assert set(DS.EDGE_SIZES) <= set(S["sizes"]) and len(sizes) == len(DS.EDGE_SIZES) + DS.N_RANDOM
    assert {1, 2, 3, 4, 5} <= set(S["sizes"])
    assert {int(0.5 * (n - 1)) for n in (1, 2, 3, 4, 5)} == {0, 1, 2}
    assert len({len(d) for d in S["kf_desc"]}) == 3 and sum(len(d) for d in S["kf_desc"]) == S["set_ptr"][-1]
    assert np.array_equal(DS.gather(S["kf_desc"], S["obs_kf"], S["obs_idx"]), S["rows"])
    assert all(len(np.unique(S["obs_kf"][b:e])) == 3 for b, e in zip(S["set_ptr"][:-1], S["set_ptr"][1:]) if e - b >= 40)   # spread over the three
    want = oracle.distinctive_descriptors(S["rows"], S["set_ptr"])
    assert want[0] == -1 and (want[sizes > 0] >= 0).all() and (want[sizes > 0] < sizes[sizes > 0]).all()
    nontrivial = sizes >= 3
    assert (want[nontrivial] != 0).sum() * 4 >= nontrivial.sum(), ((want[nontrivial] != 0).sum(), nontrivial.sum())
    for n in (64, 65, 128, 129, 300):
        assert want[S["sizes"].index(n)] != 0, n   # the boundary sets themselves tell the first row from the winner
