"""The fisheye stereo entry points (orbx_compute_stereo_fisheye_matches, orbx_stereo_fisheye_batch_*) through every layer, without a GPU: exported,
declared, bound by the ctypes loader with the C layout of orbx_kb8_rig, argument checks that refuse before any device work, and the C++ overload."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["orbx_compute_stereo_fisheye_matches", "orbx_stereo_fisheye_batch_device", "orbx_stereo_fisheye_batch_download",
           "orbx_stereo_fisheye_batch_download_all"]
BAD_ARG = -2


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm not installed")
def test_symbols_are_exported():
    lib = ROOT / "orb_slam3_amd" / "liborbx.so"
    assert lib.exists(), "build liborbx.so first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in SYMBOLS if s not in exported]


def test_symbols_are_declared_and_bound():
    h = (ROOT / "include" / "orbx.h").read_text()
    assert "typedef struct orbx_kb8_rig {" in h and "UNPINNED" in h
    from orb_slam3_amd import _lib
    src = (ROOT / "orb_slam3_amd" / "_lib.py").read_text()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, h), s
        assert s in _lib.SYMBOLS and f"L.{s}.argtypes" in src, s


def test_rig_layout():
    from orb_slam3_amd import _lib
    R = _lib.Kb8Rig
    assert C.sizeof(R) == 28 * 4
    assert (R.cam_left.offset, R.cam_right.offset, R.R_lr.offset, R.t_lr.offset) == (0, 32, 64, 100)
    r = R.make(dict(cam_left=np.arange(8), cam_right=np.arange(8) + 8, R_lr=np.arange(9).reshape(3, 3) + 16, t_lr=np.arange(3) + 25))
    assert np.array_equal(np.frombuffer(bytes(r), np.float32), np.arange(28, dtype=np.float32))
    with pytest.raises(ValueError):
        R.make(dict(cam_left=np.zeros(7), cam_right=np.zeros(8), R_lr=np.zeros(9), t_lr=np.zeros(3)))


def test_bad_arguments_are_refused_before_device_work():
    """Every check runs on the host before the matcher is touched: a stand-in handle (never dereferenced) is enough."""
    from orb_slam3_amd import _lib
    from orb_slam3_amd._lib import KP_DTYPE, ptr
    L = _lib.lib()
    fake = C.create_string_buffer(4096)
    m = C.cast(fake, C.c_void_p)
    rig = _lib.Kb8Rig()
    nl, nr = 10, 12
    kl, kr = np.zeros(nl, KP_DTYPE), np.zeros(nr, KP_DTYPE)
    dl, dr = np.zeros((nl, 32), np.uint8), np.zeros((nr, 32), np.uint8)
    s2 = np.ones(8, np.float32)
    l2r, r2l, depth, p3d = np.zeros(nl, np.int32), np.zeros(nr, np.int32), np.zeros(nl, np.float32), np.zeros((nl, 3), np.float32)

    def call(m=m, rig=C.byref(rig), kl=ptr(kl), dl=ptr(dl), nl=nl, ml=2, kr=ptr(kr), dr=ptr(dr), nr=nr, mr=3, s2=ptr(s2), nlev=8, l2r=ptr(l2r),
             r2l=ptr(r2l), depth=ptr(depth), p3d=ptr(p3d)):
        return L.orbx_compute_stereo_fisheye_matches(m, rig, kl, dl, nl, ml, kr, dr, nr, mr, s2, nlev, l2r, r2l, depth, p3d, None)
    assert call(m=None) == BAD_ARG
    assert call(rig=None) == BAD_ARG
    for ml, mr in ((-1, 0), (nl + 1, 0), (0, -1), (0, nr + 1)):
        assert call(ml=ml, mr=mr) == BAD_ARG, (ml, mr)
    for k in ("kl", "dl", "kr", "dr", "s2", "l2r", "r2l", "depth", "p3d"):
        assert call(**{k: None}) == BAD_ARG, k
    assert call(nlev=0) == BAD_ARG
    kl["octave"][4] = 8
    assert call() == BAD_ARG
    kl["octave"][4] = -1
    assert call() == BAD_ARG
    kl["octave"][4] = 0
    kr["octave"][nr - 1] = 9
    assert call() == BAD_ARG
    assert L.orbx_stereo_fisheye_batch_device(None, None, C.byref(rig)) == BAD_ARG
    assert L.orbx_stereo_fisheye_batch_download(None, 0, *[None] * 8) == BAD_ARG
    assert L.orbx_stereo_fisheye_batch_download_all(None, *[None] * 6) == BAD_ARG


def test_python_and_cpp_surfaces():
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    assert callable(osa.ORBmatcher.ComputeStereoFishEyeMatches)
    for name in ("stereo_fisheye_batch_device", "stereo_fisheye_download", "stereo_fisheye_download_all"):
        assert callable(getattr(osa.ORBextractor, name)), name
    kl, dl, kr, dr, ml, mr, rig, idl, idr = synth.make_fisheye_stereo_frame(np.random.default_rng(3), 900, 500, 480, 200, 150)
    assert (len(kl), len(kr), ml, mr) == (500, 480, 200, 150) and dl.shape == (500, 32) and dr.shape == (480, 32)
    assert np.isin(idl[ml:], idr[mr:]).mean() > 0.9   # the lapping tails hold true correspondences
    assert set(rig) == {"cam_left", "cam_right", "R_lr", "t_lr"} and rig["R_lr"].shape == (3, 3)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_cpp_wrapper_compiles(tmp_path):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(ROOT / "orb_slam3_amd" / "cpp" / "ORBmatcher.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    src = tmp_path / "t.cpp"
    src.write_text('#include "orb_slam3_amd/cpp/ORBmatcher.h"\n'
                   "int f(ORB_SLAM3::ORBmatcher &m, const orbx_keypoint *k, const uint8_t *d, const float *s, orbx_kb8_rig rig) {\n"
                   "    std::vector<int> l2r, r2l; std::vector<float> depth, ur; std::vector<std::array<float, 3>> p3d; int nd = 0;\n"
                   "    return m.ComputeStereoFishEyeMatches(k, d, 10, 2, k, d, 10, 3, s, 8, rig, l2r, r2l, depth, ur, p3d, &nd);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
