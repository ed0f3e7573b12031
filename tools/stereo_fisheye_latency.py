"""Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166): per-call latency of the device path against the callback path and the CPU work, and
the batched stage.  Prints one JSON line; every figure comes with a parity check.  Not imported by bench.py.

  single_device_ms     orbx_compute_stereo_fisheye_matches on a TUM-VI-like frame (1500 x 1500 features), median of --reps calls
  single_callback_ms   the adapter path on the same frame: orbx_knn2 on the device, ratio test and bookkeeping in Python, the oracle's
                       orbo_kb8_triangulate_matches as the host triangulation callback (through ctypes)
  cpu_ms               the same work on the CPU: orbo_knn2 once plus orbo_kb8_epipolar_constrain once over the pairs that pass the ratio test
  batch_ms             orbx_stereo_fisheye_batch_device on 64 resident frame pairs, stage + orbx_sync, median of --reps batches

usage: python tools/stereo_fisheye_latency.py [--reps 20]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

f32 = np.float32


def x3d(L, cam1, cam2, xy1, xy2, R12, t12):
    """x3D of KannalaBrandt8::TriangulateMatches in float32, in the order orbo_kb8_triangulate_matches computes it"""
    r1, r2 = np.zeros(3, f32), np.zeros(3, f32)
    L.orbo_kb8_unproject(cam1.ctypes.data_as(C.c_void_p), C.c_float(xy1[0]), C.c_float(xy1[1]), r1.ctypes.data_as(C.c_void_p))
    L.orbo_kb8_unproject(cam2.ctypes.data_as(C.c_void_p), C.c_float(xy2[0]), C.c_float(xy2[1]), r2.ctypes.data_as(C.c_void_p))
    R21 = R12.reshape(3, 3).T.copy()
    T2 = np.zeros((3, 4), f32)
    for i in range(3):
        T2[i, :3] = R21[i]
        T2[i, 3] = ((f32(0) + (-R21[i, 0]) * t12[0]) + (-R21[i, 1]) * t12[1]) + (-R21[i, 2]) * t12[2]
    T1 = np.eye(3, 4, dtype=f32)
    A = np.zeros((4, 4), f32)
    for j in range(4):
        A[0, j] = r1[0] * T1[2, j] - T1[0, j]
        A[1, j] = r1[1] * T1[2, j] - T1[1, j]
        A[2, j] = r2[0] * T2[2, j] - T2[0, j]
        A[3, j] = r2[1] * T2[2, j] - T2[1, j]
    V = np.zeros(16, f32)
    L.orbo_eigen_jacobi_svd4_V(A.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p), None)
    return V[3] / V[15], V[7] / V[15], V[11] / V[15]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    L = ob.lib()
    L.orbo_kb8_unproject.restype = None
    L.orbo_eigen_jacobi_svd4_V.restype = None
    L.orbo_kb8_triangulate_matches.restype = C.c_float
    L.orbo_kb8_triangulate_matches.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_void_p, C.c_void_p, C.c_float, C.c_float]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = {"tool": "stereo_fisheye_latency", "device": torch.cuda.get_device_name(0)}
    sigma2 = (np.array([1.2 ** i for i in range(8)], f32) ** 2).astype(f32)

    # ---- single call, 1500 x 1500 features (TUM-VI-like: 500 / 450 outside the lapping area) ----
    rng = np.random.default_rng(2024)
    kl, dl, kr, dr, ml, mr, rig, _, _ = synth.make_fisheye_stereo_frame(rng, 2900, 1500, 1500, 500, 450)
    cl, cr, R, t = (np.ascontiguousarray(rig[k], f32).ravel() for k in ("cam_left", "cam_right", "R_lr", "t_lr"))

    def tri_value(il, ir, s1, s2):
        return L.orbo_kb8_triangulate_matches(vp(cl), vp(cr), float(kl["x"][il]), float(kl["y"][il]), float(kr["x"][ir]), float(kr["y"][ir]), vp(R), vp(t),
                                              s1, s2)

    def tri_full(il, ir, s1, s2):
        v = f32(tri_value(il, ir, s1, s2))
        return float(v), (x3d(L, cl, cr, (kl["x"][il], kl["y"][il]), (kr["x"][ir], kr["y"][ir]), R, t) if v > 0 else (0.0, 0.0, 0.0))
    want = ob.stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, sigma2, tri_full)
    m = osa.ORBmatcher()
    got = m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, sigma2, rig)
    ok_dev = got[:2] == want[:2] and all(a.tobytes() == b.tobytes() for a, b in zip(got[2:], want[2:]))
    cb = m.compute_stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, sigma2, lambda il, ir, s1, s2: (tri_value(il, ir, s1, s2), (0.0, 0.0, 0.0)))
    ok_cb = cb[:2] == want[:2] and all(a.tobytes() == b.tobytes() for a, b in zip(cb[2:5], want[2:5]))   # (p3d: the timed callback skips it)

    def med(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))
    out["single"] = dict(n_left=len(kl), n_right=len(kr), mono_left=ml, mono_right=mr, n_matches=int(want[0]), desc_matches=int(want[1]),
                         device_ms=round(med(lambda: m.ComputeStereoFishEyeMatches(kl, dl, ml, kr, dr, mr, sigma2, rig)), 4),
                         callback_ms=round(med(lambda: m.compute_stereo_fisheye_matches(kl, dl, ml, kr, dr, mr, sigma2,
                                                                                       lambda il, ir, s1, s2: (tri_value(il, ir, s1, s2), (0.0, 0.0, 0.0)))), 4),
                         parity_device=bool(ok_dev), parity_callback=bool(ok_cb))

    # ---- the CPU work: orbo_knn2 once, orbo_kb8_epipolar_constrain once over the ratio-test survivors ----
    q, tr = np.ascontiguousarray(dl[ml:]), np.ascontiguousarray(dr[mr:])
    idx, dist = np.zeros((len(q), 2), np.int32), np.zeros((len(q), 2), np.int32)
    t0 = time.perf_counter()
    L.orbo_knn2(vp(q), len(q), vp(tr), len(tr), vp(idx), vp(dist))
    t_knn = time.perf_counter() - t0
    keep = np.nonzero((idx[:, 1] >= 0) & (dist[:, 0].astype(np.float32).astype(np.float64) < dist[:, 1].astype(np.float32).astype(np.float64) * 0.7))[0]
    a, b = keep + ml, idx[keep, 0] + mr
    xy1 = np.ascontiguousarray(np.stack([kl["x"][a], kl["y"][a]], 1), f32)
    xy2 = np.ascontiguousarray(np.stack([kr["x"][b], kr["y"][b]], 1), f32)
    s1, s2 = np.ascontiguousarray(sigma2[kl["octave"][a]]), np.ascontiguousarray(sigma2[kr["octave"][b]])
    okv, val = np.zeros(len(a), np.uint8), np.zeros(len(a), f32)
    L.orbo_kb8_epipolar_constrain.restype = None
    t0 = time.perf_counter()
    L.orbo_kb8_epipolar_constrain(vp(cl), vp(cr), len(a), vp(xy1), vp(xy2), vp(R), vp(t), vp(s1), vp(s2), vp(okv), vp(val))
    t_gate = time.perf_counter() - t0
    out["cpu"] = dict(knn2_ms=round(t_knn * 1e3, 4), gate_ms=round(t_gate * 1e3, 4), total_ms=round((t_knn + t_gate) * 1e3, 4), pairs=int(len(a)),
                      parity=bool(len(a) == want[1] and int(okv.sum()) == want[0] and np.array_equal(a[okv == 1], np.nonzero(want[2] >= 0)[0])))

    # ---- batched: 64 frame pairs ----
    cam = np.array(synth.TUMVI_L, f32)
    brig = dict(cam_left=cam, cam_right=cam.copy(), R_lr=np.eye(3, dtype=f32), t_lr=np.array([0.1, 0.0, 0.0], f32))
    out["batch"] = []
    for size, nf in ((512, 1000), (1024, 1500)):
        nb = 64
        canvas = synth.make_canvas(7, size=max(2048, 2 * size + 256))
        pairs = [synth.make_stereo_pair(7, i, size, size, canvas) for i in range(nb)]
        lt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        rt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        exl, exr = osa.ORBextractor(nf, 1.2, 8, 20, 7), osa.ORBextractor(nf, 1.2, 8, 20, 7)
        lap = (size // 3, size - 1)
        exl.extract_batch_device(lt.data_ptr(), nb, size, size, size, size * size, lap)
        exr.extract_batch_device(rt.data_ptr(), nb, size, size, size, size * size, lap)
        exl.sync(); exr.sync()
        sg = exl.GetScaleSigmaSquares().astype(f32)

        def stage():
            exl.stereo_fisheye_batch_device(exr, brig)
            exl.sync()
        ms = med(stage)
        nm, nd, l2r, r2l, depth, p3d = exl.stereo_fisheye_download_all()
        ok = True
        for f in (0, nb // 2, nb - 1):
            mlf, klf, dlf = exl.download(f)
            mrf, krf, drf = exr.download(f)
            s = m.ComputeStereoFishEyeMatches(klf, dlf, mlf, krf, drf, mrf, sg, brig)
            n_l, n_r = len(klf), len(krf)
            ok = ok and s[0] == nm[f] and s[1] == nd[f] and s[2].tobytes() == l2r[f, :n_l].tobytes() and s[3].tobytes() == r2l[f, :n_r].tobytes() \
                and s[4].tobytes() == depth[f, :n_l].tobytes() and s[6].tobytes() == p3d[f, :n_l].tobytes()
        out["batch"].append(dict(size=size, nfeatures=nf, frames=nb, ms=round(ms, 4), n_matches_total=int(nm.sum()), parity_vs_single=bool(ok)))
        del exl, exr
    print(json.dumps(out))


if __name__ == "__main__":
    main()
