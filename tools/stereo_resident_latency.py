#!/usr/bin/env python3
"""Latency of the rectified-stereo / RGB-D depth path on resident frames and key frames (not imported by bench.py).  Three measurements:
  resident   making one 1000-feature rectified frame resident, its extraction and stereo stage done:
             (a) host   orbx_stereo_batch_download + orbx_batch_download + orbx_frame_load_host with u_right, closed by orbx_frame_count (the
                        parent's route, this build's existing entry points)
             (b) device orbx_frame_load_stereo_batch + orbx_frame_count
             with the bytes that cross the link in each route; `device_below_host_min`: (b)'s median lies below (a)'s min
  rgbd       k_stereo_from_rgbd for a batch of 256 frames of 640 x 480, kernel-only, from one serialized rocprofv3 --kernel-trace --stats run of a
             child (no counters), against the member as a C++ host loop over the downloaded key points on one core (stereo_resident_host_loop.cpp)
  fused      orbx_keyframe_search_and_triangulate_stereo on two 1000-feature stereo key frames against the plain fused call of this build on the same
             key frames (which leaves the stereo pairs undecided: `plain_undecided`); `stereo_within_spread`: the new median is not above the plain
             one's by more than the plain one's own max - min
40 timed repetitions, the forms alternating, every output checked in every repetition; median (min - max) in microseconds, host clock around calls
that end in a stream synchronisation.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

f32 = np.float32
RGBD_SHAPE = (256, 640, 480)   # frames, width, height


def stats(res, key, a):
    a = np.array(a)
    res[f"{key}_med_us"], res[f"{key}_min_us"], res[f"{key}_max_us"] = round(float(np.median(a)), 1), round(float(a.min()), 1), round(float(a.max()), 1)


def resident(res, reps, warmup):
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    w, h = 752, 480
    canvas = synth.make_canvas(30, size=2048, n_shapes=2400)
    left, right = synth.make_stereo_pair(30, 0, w, h, canvas)
    dl, dr = torch.from_numpy(left[None].copy()).cuda(), torch.from_numpy(right[None].copy()).cuda()
    exl, exr = osa.ORBextractor(1000, 1.2, 8, 20, 7), osa.ORBextractor(1000, 1.2, 8, 20, 7)
    exl.extract_batch_device(dl.data_ptr(), 1, w, h, w, w * h, (0, 0))
    exr.extract_batch_device(dr.data_ptr(), 1, w, h, w, w * h, (0, 0))
    exl.stereo_batch_device(exr, 0.11 * 458.654, 0.11)
    exl.sync()
    nm0, ur0, depth0 = exl.stereo_download(0)
    _, k0, d0 = exl.download(0)
    n, cap = len(k0), exl.batch_view().cap
    sf = exl.GetScaleFactors().astype(f32)
    m = osa.ORBmatcher(0.9, True)
    A, B = osa.DeviceFrame(m, cap), osa.DeviceFrame(m, cap)
    view = (np.eye(3, dtype=f32), np.zeros(3, f32), np.zeros(3, f32), 458.654, 457.296, 367.215, 248.375)
    rng = np.random.default_rng(3)
    src = rng.integers(0, n, 400)
    mp = dict(proj_x=k0["x"][src] + 1.0, proj_y=k0["y"][src] - 1.0, proj_xr=np.where(ur0[src] >= 0, ur0[src] + 1.0, 0).astype(f32),
              level=k0["octave"][src].astype(np.int32), view_cos=np.full(400, 0.9, f32), desc=d0[src], in_view=np.ones(400, np.uint8),
              has_obs=np.ones(400, np.uint8))

    def host():
        nm, ur, _ = exl.stereo_download(0)
        _, k, d = exl.download(0)
        A.load(osa.FrameView(k, d, 0.0, float(w), 0.0, float(h), sf, ur))
        return A, A.count(), ur

    def device():
        B.load_stereo_batch(exl, 0)
        return B, B.count(), None

    want = None
    times = {"host": [], "device": []}
    for rep in range(warmup + reps):
        for name, fn in (("host", host), ("device", device)):
            t0 = time.perf_counter()
            D, count, ur = fn()
            dt = time.perf_counter() - t0
            row = m.SearchByProjection(D, mp, 3.0)                # outside the clock: the handle holds the frame, mvuRight included
            want = row if want is None else want
            assert count == n and row[0] == want[0] and np.array_equal(row[1], want[1]) and (ur is None or np.array_equal(ur, ur0)), (name, rep)
            if name == "device":
                got = m.UnprojectStereo(D, view)
                assert got[0] == nm0 and np.array_equal(got[1], ur0) and np.array_equal(got[2], depth0), rep
            if rep >= warmup:
                times[name].append(dt * 1e6)
    for name, a in times.items():
        stats(res, f"resident_{name}", a)
    A.load(osa.FrameView(k0, d0, 0.0, float(w), 0.0, float(h), sf, ur0))
    res["resident_features"], res["resident_stereo_matches"], res["resident_want_matches"] = n, int(nm0), int(want[0])
    # (a): mvuRight, mvDepth (4 + 4 bytes), key point and descriptor (28 + 32) per feature and two counts come down; the loader's own counter says what goes up
    res["resident_host_download_bytes"], res["resident_host_upload_bytes"] = 68 * n + 12, int(m.last_transfers()["upload_bytes"])
    res["resident_device_download_bytes"], res["resident_device_upload_bytes"] = 4, 0    # (b): the count
    res["resident_device_below_host_min"] = bool(res["resident_device_med_us"] < res["resident_host_min_us"])


def rgbd_setup():
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    B, w, h = RGBD_SHAPE
    canvas = synth.make_canvas(7, size=2048, n_shapes=2400)
    frames = np.stack([synth.frame_from_canvas(canvas, t, w, h, 900 + t) for t in range(B)])
    d_frames = torch.from_numpy(frames).cuda()
    x, y = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    img = (0.5 + 0.01 * x + 0.003 * y).astype(f32)
    img[:, 100:140] = 0.0
    depth = np.ascontiguousarray(np.broadcast_to(img, (B, h, w)))
    d_depth = torch.from_numpy(depth).cuda()
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    ex.set_camera((517.3, 516.5, 318.6, 255.3, 0.2624, -0.9531, -0.0054, 0.0026, 1.1633, 40.0))   # TUM fr1
    ex.extract_batch_device(d_frames.data_ptr(), B, w, h, w, w * h, (0, 0))
    return ex, depth, d_depth, (d_frames,)


def rgbd_child(reps):
    ex, depth, d_depth, keep = rgbd_setup()
    _, w, h = RGBD_SHAPE
    for _ in range(reps):
        ex.RGBDBatch(d_depth.data_ptr(), 4 * w, 4 * w * h, 40.0)
    ex.sync()
    ex.stereo_download(0)
    del keep


def rgbd(res, out_dir):
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 is not installed")
    d = Path(out_dir) / "kt"
    shutil.rmtree(d, ignore_errors=True)
    r = subprocess.run([exe, "--kernel-trace", "--stats", "-d", str(d), "-o", "kt", "--", sys.executable, str(Path(__file__).resolve()), "--rgbd-child",
                        "--reps", "20"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the traced child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    dbs = sorted(d.rglob("*.db"), key=lambda p: p.stat().st_size)
    if not dbs:
        raise RuntimeError("rocprofv3 wrote no .db")
    for name, calls, total, avg in sqlite3.connect(str(dbs[-1])).execute("select name, total_calls, total_duration, average from top_kernels"):
        if "k_stereo_from_rgbd" in name:
            res["rgbd_kernel_calls"], res["rgbd_kernel_avg_us"] = int(calls), round(float(avg), 2)   # (the view's durations are microseconds)
    shutil.rmtree(d, ignore_errors=True)
    # the member as a host loop over the downloaded key points, one core; its results must be the device's
    ex, depth, d_depth, keep = rgbd_setup()
    B, w, h = RGBD_SHAPE
    ex.RGBDBatch(d_depth.data_ptr(), 4 * w, 4 * w * h, 40.0)
    cap = ex.batch_view().cap
    kps, _, counts, _ = ex.download_all()
    kun = np.zeros((B, cap), osa.KP_DTYPE)
    for f in range(B):
        k = ex.download_keypoints_un(f)
        kun[f, :len(k)] = k
    ur_d, dep_d, nm = np.zeros((B, cap), f32), np.zeros((B, cap), f32), np.zeros(B, np.int32)
    ex.stereo_download_all(ur_d.ctypes.data, dep_d.ctypes.data, nm.ctypes.data)
    with tempfile.TemporaryDirectory() as td:
        so = Path(td) / "host_loop.so"
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", str(so), str(Path(__file__).with_name("stereo_resident_host_loop.cpp"))], check=True)
        L = C.CDLL(str(so))
        L.rgbd_host_loop.restype = C.c_double
        L.rgbd_host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_int]
        kps = np.ascontiguousarray(kps).reshape(B, cap)
        ur_h, dep_h = np.zeros((B, cap), f32), np.zeros((B, cap), f32)
        us = L.rgbd_host_loop(_lib.ptr(kps), _lib.ptr(kun), _lib.ptr(counts), cap, B, _lib.ptr(depth), 4 * w, 4 * w * h, 40.0, _lib.ptr(ur_h), _lib.ptr(dep_h), 10)
    for f in range(B):
        n = counts[f]
        assert np.array_equal(ur_h[f, :n].view(np.uint32), ur_d[f, :n].view(np.uint32)) and np.array_equal(dep_h[f, :n].view(np.uint32), dep_d[f, :n].view(np.uint32)), f
        assert nm[f] == (dep_h[f, :n] > 0).sum()
    res["rgbd_frames"], res["rgbd_features"], res["rgbd_with_depth"], res["rgbd_host_loop_us"] = B, int(counts.sum()), int(nm.sum()), round(float(us), 1)
    del keep


def fused(res, reps, warmup):
    import orb_slam3_amd as osa
    import new_points_scene as N
    import stereo_resident_scene as S
    from oracle import oracle_binding as ob
    from test_gpu_frame_bow import SF, Scene
    from test_gpu_keyframe_bow import ISG, SG, _stereo_pair
    ob.lib()
    bow = Scene(978, 1000, 8, 4)
    m = osa.ORBmatcher(0.6, True)
    fx, fy, cx, cy, b = 458.654, 457.296, 367.215, 248.375, 0.11
    Kc = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    F = (np.linalg.inv(Kc).T @ np.array([[0, 0, 0], [0, 0, -b], [0, b, 0]]) @ np.linalg.inv(Kc)).astype(f32)
    eye, p4 = np.eye(3, dtype=f32), np.array([fx, fy, cx, cy], f32)
    views = [[dict(R=eye, t=np.zeros(3, f32), Ow=np.zeros(3, f32), p=p4)], [dict(R=eye, t=np.array([-b, 0, 0], f32), Ow=np.array([b, 0, 0], f32), p=p4)]]
    a, q = _stereo_pair(ob, m, bow, 2, 1000, True)
    n = len(a.d)
    kfs_host, dev = [], []
    for kf in (a, q):
        disp = kf.k["x"] - kf.ur
        depth = np.where(kf.ur >= 0, f32(b * fx) / np.where(kf.ur >= 0, disp, 1).astype(f32), f32(-1)).astype(f32)
        xy = np.stack([kf.k["x"], kf.k["y"]], axis=1).astype(f32)
        kfs_host.append(dict(n_left=n, n_right=-1, x=kf.k["x"].astype(f32), y=kf.k["y"].astype(f32), octave=kf.k["octave"].astype(np.int32), u_right=kf.ur,
                             depth=depth, keys_xy=xy, scale=SF, sigma2=SG))
        d = osa.DeviceKeyFrame.create_host_stereo(m, kf.view, depth, xy, ISG)
        d.compute_bow(m, bow.voc, 2, download=False)
        dev.append(d)
    base = dict(views=views, ratio_factor=f32(1.8), inertial=0, far_points=0, th_far_points=0.0, mb=(f32(b), f32(b)), mbf=(f32(b * fx), f32(b * fx)))
    sc = dict(rig=False, key_frames=kfs_host, variants=dict(base=base))
    v1, v2 = m.NewPointsViews((eye, views[0][0]["t"], views[0][0]["Ow"], fx, fy, cx, cy), (eye, views[1][0]["t"], views[1][0]["Ow"], fx, fy, cx, cy))
    st = osa._lib.NewPointsStereo(b, b * fx, b, b * fx)
    ep = (1e6, 1e6)

    def plain():
        return m.SearchAndTriangulateResident(dev[0], dev[1], None, None, SG, SG, F, ep, v1, v2, 1.8, False, True)

    def stereo():
        return m.SearchAndTriangulateResident(dev[0], dev[1], None, None, SG, SG, F, ep, v1, v2, 1.8, False, True, stereo=st)

    nm, m12, _, _, pst = plain()
    idx1 = np.arange(n, dtype=np.int32)
    wst, wpos, info = S.reference_stereo(sc, "base", idx1, m12)
    ok = wst == N.OK
    decided = info["path"] != 0
    times = {"plain": [], "stereo": []}
    for rep in range(warmup + reps):
        for name, fn in (("plain", plain), ("stereo", stereo)):
            t0 = time.perf_counter()
            fn_, row, acc, pos, status = fn()
            dt = time.perf_counter() - t0
            assert fn_ == nm and np.array_equal(row, m12), (name, rep)
            if name == "stereo":
                assert acc == int(ok.sum()) and np.array_equal(status, wst) and np.array_equal(S.bits(pos[ok]), S.bits(wpos[ok])), rep
            else:
                assert (status[decided] == N.STEREO_LEFT_TO_HOST).all() and np.array_equal(status[~decided], wst[~decided]), rep
            if rep >= warmup:
                times[name].append(dt * 1e6)
    for name, t in times.items():
        stats(res, f"fused_{name}", t)
    res["fused_features"], res["fused_matches"], res["fused_plain_undecided"], res["fused_stereo_accepted"] = [n, n], int(nm), int(decided.sum()), int(ok.sum())
    res["fused_unprojected"], res["fused_stereo_triangulated"] = int((info["path"] >= 2).sum()), int((info["path"] == 1).sum())
    spread = res["fused_plain_max_us"] - res["fused_plain_min_us"]
    res["fused_stereo_minus_plain_us"] = round(res["fused_stereo_med_us"] - res["fused_plain_med_us"], 1)
    res["fused_stereo_within_spread"] = bool(res["fused_stereo_med_us"] <= res["fused_plain_med_us"] + spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--rgbd-child", action="store_true")
    args = ap.parse_args()
    if args.rgbd_child:
        rgbd_child(args.reps)
        return
    res = {"tool": "stereo_resident_latency", "reps": args.reps}
    resident(res, args.reps, args.warmup)
    fused(res, args.reps, args.warmup)
    if not args.no_trace:
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="stereo_resident_trace_"))
        out_dir.mkdir(parents=True, exist_ok=True)
        rgbd(res, out_dir)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
