#!/usr/bin/env python3
"""What rectifying raw stereo frames on the device costs (not imported by bench.py).  256 frames of 752 x 480 and a radial-tangential map of EuRoC's
strength.  Measurements:
  step     (a) rectify_batch + extract_batch_device + sync against (b) extract_batch_device + sync on the same rectified frames, and (c) rectify_batch +
           sync alone; `rectify_price_us` = (a) - (b) medians, beside (b)'s own max - min
  kernel   k_rectify's time from one serialized rocprofv3 --kernel-trace --stats run of a child (no counters), its compulsory traffic (the map once,
           every source byte once, every destination byte once) over that time, and beside it a device-to-device copy of the same frames timed by
           device events in this process (bytes read + written over time)
  host     the same arithmetic as a C++ loop on one core (image_prep_host_loop.cpp, g++ -O3, its own clock, fastest of 3 repetitions); its output
           must be the device's.  It is not cv::remap's SIMD code; OpenCV's own speed is not measured.  `device_below_host_min`: (c)'s median lies
           below the loop's minimum
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

f32 = np.float32
B, W, H = 256, 752, 480


def stats(res, key, a):
    a = np.array(a)
    res[f"{key}_med_us"], res[f"{key}_min_us"], res[f"{key}_max_us"] = round(float(np.median(a)), 1), round(float(a.min()), 1), round(float(a.max()), 1)


def euroc_like_maps():
    """initUndistortRectifyMap's field for EuRoC cam0's intrinsics and distortion (no rotation): where the rectified pixel lies in the raw image."""
    fx, fy, cx, cy, k1, k2, p1, p2 = 458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    xn, yn = (x - cx) / fx, (y - cy) / fy
    r2 = xn * xn + yn * yn
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd, yd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn), yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    return (fx * xd + cx).astype(f32), (fy * yd + cy).astype(f32)


def setup():
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    canvas = synth.make_canvas(7, size=2048, n_shapes=2400)
    raw = np.stack([synth.frame_from_canvas(canvas, t, W, H, 900 + t) for t in range(B)])
    mx, my = euroc_like_maps()
    d_raw = torch.from_numpy(raw).cuda()
    d_rect = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return osa.DeviceRectifier(mx, my), osa.ORBextractor(1000, 1.2, 8, 20, 7), raw, (mx, my), d_raw, d_rect


def rectify(rect, ex, d_raw, d_rect):
    rect.rectify_batch(ex, d_raw.data_ptr(), B, W, H, W, W * H, d_rect.data_ptr(), W, W * H)


def step(res, reps, warmup):
    import torch
    rect, ex, raw, maps, d_raw, d_rect = setup()
    rectify(rect, ex, d_raw, d_rect)
    ex.sync()
    want_rect = d_rect.cpu().numpy()
    d_fixed = d_rect.clone()   # form (b)'s frames: never written again
    torch.cuda.synchronize()

    def a():
        rectify(rect, ex, d_raw, d_rect)
        ex.extract_batch_device(d_rect.data_ptr(), B, W, H, W, W * H, (0, 0))
        ex.sync()

    def b():
        ex.extract_batch_device(d_fixed.data_ptr(), B, W, H, W, W * H, (0, 0))
        ex.sync()

    def c():
        rectify(rect, ex, d_raw, d_rect)
        ex.sync()

    b()
    want = [x.copy() for x in ex.download_all()]
    times = {"rectify_extract": [], "extract": [], "rectify": []}
    for rep in range(warmup + reps):
        for name, fn in (("rectify_extract", a), ("extract", b), ("rectify", c)):
            if name != "extract":
                d_rect.zero_()
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if name == "rectify":
                assert np.array_equal(d_rect.cpu().numpy(), want_rect), rep
            else:
                got = ex.download_all()
                assert all(np.array_equal(g, w) for g, w in zip(got[2:], want[2:])), (name, rep)
                for f in range(B):
                    n = int(want[2][f])
                    assert got[0][f, :n].tobytes() == want[0][f, :n].tobytes() and np.array_equal(got[1][f, :n], want[1][f, :n]), (name, rep, f)
            if rep >= warmup:
                times[name].append(dt * 1e6)
    for name, t in times.items():
        stats(res, name, t)
    res["frames"], res["shape"], res["features"] = B, [W, H], int(want[2].sum())
    res["rectify_price_us"] = round(res["rectify_extract_med_us"] - res["extract_med_us"], 1)
    res["extract_spread_us"] = round(res["extract_max_us"] - res["extract_min_us"], 1)
    # a device-to-device copy of the same frames: bytes read + written over the time between two device events
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_us = []
    for rep in range(warmup + reps):
        ev0.record()
        d_rect.copy_(d_fixed)
        ev1.record()
        ev1.synchronize()
        if rep >= warmup:
            copy_us.append(ev0.elapsed_time(ev1) * 1e3)
    stats(res, "copy", copy_us)
    res["copy_gb_per_s"] = round(2 * B * W * H / (res["copy_med_us"] * 1e-6) / 1e9, 1)
    # the host loop; its output must be the device's
    with tempfile.TemporaryDirectory() as td:
        so = Path(td) / "host_loop.so"
        subprocess.run(["g++", "-O3", "-shared", "-fPIC", "-o", str(so), str(Path(__file__).with_name("image_prep_host_loop.cpp"))], check=True)
        L = C.CDLL(str(so))
        L.remap_host_loop.restype = C.c_double
        L.remap_host_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        out = np.zeros((B, H, W), np.uint8)
        us = L.remap_host_loop(raw.ctypes.data, B, W, H, maps[0].ctypes.data, maps[1].ctypes.data, W, H, out.ctypes.data, 3)
    assert np.array_equal(out, want_rect)
    res["host_loop_min_us"] = round(float(us), 1)
    res["device_below_host_min"] = bool(res["rectify_med_us"] < res["host_loop_min_us"])
    res["outside_pixels_per_frame"] = int((want_rect[0] == 0).sum())


def kernel_child(reps):
    rect, ex, _, _, d_raw, d_rect = setup()
    for _ in range(reps):
        rectify(rect, ex, d_raw, d_rect)
    ex.sync()


def kernel(res, out_dir):
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 is not installed")
    d = Path(out_dir) / "kt"
    shutil.rmtree(d, ignore_errors=True)
    r = subprocess.run([exe, "--kernel-trace", "--stats", "-d", str(d), "-o", "kt", "--", sys.executable, str(Path(__file__).resolve()), "--kernel-child",
                        "--reps", "20"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the traced child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    dbs = sorted(d.rglob("*.db"), key=lambda p: p.stat().st_size)
    if not dbs:
        raise RuntimeError("rocprofv3 wrote no .db")
    for name, calls, total, avg in sqlite3.connect(str(dbs[-1])).execute("select name, total_calls, total_duration, average from top_kernels"):
        if "k_rectify" in name:
            res["kernel_calls"], res["kernel_avg_us"] = int(calls), round(float(avg), 2)   # (the view's durations are microseconds)
    shutil.rmtree(d, ignore_errors=True)
    res["kernel_compulsory_bytes"] = 6 * W * H + 2 * B * W * H
    res["kernel_gb_per_s"] = round(res["kernel_compulsory_bytes"] / (res["kernel_avg_us"] * 1e-6) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--kernel-child", action="store_true")
    args = ap.parse_args()
    if args.kernel_child:
        kernel_child(args.reps)
        return
    res = {"tool": "image_prep_latency", "reps": args.reps}
    step(res, args.reps, args.warmup)
    if not args.no_trace:
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="image_prep_trace_"))
        out_dir.mkdir(parents=True, exist_ok=True)
        kernel(res, out_dir)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
