#!/usr/bin/env python3
"""What converting colour, resizing and CLAHE-equalizing raw frames on the device costs (not imported by bench.py).  256 frames per workload:
  gray          752 x 480 from 3 interleaved channels (BGR)
  resize_half   752 x 480 from 1504 x 960 (k_resize_half)
  resize        752 x 480 from 1000 x 640 (k_resize, the generic path)
  clahe_512     512 x 512, CLAHE 3.0 / 8 x 8   (k_clahe_lut + k_clahe_apply; TUM-VI's 512 x 512 sequences)
  clahe_1024    1024 x 1024, the same          (TUM-VI's 1024 x 1024 sequences)
Per workload:
  step     (a) stage + extract_batch_device + sync against (b) extract_batch_device + sync on the same prepared frames, and (c) stage + sync alone;
           `price_us` = (a) - (b) medians, beside (b)'s own max - min (`extract_spread_us`) and as a share of (b) (`price_share`)
  kernel   each kernel's time from one serialized rocprofv3 --kernel-trace --stats run of a child (no counters), its compulsory traffic over that
           time, and beside it a device-to-device copy of the stage's source + destination bytes timed by device events in this process
  host     the same arithmetic as a C++ loop on one core (image_enhance_host_loop.cpp, g++ -O3, its own clock, fastest of 2 repetitions); its output
           must be the device's, every frame.  It is not OpenCV's SIMD code; OpenCV's own speed is not measured.
Timed repetitions with the forms alternating, every output checked in every repetition; median (min - max) in microseconds, host clock around calls
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

B = 256
# name -> (kind, source width, source height, destination width, destination height)
WORKLOADS = {"gray": ("gray", 752, 480, 752, 480), "resize_half": ("resize", 1504, 960, 752, 480), "resize": ("resize", 1000, 640, 752, 480),
             "clahe_512": ("clahe", 512, 512, 512, 512), "clahe_1024": ("clahe", 1024, 1024, 1024, 1024)}
KERNELS = {"gray": ["k_gray"], "resize_half": ["k_resize_half"], "resize": ["k_resize"], "clahe_512": ["k_clahe_lut", "k_clahe_apply"],
           "clahe_1024": ["k_clahe_lut", "k_clahe_apply"]}


def stats(res, key, a):
    a = np.array(a)
    res[f"{key}_med_us"], res[f"{key}_min_us"], res[f"{key}_max_us"] = round(float(np.median(a)), 1), round(float(a.min()), 1), round(float(a.max()), 1)


def compulsory_bytes(name):
    """Per kernel: every source byte once, every destination byte once, the tables once."""
    kind, sw, sh, dw, dh = WORKLOADS[name]
    if kind == "gray":
        return {"k_gray": B * sw * sh * 4}
    if name == "resize_half":
        return {"k_resize_half": B * (sw * sh + dw * dh)}
    if kind == "resize":
        return {"k_resize": B * (sw * sh + dw * dh) + 8 * dw + 16 * dh}
    return {"k_clahe_lut": B * (sw * sh + 64 * 256), "k_clahe_apply": B * (2 * sw * sh + 64 * 256)}


def setup(name):
    """(stage(ex): enqueue the workload's calls, the extractor, host source [B, ...], device source, device destination [B, dh, dw])"""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    kind, sw, sh, dw, dh = WORKLOADS[name]
    canvas = synth.make_canvas(7, size=2048, n_shapes=2400)
    some = np.stack([synth.frame_from_canvas(canvas, 5 * t, sw, sh, 900 + t) for t in range(8)])
    src = np.concatenate([np.roll(some, 3 * k, axis=2) for k in range(B // 8)])   # 256 different frames of the same scene
    if kind == "gray":
        src = np.ascontiguousarray(np.stack([src, 255 - src // 2, np.roll(src, 1, axis=2)], axis=-1))
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.zeros((B, dh, dw), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ex = osa.ORBextractor(1000, 1.2, 8, 20, 7)
    if kind == "gray":
        stage = lambda: ex.gray_batch(d_src.data_ptr(), B, sw, sh, 3, False, 3 * sw, 3 * sw * sh, d_dst.data_ptr(), dw, dw * dh)   # noqa: E731
    elif kind == "resize":
        stage = lambda: ex.resize_batch(d_src.data_ptr(), B, sw, sh, sw, sw * sh, d_dst.data_ptr(), dw, dh, dw, dw * dh)   # noqa: E731
    else:
        clahe = osa.DeviceClahe(3.0, (8, 8))
        stage = lambda: clahe.apply_batch(ex, d_src.data_ptr(), B, sw, sh, sw, sw * sh, d_dst.data_ptr(), dw, dw * dh)   # noqa: E731
    return stage, ex, src, d_src, d_dst


def host_loop(name, src, L):
    kind, sw, sh, dw, dh = WORKLOADS[name]
    out = np.zeros((B, dh, dw), np.uint8)
    if kind == "gray":
        us = L.gray_host_loop(src.ctypes.data, B, sw, sh, 3, 0, out.ctypes.data, 2)
    elif kind == "resize":
        us = L.resize_host_loop(src.ctypes.data, B, sw, sh, out.ctypes.data, dw, dh, 2)
    else:
        us = L.clahe_host_loop(src.ctypes.data, B, sw, sh, 3.0, 8, 8, out.ctypes.data, 2)
    return out, float(us)


def step(name, reps, warmup, L):
    import torch
    res = {}
    kind, sw, sh, dw, dh = WORKLOADS[name]
    stage, ex, src, d_src, d_dst = setup(name)
    stage()
    ex.sync()
    want_dst = d_dst.cpu().numpy()
    host_out, host_us = host_loop(name, src, L)
    assert np.array_equal(host_out, want_dst), name   # the device's bytes are the loop's, every frame
    d_fixed = d_dst.clone()   # form (b)'s frames: never written again
    torch.cuda.synchronize()

    def a():
        stage()
        ex.extract_batch_device(d_dst.data_ptr(), B, dw, dh, dw, dw * dh, (0, 0))
        ex.sync()

    def b():
        ex.extract_batch_device(d_fixed.data_ptr(), B, dw, dh, dw, dw * dh, (0, 0))
        ex.sync()

    def c():
        stage()
        ex.sync()

    b()
    want = [x.copy() for x in ex.download_all()]
    times = {"stage_extract": [], "extract": [], "stage": []}
    for rep in range(warmup + reps):
        for form, fn in (("stage_extract", a), ("extract", b), ("stage", c)):
            if form != "extract":
                d_dst.zero_()
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if form == "stage":
                assert torch.equal(d_dst, d_fixed), (name, rep)
            else:
                got = ex.download_all()
                assert all(np.array_equal(g, w) for g, w in zip(got[2:], want[2:])), (name, form, rep)
                n = want[2].astype(np.int64)
                mask = np.arange(got[0].shape[1])[None, :] < n[:, None]
                assert got[0][mask].tobytes() == want[0][mask].tobytes() and np.array_equal(got[1][mask], want[1][mask]), (name, form, rep)
            if rep >= warmup:
                times[form].append(dt * 1e6)
    for form, t in times.items():
        stats(res, form, t)
    res["frames"], res["src_shape"], res["dst_shape"], res["features"] = B, [sw, sh], [dw, dh], int(want[2].sum())
    res["price_us"] = round(res["stage_extract_med_us"] - res["extract_med_us"], 1)
    res["extract_spread_us"] = round(res["extract_max_us"] - res["extract_min_us"], 1)
    res["price_share"] = round(res["price_us"] / res["extract_med_us"], 3)
    # a device-to-device copy of as many bytes as the stage must read and write, timed by device events
    nbytes = int(src.nbytes + B * dw * dh)
    d_a = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
    d_b = torch.ones(nbytes // 2, dtype=torch.uint8, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_us = []
    for rep in range(warmup + reps):
        ev0.record()
        d_a.copy_(d_b)
        ev1.record()
        ev1.synchronize()
        if rep >= warmup:
            copy_us.append(ev0.elapsed_time(ev1) * 1e3)
    stats(res, "copy", copy_us)
    res["copy_bytes"] = nbytes
    res["copy_gb_per_s"] = round(nbytes / (res["copy_med_us"] * 1e-6) / 1e9, 1)
    res["host_loop_min_us"] = round(host_us, 1)
    res["device_below_host_min"] = bool(res["stage_med_us"] < res["host_loop_min_us"])
    return res


def kernel_child(name, reps):
    stage, ex, _, _, _ = setup(name)
    for _ in range(reps):
        stage()
    ex.sync()


def kernel(name, res, out_dir):
    exe = shutil.which("rocprofv3")
    if not exe:
        raise RuntimeError("rocprofv3 is not installed")
    d = Path(out_dir) / ("kt_" + name)
    shutil.rmtree(d, ignore_errors=True)
    r = subprocess.run([exe, "--kernel-trace", "--stats", "-d", str(d), "-o", "kt", "--", sys.executable, str(Path(__file__).resolve()), "--kernel-child", name,
                        "--reps", "20"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the traced child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    dbs = sorted(d.rglob("*.db"), key=lambda p: p.stat().st_size)
    if not dbs:
        raise RuntimeError("rocprofv3 wrote no .db")
    need = compulsory_bytes(name)
    res["kernels"] = {}
    for kname, calls, total, avg in sqlite3.connect(str(dbs[-1])).execute("select name, total_calls, total_duration, average from top_kernels"):
        for k in KERNELS[name]:
            if k + "(" in kname or kname == k or kname.endswith("::" + k) or ("4orbx" + str(len(k)) + k) in kname:
                us = float(avg)   # (the view's durations are microseconds)
                res["kernels"][k] = {"calls": int(calls), "avg_us": round(us, 2), "compulsory_bytes": need[k], "gb_per_s": round(need[k] / (us * 1e-6) / 1e9, 1)}
    shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--kernel-child", default="")
    args = ap.parse_args()
    if args.kernel_child:
        kernel_child(args.kernel_child, args.reps)
        return
    res = {"tool": "image_enhance_latency", "reps": args.reps, "workloads": {}}
    with tempfile.TemporaryDirectory() as td:
        so = Path(td) / "host_loop.so"
        subprocess.run(["g++", "-O3", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(Path(__file__).with_name("image_enhance_host_loop.cpp"))], check=True)
        L = C.CDLL(str(so))
        vp, i32 = C.c_void_p, C.c_int
        L.gray_host_loop.restype = L.resize_host_loop.restype = L.clahe_host_loop.restype = C.c_double
        L.gray_host_loop.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32]
        L.resize_host_loop.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32]
        L.clahe_host_loop.argtypes = [vp, i32, i32, i32, C.c_double, i32, i32, vp, i32]
        out_dir = Path(args.out).parent if args.out else Path(tempfile.mkdtemp(prefix="image_enhance_trace_"))
        out_dir.mkdir(parents=True, exist_ok=True)
        for name in WORKLOADS:
            if args.only and name not in args.only.split(","):
                continue
            res["workloads"][name] = step(name, args.reps, args.warmup, L)
            if not args.no_trace:
                kernel(name, res["workloads"][name], out_dir)
            print(name, json.dumps(res["workloads"][name]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
