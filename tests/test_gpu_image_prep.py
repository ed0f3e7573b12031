"""Raw sensor images on the device: orbx_rectify_batch_device (System::TrackStereo's cv::remap in front of the extractor) and
orbx_rgbd_batch_device_u16 (Tracking::GrabImageRGBD's convertTo folded into Frame::ComputeStereoFromRGBD), against tests/image_prep_scene.py's integer
restatement, bit for bit.  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import ctypes as C
import os

import numpy as np
import pytest

import image_prep_scene as S

pytestmark = pytest.mark.gpu
BAD, STALE = -2, -9   # ORBX_E_BAD_ARG, ORBX_E_STALE
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))
BF, BASELINE = float(np.float32(0.53716 * 718.856)), float(np.float32(0.53716))
# (source row stride, source offset, destination row stride, destination offset) on the base shape: strides above the widths; "odd" has an odd destination
# stride and odd offsets (rows start at every alignment: the byte stores), "aligned" rows that start on a dword (the dword stores, the last group aside)
LAYOUTS = {"odd": (S.SW + 3, 5, S.DW + 4, 3), "aligned": (S.SW + 7, 0, S.DW + 5, 0)}


def _extractor(nf=500):
    import orb_slam3_amd as osa
    return osa.ORBextractor(nf, 1.2, 8, 20, 7)


@pytest.fixture(scope="module")
def ex():
    return _extractor()


def _buffers(src, dw, dh, s_rs, s_off, d_rs, d_off, seed=3):
    """Host images of the two device buffers: the frames inside random bytes (5 / 9 bytes between the frames), and where the destination rectangles lie."""
    n, sh, sw = src.shape
    rng = np.random.default_rng(seed)
    s_fs, d_fs = s_rs * sh + 5, d_rs * dh + 9
    sbuf = rng.integers(0, 256, s_off + n * s_fs + 8, dtype=np.uint8)
    dbuf = rng.integers(0, 256, d_off + n * d_fs + 8, dtype=np.uint8)
    inside = np.zeros(dbuf.shape, bool)
    for f in range(n):
        np.lib.stride_tricks.as_strided(sbuf[s_off + f * s_fs:], (sh, sw), (s_rs, 1))[:] = src[f]
        np.lib.stride_tricks.as_strided(inside[d_off + f * d_fs:], (dh, dw), (d_rs, 1))[:] = True
    return sbuf, s_fs, dbuf, d_fs, inside


def _rectify(rect, ex, src, layout, call=None):
    """rectify_batch of src [n, sh, sw] through device buffers laid out as `layout`; returns (rectified [n, dh, dw], the bytes outside the
    rectangles are the ones the buffer held before)."""
    import torch
    dw, dh = rect.width, rect.height
    s_rs, s_off, d_rs, d_off = layout
    sbuf, s_fs, dbuf, d_fs, inside = _buffers(src, dw, dh, s_rs, s_off, d_rs, d_off)
    d_s, d_d = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf.copy()).cuda()
    assert d_s.data_ptr() % 4 == 0 and d_d.data_ptr() % 4 == 0
    n, sh, sw = src.shape
    (call or rect.rectify_batch)(ex, d_s.data_ptr() + s_off, n, sw, sh, s_rs, s_fs, d_d.data_ptr() + d_off, d_rs, d_fs)
    ex.sync()
    out = d_d.cpu().numpy()
    got = np.stack([np.lib.stride_tricks.as_strided(out[d_off + f * d_fs:], (dh, dw), (d_rs, 1)).copy() for f in range(n)])
    return got, np.array_equal(out[~inside], dbuf[~inside])


# ---- (1) the arithmetic ----
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cls", S.CLASSES)
def test_every_map_class_bit_for_bit(ex, cls, layout):
    """The base shape (3 frames, 61 x 17 -> 67 x 13): every frame equals the reference, every byte outside the written rectangles keeps its value."""
    import orb_slam3_amd as osa
    mx, my, want = S.base_case(cls)
    got, untouched = _rectify(osa.DeviceRectifier(mx, my), ex, S.sources(), LAYOUTS[layout])
    assert np.array_equal(got, want), (cls, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    assert untouched, cls


@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("dw", [1, 3, 4, 5, 63, 65])
def test_frame_counts_and_widths(ex, n, dw):
    """1, 3 and 9 frames (a part of a chunk of four, and two chunks and a part) at destination widths around the four-pixel group and around 64: the
    distortion class and the far-edge class, both layouts, and a map whose rows are further apart than its width."""
    import orb_slam3_amd as osa
    src = S.sources(frames=n)
    for cls in ("distortion", "at_the_far_edge"):
        mx, my = S.make_maps(cls, dw, S.DH)
        want = np.stack([S.reference_remap(s, mx, my) for s in src])
        wide = np.full((S.DH, dw + 3), np.nan, np.float32)   # what lies between the map's rows is never read
        wx, wy = wide.copy(), wide.copy()
        wx[:, :dw], wy[:, :dw] = mx, my
        for name, (s_rs, s_off, d_rs, d_off) in LAYOUTS.items():
            lay = (s_rs, s_off, d_rs - S.DW + dw, d_off)
            for rect in (osa.DeviceRectifier(mx, my), _strided_rectifier(wx, wy, dw)):
                got, untouched = _rectify(rect, ex, src, lay)
                assert np.array_equal(got, want), (cls, name, int((got != want).sum()))
                assert untouched, (cls, name)


def _strided_rectifier(wx, wy, dw):
    """A rectifier made through the C ABI from maps with map_stride > dst_width."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    r = osa.DeviceRectifier.__new__(osa.DeviceRectifier)
    r._L, r._h, r.width, r.height, r.device = _lib.lib(), C.c_void_p(), dw, wx.shape[0], 0
    assert r._L.orbx_rectifier_create(0, _lib.ptr(wx), _lib.ptr(wy), dw, wx.shape[0], wx.shape[1], C.byref(r._h)) == 0
    return r


def test_one_rectifier_two_extractors(ex):
    import orb_slam3_amd as osa
    mx, my, want = S.base_case("distortion")
    rect, other = osa.DeviceRectifier(mx, my), _extractor()
    for e in (ex, other, ex):
        got, untouched = _rectify(rect, e, S.sources(), LAYOUTS["odd"])
        assert np.array_equal(got, want) and untouched


# ---- (2) in front of the extractor ----
RAW_W, RAW_H, W, H = 336, 250, 320, 240
_E2E = {}


def _e2e_reference(canvas, B, w=W, h=H):
    """B raw frames of (w + 16) x (h + 10), their reference rectification to w x h, and what an extractor gives for the rectified frames uploaded the
    ordinary way: computed once."""
    if (B, w, h) not in _E2E:
        import torch
        from orb_slam3_amd import synth
        raw = np.stack([synth.frame_from_canvas(canvas, 3 * t, w + 16, h + 10, 900 + t) for t in range(B)])
        mx, my = S.smooth_maps(w, h, w + 16, h + 10)
        want = np.stack([S.reference_remap(r, mx, my) for r in raw])
        e = _extractor()
        d = torch.from_numpy(want.copy()).cuda()
        e.extract_batch_device(d.data_ptr(), B, w, h, w, w * h, (0, 0))
        outs = [e.download(f) for f in range(B)]
        level0 = e.get_level(0, B - 1)
        e.sync()
        for a in (raw, want, level0):
            a.setflags(write=False)
        _E2E[(B, w, h)] = dict(raw=raw, maps=(mx, my), want=want, outs=outs, level0=level0)
    return _E2E[(B, w, h)]


def check_rectify_then_extract(canvas, w, h, B, in_place):
    """rectify_batch and extract_batch_device with nothing between them == the reference-rectified frames extracted the ordinary way: key points,
    descriptors, (larger batches) orbx_get_level(0) before any wait, and afterwards the rectified bytes themselves.  in_place: the batch must have
    read level 0 from d_dst itself -- only such a batch, if it never copied level 0, has none after orbx_sync."""
    import torch
    import orb_slam3_amd as osa
    R = _e2e_reference(canvas, B, w, h)
    rw, rh = w + 16, h + 10
    rect, e = osa.DeviceRectifier(*R["maps"]), _extractor()
    d_raw, d_dst = torch.from_numpy(R["raw"].copy()).cuda(), torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # the buffers are complete; from here on only the extractor's stream orders anything
    rect.rectify_batch(e, d_raw.data_ptr(), B, rw, rh, rw, rw * rh, d_dst.data_ptr(), w, w * h)
    e.extract_batch_device(d_dst.data_ptr(), B, w, h, w, w * h, (0, 0))
    if B > 2:
        assert np.array_equal(e.get_level(0, B - 1), R["level0"])
    total = 0
    for f in range(B):
        mono, kps, desc = e.download(f)
        omono, okps, odesc = R["outs"][f]
        assert mono == omono and kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc), f
        total += len(kps)
    e.sync()
    assert np.array_equal(d_dst.cpu().numpy(), R["want"])
    d_dst.zero_()
    torch.cuda.synchronize()
    rect.rectify_batch(e, d_raw.data_ptr(), B, rw, rh, rw, rw * rh, d_dst.data_ptr(), w, w * h)
    e.extract_batch_device(d_dst.data_ptr(), B, w, h, w, w * h, (0, 0))
    e.sync()
    if in_place:
        with pytest.raises(osa.OrbxError) as err:
            e.get_level(0, 0)
        assert err.value.status == STALE
    else:
        assert np.array_equal(e.get_level(0, B - 1), R["level0"])
    for f in (0, B - 1):
        assert e.download(f)[1].tobytes() == R["outs"][f][1].tobytes(), f
    return total


@pytest.mark.parametrize("B", [2, 48])
def test_rectify_then_extract_without_a_wait(canvas1, B):
    """320 x 240, 2 and 48 frames, with orbx_get_level(0) before the wait for the 48.  (Both batches copy level 0: at 320 x 240 the smallest pyramid
    levels have FAST cells too large for the strip kernel, which reading level 0 in place needs.  The next test is the in-place route.)"""
    assert check_rectify_then_extract(canvas1, W, H, B, False) > 100 * B


def test_rectify_then_extract_in_place(canvas1, monkeypatch):
    """517 x 389, 48 frames: the extraction reads level 0 from the rectified frames in place, and orbx_get_level(0) copies it from them before the
    wait.  (On the CPU emulator, for its speed: 5 frames, the in-place route forced by ORBX_PYR_STREAM_MIN as tests/test_gpu_level0_in_place.py does.)"""
    B = 48
    if EMULATOR:
        B = 5
        monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,20")
    assert check_rectify_then_extract(canvas1, 517, 389, B, True) > 300 * B


def test_two_rectified_extractors_then_the_stereo_stage(canvas1):
    """A left and a right extractor with a rectifier each, then orbx_stereo_batch_device: mvuRight / mvDepth equal those of the host-rectified route."""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import synth
    B = 2
    pairs = [synth.make_stereo_pair(1, 4 * t, RAW_W, RAW_H, canvas1) for t in range(B)]
    raw = [np.stack([p[side] for p in pairs]) for side in (0, 1)]
    maps = [S.smooth_maps(W, H, RAW_W, RAW_H), S.smooth_maps(W, H, RAW_W, RAW_H, strength=1.05)]
    results = {}
    for route in ("host", "device"):
        exs, keep = [_extractor(), _extractor()], []
        for side in (0, 1):
            if route == "host":
                d = torch.from_numpy(np.stack([S.reference_remap(r, *maps[side]) for r in raw[side]])).cuda()
                keep.append(d)
            else:
                d_raw, d = torch.from_numpy(raw[side]).cuda(), torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                keep += [d_raw, d]
                rect = osa.DeviceRectifier(*maps[side])
                keep.append(rect)
                rect.rectify_batch(exs[side], d_raw.data_ptr(), B, RAW_W, RAW_H, RAW_W, RAW_W * RAW_H, d.data_ptr(), W, W * H)
            exs[side].extract_batch_device(d.data_ptr(), B, W, H, W, W * H, (0, 0))
        exs[0].stereo_batch_device(exs[1], BF, BASELINE)
        results[route] = [exs[0].stereo_download(t) for t in range(B)]
        exs[0].sync()
        exs[1].sync()
    for t in range(B):
        (nm, ur, d), (wnm, wur, wd) = results["device"][t], results["host"][t]
        assert nm == wnm and ur.tobytes() == wur.tobytes() and d.tobytes() == wd.tobytes(), t
        assert nm > 20 and len(ur) > 100, (t, nm, len(ur))


# ---- (3) the 16-bit depth image ----
@pytest.mark.parametrize("factor", S.DEPTH_FACTORS, ids=["1/5000", "1/1000"])
def test_rgbd_u16_equals_rgbd_on_the_converted_images(canvas1, factor):
    """A 2-frame 320 x 240 batch, the pitch above the row, holes of 0, the designed raw values under the first key points:
    rgbd_batch_u16 == RGBDBatch on the reference-converted float images, every bit of mvuRight / mvDepth and the counts."""
    import torch
    from orb_slam3_amd import synth
    import stereo_resident_scene as SR
    B, pitch16, pitch32 = 2, 2 * W + 6, 4 * W + 8
    e = _extractor()
    e.set_camera(SR.CAMERA)
    d_frames = torch.from_numpy(np.stack([synth.frame_from_canvas(canvas1, 5 * t, W, H, 700 + t) for t in range(B)])).cuda()
    e.extract_batch_device(d_frames.data_ptr(), B, W, H, W, W * H, (0, 0))
    kps = [e.download(f)[1] for f in range(B)]
    yy, xx = np.mgrid[0:H, 0:W]
    raw = np.zeros((B, H, pitch16 // 2), np.uint16)
    for f in range(B):
        img = (300 + (xx * 13 + yy * 7 + 1000 * f) % 60000).astype(np.uint16)
        img[((xx // 16 + yy // 16) % 5) == 0] = 0
        for i in range(min(len(kps[f]), 4 * len(S.DEPTH_RAW))):
            img[int(kps[f]["y"][i]), int(kps[f]["x"][i])] = S.DEPTH_RAW[i % len(S.DEPTH_RAW)]
        raw[f, :, :W] = img
        raw[f, :, W:] = 0xabcd
    conv = np.full((B, H, pitch32 // 4), np.float32(777), np.float32)
    conv[:, :, :W] = S.reference_depth(raw[:, :, :W], factor)
    d_raw, d_conv = torch.from_numpy(raw).cuda(), torch.from_numpy(conv).cuda()
    e.RGBDBatch(d_conv.data_ptr(), pitch32, pitch32 * H, BF)
    want = [e.stereo_download(f) for f in range(B)]
    e.sync()
    e.rgbd_batch_u16(d_raw.data_ptr(), pitch16, pitch16 * H, float(factor), BF)
    for f in range(B):
        (nm, ur, d), (wnm, wur, wd) = e.stereo_download(f), want[f]
        assert nm == wnm and ur.tobytes() == wur.tobytes() and d.tobytes() == wd.tobytes(), f
        assert 50 < nm < len(ur) and (d == -1).any() and len(ur) == len(kps[f]), (f, nm)
    # the refusals leave the stage's results alone
    from orb_slam3_amd import _lib
    L, p, fs = _lib.lib(), C.c_void_p(d_raw.data_ptr()), pitch16 * H
    fresh = _extractor()
    refused = [L.orbx_rgbd_batch_device_u16(None, p, pitch16, fs, factor, BF), L.orbx_rgbd_batch_device_u16(e._h, None, pitch16, fs, factor, BF),
               L.orbx_rgbd_batch_device_u16(e._h, p, 2 * W - 2, fs, factor, BF), L.orbx_rgbd_batch_device_u16(e._h, p, pitch16 + 1, fs, factor, BF),
               L.orbx_rgbd_batch_device_u16(e._h, p, pitch16, fs + 1, factor, BF), L.orbx_rgbd_batch_device_u16(e._h, C.c_void_p(p.value + 1), pitch16, fs, factor, BF),
               L.orbx_rgbd_batch_device_u16(e._h, p, pitch16, fs, 0.0, BF), L.orbx_rgbd_batch_device_u16(e._h, p, pitch16, fs, -1.0, BF),
               L.orbx_rgbd_batch_device_u16(e._h, p, pitch16, fs, float("nan"), BF), L.orbx_rgbd_batch_device_u16(e._h, p, pitch16, fs, float("inf"), BF),
               L.orbx_rgbd_batch_device_u16(e._h, p, pitch16, fs, factor, 0.0), L.orbx_rgbd_batch_device_u16(fresh._h, p, pitch16, fs, factor, BF)]
    assert refused == [BAD] * len(refused), refused
    nm, ur, d = e.stereo_download(1)
    assert nm == want[1][0] and ur.tobytes() == want[1][1].tobytes()


# ---- (4) refusals ----
def test_rectify_refusals_change_nothing(canvas1):
    """Every refusal returns ORBX_E_BAD_ARG, leaves d_dst as it was and the extractor's batch alone; the same extractor and rectifier work afterwards.
    (An extractor on another device than the rectifier's needs two devices: checked where there are two.)"""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L, vp = _lib.lib(), C.c_void_p
    mx, my, want = S.base_case("distortion")
    rect, e = osa.DeviceRectifier(mx, my), _extractor()
    R = _e2e_reference(canvas1, 2)
    d_img = torch.from_numpy(R["want"].copy()).cuda()
    e.extract_batch_device(d_img.data_ptr(), 2, W, H, W, W * H, (0, 0))
    before = e.download(1)
    view = e.batch_view()
    src = S.sources()
    s_rs, s_off, d_rs, d_off = LAYOUTS["odd"]
    sbuf, s_fs, dbuf, d_fs, _ = _buffers(src, S.DW, S.DH, s_rs, s_off, d_rs, d_off)
    d_s, d_d = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf.copy()).cuda()
    ps, pd = d_s.data_ptr() + s_off, d_d.data_ptr() + d_off
    ok = (rect._h, e._h, vp(ps), S.FRAMES, S.SW, S.SH, s_rs, s_fs, vp(pd), d_rs, d_fs)

    def call(**kw):
        names = ("r", "ex", "src", "n", "sw", "sh", "s_rs", "s_fs", "dst", "d_rs", "d_fs")
        return L.orbx_rectify_batch_device(*[kw.get(k, v) for k, v in zip(names, ok)])

    refused = dict(null_rectifier=call(r=None), null_extractor=call(ex=None), null_src=call(src=None), null_dst=call(dst=None),
                   no_frames=call(n=0), negative_frames=call(n=-1), zero_width=call(sw=0), zero_height=call(sh=0), wide=call(sw=32767, s_rs=40000),
                   high=call(sh=32767), src_stride=call(s_rs=S.SW - 1), dst_stride=call(d_rs=S.DW - 1), dst_frames_overlap=call(d_fs=d_rs * (S.DH - 1)),
                   dst_is_src=call(dst=vp(ps)), dst_ends_in_src=call(dst=vp(ps - (S.FRAMES - 1) * d_fs - (S.DH - 1) * d_rs - S.DW + 1)),
                   dst_starts_in_src=call(dst=vp(ps + (S.FRAMES - 1) * s_fs + (S.SH - 1) * s_rs + S.SW - 1)))
    if torch.cuda.device_count() > 1 and not EMULATOR:
        refused["other_device"] = L.orbx_rectify_batch_device(rect._h, osa.ORBextractor(500, 1.2, 8, 20, 7, device=1)._h, *ok[2:])
    assert all(v == BAD for v in refused.values()), refused
    h = vp()
    nan = np.zeros((2, 2), np.float32)
    created = [L.orbx_rectifier_create(0, None, _lib.ptr(nan), 2, 2, 2, C.byref(h)), L.orbx_rectifier_create(0, _lib.ptr(nan), None, 2, 2, 2, C.byref(h)),
               L.orbx_rectifier_create(0, _lib.ptr(nan), _lib.ptr(nan), 2, 2, 2, None), L.orbx_rectifier_create(0, _lib.ptr(nan), _lib.ptr(nan), 0, 2, 2, C.byref(h)),
               L.orbx_rectifier_create(0, _lib.ptr(nan), _lib.ptr(nan), 2, 32767, 2, C.byref(h)), L.orbx_rectifier_create(0, _lib.ptr(nan), _lib.ptr(nan), 2, 2, 1, C.byref(h))]
    assert created == [BAD] * len(created) and not h.value, created
    e.sync()
    assert np.array_equal(d_d.cpu().numpy(), dbuf) and np.array_equal(d_s.cpu().numpy(), sbuf)
    after, view2 = e.download(1), e.batch_view()
    assert (view2.n_frames, view2.cap) == (view.n_frames, view.cap) and after[0] == before[0]
    assert after[1].tobytes() == before[1].tobytes() and np.array_equal(after[2], before[2])
    # the same rectifier and extractor afterwards
    got, untouched = _rectify(rect, e, src, LAYOUTS["odd"])
    assert np.array_equal(got, want) and untouched
    e.extract_batch_device(d_img.data_ptr(), 2, W, H, W, W * H, (0, 0))
    again = e.download(1)
    assert again[1].tobytes() == before[1].tobytes() and np.array_equal(again[2], before[2])
