"""Colour, size and contrast of raw frames on the device: orbx_gray_batch_device (Tracking::GrabImage*'s cvtColor), orbx_resize_batch_device
(System::Track*'s cv::resize) and orbx_clahe_batch_device (the TUM-VI examples' CLAHE) through the Python wrappers, against
tests/image_enhance_scene.py's references, bit for bit.  Runs on the CPU emulator as well (ORBX_TEST_EMULATOR=1)."""
import ctypes as C
import os

import numpy as np
import pytest

import image_enhance_scene as S

pytestmark = pytest.mark.gpu
BAD, STALE = -2, -9   # ORBX_E_BAD_ARG, ORBX_E_STALE
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))
# (source offset, source row slack, destination offset, destination row slack): both blocks start on a dword, so the offsets 0 .. 3 are the rows'
# alignments; slack 0 mod 4 keeps every row at the offset's alignment (the dword paths where it is 0), odd slack walks through all four
LAYOUTS = [(0, 4, 0, 8), (1, 3, 3, 5), (2, 5, 1, 4), (3, 8, 2, 7)]
GUARD = 13   # bytes before the first and after the last frame of a destination block, and whatever the strides leave between rows and frames


def _extractor(nf=500):
    import orb_slam3_amd as osa
    return osa.ORBextractor(nf, 1.2, 8, 20, 7)


@pytest.fixture(scope="module")
def ex():
    return _extractor()


class Block:
    """n images of `row_bytes` x h bytes inside a block of random bytes at `off` (row stride row_bytes + slack, 5 bytes between the frames), on the
    device."""

    def __init__(self, n, row_bytes, h, off, slack, seed, frames=None):
        import torch
        self.n, self.rb, self.h, self.rs = n, row_bytes, h, row_bytes + slack
        self.fs = self.rs * h + 5
        self.off = GUARD + 3 + off   # GUARD + 3 = 16: the offset is the alignment
        self.host = np.random.default_rng(seed).integers(0, 256, self.off + n * self.fs + GUARD, dtype=np.uint8)
        self.inside = np.zeros(self.host.shape, bool)
        for f in range(n):
            np.lib.stride_tricks.as_strided(self.inside[self.off + f * self.fs:], (h, row_bytes), (self.rs, 1))[:] = True
            if frames is not None:
                np.lib.stride_tricks.as_strided(self.host[self.off + f * self.fs:], (h, row_bytes), (self.rs, 1))[:] = frames[f].reshape(h, row_bytes)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 4 == 0
        self.ptr = self.dev.data_ptr() + self.off

    def read(self):
        """(the images [n, h, row_bytes], whether every byte outside them kept its value)"""
        out = self.dev.cpu().numpy()
        got = np.stack([np.lib.stride_tricks.as_strided(out[self.off + f * self.fs:], (self.h, self.rb), (self.rs, 1)).copy() for f in range(self.n)])
        return got, np.array_equal(out[~self.inside], self.host[~self.inside])

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


# ---- (1) gray ----
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("w", S.GRAY_WIDTHS)
def test_gray_every_code_and_alignment(ex, w, n):
    """The four colour codes on the designed pixels (sums on the .5 tie and next to it, saturated pixels, alpha 255 and random) at every source and
    destination alignment, strides above the rows: every frame equals the reference, every byte outside the destination rectangles keeps its value."""
    for channels, rgb in S.CODES:
        src = S.gray_frames(n, w, channels)
        want = S.reference_gray(src, rgb)
        for s_off, s_slack, d_off, d_slack in LAYOUTS:
            s, d = Block(n, w * channels, S.GRAY_H, s_off, s_slack, 1, src), Block(n, w, S.GRAY_H, d_off, d_slack, 2)
            ex.gray_batch(s.ptr, n, w, S.GRAY_H, channels, rgb, s.rs, s.fs, d.ptr, d.rs, d.fs)
            ex.sync()
            got, untouched = d.read()
            assert np.array_equal(got, want), (channels, rgb, s_off, d_off, np.argwhere(got != want)[:4].tolist())
            assert untouched and s.unchanged(), (channels, rgb, s_off, d_off)


def test_gray_one_buffer_four_codes(ex):
    """One buffer read under all four codes gives four different images, each the reference's."""
    buf = np.random.default_rng(5).integers(0, 256, (1, S.GRAY_H, 12 * 16), dtype=np.uint8)
    buf[..., 3::4] = 255
    outs = []
    for channels, rgb in S.CODES:
        w = 12 * 16 // channels
        s, d = Block(1, 12 * 16, S.GRAY_H, 0, 0, 1, buf), Block(1, w, S.GRAY_H, 0, 0, 2)
        ex.gray_batch(s.ptr, 1, w, S.GRAY_H, channels, rgb, s.rs, s.fs, d.ptr, d.rs, d.fs)
        ex.sync()
        got, untouched = d.read()
        assert np.array_equal(got[0], S.reference_gray(buf[0].reshape(S.GRAY_H, w, channels), rgb)) and untouched
        outs.append(got[0][:, :48])
    assert all(not np.array_equal(outs[i], outs[j]) for i in range(4) for j in range(i + 1, 4))


# ---- (2) resize ----
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("case", list(S.RESIZE_CASES))
def test_resize_every_class_and_alignment(ex, case, n):
    sw, sh, dw, dh = S.RESIZE_CASES[case]
    src = S.resize_frames(n, sw, sh)
    want = np.stack([S.reference_resize(f, dw, dh) for f in src])
    for s_off, s_slack, d_off, d_slack in LAYOUTS:
        s, d = Block(n, sw, sh, s_off, s_slack, 1, src), Block(n, dw, dh, d_off, d_slack, 2)
        ex.resize_batch(s.ptr, n, sw, sh, s.rs, s.fs, d.ptr, dw, dh, d.rs, d.fs)
        ex.sync()
        got, untouched = d.read()
        assert np.array_equal(got, want), (case, s_off, d_off, np.argwhere(got != want)[:4].tolist())
        assert untouched and s.unchanged(), (case, s_off, d_off)


def test_resize_more_size_pairs_than_table_slots():
    """Six size pairs in turn, twice, on one extractor with no wait in between: the tables of a size pair are found again or rebuilt, never mixed up."""
    e = _extractor()
    names = ["enlarge", "reduce_752_like", "half_in_x_only", "reduce_non_integer", "to_width_3", "half_in_y_only"]
    runs = []
    for name in names + names:
        sw, sh, dw, dh = S.RESIZE_CASES[name]
        src = S.resize_frames(2, sw, sh)
        s, d = Block(2, sw, sh, 1, 3, 1, src), Block(2, dw, dh, 2, 5, 2)
        e.resize_batch(s.ptr, 2, sw, sh, s.rs, s.fs, d.ptr, dw, dh, d.rs, d.fs)
        runs.append((name, src, s, d))
    e.sync()
    for name, src, s, d in runs:
        sw, sh, dw, dh = S.RESIZE_CASES[name]
        got, untouched = d.read()
        assert np.array_equal(got, np.stack([S.reference_resize(f, dw, dh) for f in src])) and untouched, name


# ---- (3) CLAHE ----
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("case", list(S.CLAHE_CASES))
def test_clahe_every_class_in_and_out_of_place(ex, case, n):
    """Every case of the scene module (the four divisibility classes at 8 x 8, the grids 1 x 1, 2 x 3 and 3 x 8, no clipping, a high limit) out of
    place at every alignment and in place: the reference's bytes, the guard bands and (out of place) the source untouched."""
    import orb_slam3_amd as osa
    w, h, tiles_x, tiles_y, clip_limit = S.CLAHE_CASES[case]
    src, want, _ = S.clahe_case(case, n)
    clahe = osa.DeviceClahe(clip_limit, (tiles_x, tiles_y))
    for s_off, s_slack, d_off, d_slack in LAYOUTS:
        s, d = Block(n, w, h, s_off, s_slack, 1, src), Block(n, w, h, d_off, d_slack, 2)
        clahe.apply_batch(ex, s.ptr, n, w, h, s.rs, s.fs, d.ptr, d.rs, d.fs)
        ex.sync()
        got, untouched = d.read()
        assert np.array_equal(got, want), (case, s_off, d_off, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert untouched and s.unchanged(), (case, s_off, d_off)
        clahe.apply_batch(ex, s.ptr, n, w, h, s.rs, s.fs, s.ptr, s.rs, s.fs)   # apply(im, im)
        ex.sync()
        got, untouched = s.read()
        assert np.array_equal(got, want) and untouched, (case, s_off, "in place")


def test_one_clahe_two_extractors(ex):
    """One object, two extractors in turn with a wait in between (the documented rule), a larger batch after a smaller one (the tables grow)."""
    import orb_slam3_amd as osa
    clahe, other = osa.DeviceClahe(3.0, (8, 8)), _extractor()
    for e, n in ((ex, 1), (other, 3), (ex, 5)):
        src, want, _ = S.clahe_case("neither_8x8", n)
        s, d = Block(n, 61, 45, 1, 3, 1, src), Block(n, 61, 45, 2, 5, 2)
        clahe.apply_batch(e, s.ptr, n, 61, 45, s.rs, s.fs, d.ptr, d.rs, d.fs)
        e.sync()
        got, untouched = d.read()
        assert np.array_equal(got, want) and untouched, n


# ---- (4) the chain in front of the extractor ----
_CHAIN = {}


def _chain_reference(canvas, B, w, h):
    """B colour frames (BGR) of (w + w // 3) x (h + h // 3), and the reference's gray -> resize to w x h -> CLAHE 3.0 / 8 x 8 of them; what an extractor
    gives for those prepared frames uploaded the ordinary way: computed once."""
    if (B, w, h) not in _CHAIN:
        import torch
        from orb_slam3_amd import synth
        rw, rh = w + w // 3, h + h // 3
        base = np.stack([synth.frame_from_canvas(canvas, 3 * t, rw, rh, 900 + t) for t in range(B)])
        raw = np.stack([base, 255 - base // 2, np.roll(base, 1, axis=2)], axis=-1)   # B, G, R
        gray = S.reference_gray(raw, False)
        small = np.stack([S.reference_resize(g, w, h) for g in gray])
        want = np.stack([S.reference_clahe(f, 3.0, 8, 8) for f in small])
        e = _extractor()
        d = torch.from_numpy(want.copy()).cuda()
        e.extract_batch_device(d.data_ptr(), B, w, h, w, w * h, (0, 0))
        outs = [e.download(f) for f in range(B)]
        e.sync()
        _CHAIN[(B, w, h)] = dict(raw=raw, want=want, outs=outs)
    return _CHAIN[(B, w, h)]


def check_chain_then_extract(canvas, w, h, B, in_place):
    """gray_batch, resize_batch, DeviceClahe.apply_batch (in place) and extract_batch_device with nothing between them == the reference-prepared frames
    extracted the ordinary way: key points, descriptors, and afterwards the prepared bytes themselves.  in_place: the batch must have read level 0 from
    the prepared frames themselves -- only such a batch has no level 0 after orbx_sync."""
    import torch
    import orb_slam3_amd as osa
    R = _chain_reference(canvas, B, w, h)
    rw, rh = w + w // 3, h + h // 3
    e, clahe = _extractor(), osa.DeviceClahe(3.0, (8, 8))
    d_raw = torch.from_numpy(R["raw"].copy()).cuda()
    d_gray = torch.zeros((B, rh, rw), dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # the buffers are complete; from here on only the extractor's stream orders anything
    e.gray_batch(d_raw.data_ptr(), B, rw, rh, 3, False, 3 * rw, 3 * rw * rh, d_gray.data_ptr(), rw, rw * rh)
    e.resize_batch(d_gray.data_ptr(), B, rw, rh, rw, rw * rh, d_dst.data_ptr(), w, h, w, w * h)
    clahe.apply_batch(e, d_dst.data_ptr(), B, w, h, w, w * h, d_dst.data_ptr(), w, w * h)
    e.extract_batch_device(d_dst.data_ptr(), B, w, h, w, w * h, (0, 0))
    total = 0
    for f in range(B):
        mono, kps, desc = e.download(f)
        omono, okps, odesc = R["outs"][f]
        assert mono == omono and kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc), f
        total += len(kps)
    e.sync()
    assert np.array_equal(d_dst.cpu().numpy(), R["want"])
    if in_place:
        with pytest.raises(osa.OrbxError) as err:
            e.get_level(0, 0)
        assert err.value.status == STALE
    else:
        assert np.array_equal(e.get_level(0, B - 1)[19:19 + h, 19:19 + w], R["want"][B - 1])
    return total


def test_chain_then_extract_without_a_wait(canvas1):
    """320 x 240, 2 frames.  (At 320 x 240 no batch reads level 0 in place; the next test is the in-place route.)"""
    assert check_chain_then_extract(canvas1, 320, 240, 2, False) > 100 * 2


def test_chain_then_extract_in_place(canvas1, monkeypatch):
    """517 x 389, 48 frames: the extraction reads level 0 from the prepared frames in place, as tests/test_gpu_image_prep.py's in-place case does.  (On
    the CPU emulator, for its speed: 5 frames, the in-place route forced by ORBX_PYR_STREAM_MIN as there.)"""
    B = 48
    if EMULATOR:
        B = 5
        monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,20")
    assert check_chain_then_extract(canvas1, 517, 389, B, True) > 300 * B


# ---- (5) refusals ----
def test_refusals_change_nothing(ex):
    """Every refusal returns ORBX_E_BAD_ARG and leaves the destination as it was; the same objects work afterwards.  (An extractor on another device
    than the CLAHE object's needs two devices: checked where there are two.)"""
    import torch
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    L, vp = _lib.lib(), C.c_void_p
    n, w, h = 3, 61, 45
    src, want, _ = S.clahe_case("neither_8x8", n)
    clahe = osa.DeviceClahe(3.0, (8, 8))
    s, d = Block(n, w, h, 1, 3, 1, src), Block(n, w, h, 2, 5, 2)
    last_of = lambda b, row_bytes: (b.n - 1) * b.fs + (b.h - 1) * b.rs + row_bytes   # noqa: E731  the span of a block's images

    ok = dict(c=clahe._h, ex=ex._h, src=vp(s.ptr), n=n, w=w, h=h, s_rs=s.rs, s_fs=s.fs, dst=vp(d.ptr), d_rs=d.rs, d_fs=d.fs)
    call = lambda **kw: L.orbx_clahe_batch_device(*[kw.get(k, v) for k, v in ok.items()])   # noqa: E731
    refused = dict(null_object=call(c=None), null_extractor=call(ex=None), null_src=call(src=None), null_dst=call(dst=None), no_frames=call(n=0),
                   negative_frames=call(n=-1), zero_width=call(w=0), zero_height=call(h=0), src_stride=call(s_rs=w - 1), dst_stride=call(d_rs=w - 1),
                   dst_frames_overlap=call(d_fs=d.rs * (h - 1)), shifted_in_place=call(dst=vp(s.ptr + 1), d_rs=s.rs, d_fs=s.fs),
                   in_place_other_stride=call(dst=vp(s.ptr), d_rs=s.rs + 1, d_fs=s.fs + h),
                   dst_ends_in_src=call(dst=vp(s.ptr - last_of(d, w) + 1)), dst_starts_in_src=call(dst=vp(s.ptr + last_of(s, w) - 1)),
                   pad_as_wide_as_the_image=call(w=3, s_rs=s.rs, d_rs=d.rs), pad_as_high_as_the_image=call(h=4))
    if torch.cuda.device_count() > 1 and not EMULATOR:
        refused["other_device"] = call(ex=osa.ORBextractor(500, 1.2, 8, 20, 7, device=1)._h)
    hdl = vp()
    created = [L.orbx_clahe_create(0, 3.0, 0, 8, C.byref(hdl)), L.orbx_clahe_create(0, 3.0, 8, 65, C.byref(hdl)), L.orbx_clahe_create(0, 3.0, -1, 8, C.byref(hdl)),
               L.orbx_clahe_create(0, 3.0, 8, 8, None), L.orbx_clahe_create(0, float("nan"), 8, 8, C.byref(hdl))]
    assert created == [BAD] * len(created) and not hdl.value, created

    cs, gd = Block(n, 4 * w, h, 1, 3, 1), Block(n, w, h, 2, 5, 2)
    gok = dict(ex=ex._h, src=vp(cs.ptr), n=n, w=w, h=h, ch=4, rgb=1, s_rs=cs.rs, s_fs=cs.fs, dst=vp(gd.ptr), d_rs=gd.rs, d_fs=gd.fs)
    gray = lambda **kw: L.orbx_gray_batch_device(*[kw.get(k, v) for k, v in gok.items()])   # noqa: E731
    refused.update(gray_null_extractor=gray(ex=None), gray_null_src=gray(src=None), gray_null_dst=gray(dst=None), gray_no_frames=gray(n=0),
                   gray_zero_width=gray(w=0), gray_zero_height=gray(h=0), gray_one_channel=gray(ch=1), gray_two_channels=gray(ch=2),
                   gray_five_channels=gray(ch=5), gray_src_stride=gray(s_rs=4 * w - 1), gray_src_stride_of_three=gray(s_rs=3 * w),
                   gray_dst_stride=gray(d_rs=w - 1), gray_dst_frames_overlap=gray(d_fs=gd.rs * (h - 1)), gray_in_place=gray(dst=vp(cs.ptr)),
                   gray_dst_ends_in_src=gray(dst=vp(cs.ptr - last_of(gd, w) + 1)), gray_dst_starts_in_src=gray(dst=vp(cs.ptr + last_of(cs, 4 * w) - 1)))

    dw, dh = 40, 31
    rd = Block(n, dw, dh, 3, 5, 2)
    rok = dict(ex=ex._h, src=vp(s.ptr), n=n, sw=w, sh=h, s_rs=s.rs, s_fs=s.fs, dst=vp(rd.ptr), dw=dw, dh=dh, d_rs=rd.rs, d_fs=rd.fs)
    resize = lambda **kw: L.orbx_resize_batch_device(*[kw.get(k, v) for k, v in rok.items()])   # noqa: E731
    refused.update(resize_null_extractor=resize(ex=None), resize_null_src=resize(src=None), resize_null_dst=resize(dst=None), resize_no_frames=resize(n=0),
                   resize_zero_src_width=resize(sw=0), resize_zero_src_height=resize(sh=0), resize_zero_dst_width=resize(dw=0),
                   resize_zero_dst_height=resize(dh=-3), resize_src_stride=resize(s_rs=w - 1), resize_dst_stride=resize(d_rs=dw - 1),
                   resize_dst_frames_overlap=resize(d_fs=rd.rs * (dh - 1)), resize_in_place=resize(dst=vp(s.ptr)),
                   resize_dst_ends_in_src=resize(dst=vp(s.ptr - last_of(rd, dw) + 1)), resize_dst_starts_in_src=resize(dst=vp(s.ptr + last_of(s, w) - 1)))
    assert all(v == BAD for v in refused.values()), {k: v for k, v in refused.items() if v != BAD}
    ex.sync()
    assert s.unchanged() and d.unchanged() and cs.unchanged() and gd.unchanged() and rd.unchanged()
    # the same objects afterwards
    clahe.apply_batch(ex, s.ptr, n, w, h, s.rs, s.fs, d.ptr, d.rs, d.fs)
    ex.sync()
    got, untouched = d.read()
    assert np.array_equal(got, want) and untouched
    with pytest.raises(osa.OrbxError) as err:
        ex.gray_batch(cs.ptr, n, w, h, 2, True, cs.rs, cs.fs, gd.ptr, gd.rs, gd.fs)
    assert err.value.status == BAD
