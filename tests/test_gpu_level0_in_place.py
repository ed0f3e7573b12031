"""Level 0 read in place (batches of ps_min_frames frames or more: k_pyr_stream, k_fast_strip, the FAST list pass and k_describe_fused take the frames
the extraction was called with, with the caller's pointer, row stride and frame stride; the padded level 0 is written on request only) against the CPU
oracle, bit for bit:

* device frames that are a strided, offset, gapped view of a larger allocation, with zeros and with random bytes around them;
* the rules after which the frames count as handed back to the caller (orbx_sync, orbx_download_wait): which requests are refused with
  ORBX_E_STALE on the orbx_extract_batch_device route, that nothing is refused on the orbx_extract_batch_host route (its frames lie in the library's
  own upload slab), and the first orbx_stereo_batch_device after in-place batches;
* orbx_get_level_device, whose pointer must be complete when it is returned.

ORBX_PYR_STREAM_MIN = "1,<workgroups>" forces the in-place form onto batches of three and five frames; it is read when a geometry is configured, so every
extractor here is created after the variable is set.  The check_* functions take no fixtures: tests/test_simt_emulation.py runs two of them on the CPU
emulator."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STALE = -9
EMULATOR = bool(os.environ.get("ORBX_TEST_EMULATOR"))
W, H, NF = 517, 389, 700
BF, BASELINE = float(np.float32(0.53716 * 718.856)), float(np.float32(0.53716))

_REF = {}   # the oracle's results per frame: computed once, read-only, shared by every test of this file


def _frozen(a):
    a.setflags(write=False)
    return a


def _ref_of(key, img, nf):
    """Everything the oracle says about `img`: keypoints / descriptors for both lapping areas used here and every stage of the extraction."""
    if key not in _REF:
        from oracle import oracle_binding as ob
        oex = ob.OracleExtractor(nf, 1.2, 8, 20, 7, flags=ob.FLAG_DESC_FMA)
        r = SimpleNamespace(img=_frozen(img))
        r.out = {(0, 0): oex.extract(img, lap=(0, 0)), (0, 1000): oex.extract(img, lap=(0, 1000))}   # the stages below do not depend on the lapping area
        r.padded = [_frozen(oex.level_padded(l)) for l in range(8)]
        r.blurred = [_frozen(oex.level_blurred(l)) for l in range(8)]
        r.reflected = [_frozen(np.pad(b, 18, mode="reflect")) for b in r.blurred]   # BORDER_REFLECT_101 extension of the blurred level
        r.cands = [_frozen(oex.level_candidates(l)) for l in range(8)]
        r.scale = _frozen(oex.tables()["scale"])
        r.inv_scale = _frozen(oex.tables()["inv_scale"])
        _REF[key] = r
    return _REF[key]


def _ref(canvas, t, w=W, h=H, nf=NF):
    from orb_slam3_amd import synth
    key = ("mono", t, w, h, nf)
    return _REF[key] if key in _REF else _ref_of(key, synth.frame_from_canvas(canvas, t, w, h, 3000 + t), nf)


def _refs(canvas, ts, w=W, h=H, nf=NF):
    refs = [_ref(canvas, t, w, h, nf) for t in ts]
    return refs, np.stack([r.img for r in refs])


def _stereo_refs(canvas, ts):
    from orb_slam3_amd import synth
    out = []
    for t in ts:
        if ("left", t) not in _REF:
            l, r = synth.make_stereo_pair(1, t, W, H, canvas)
            _ref_of(("left", t), l, NF), _ref_of(("right", t), r, NF)
        out.append((_REF[("left", t)], _REF[("right", t)]))
    return out


def _extractor(nf=NF):
    import orb_slam3_amd as osa
    return osa.ORBextractor(nf, 1.2, 8, 20, 7)


def _same_output(got, ref, lap):
    mono, kps, desc = got
    omono, okps, odesc = ref.out[lap]
    return mono == omono and kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)


def _same_candidates(ex, ref, f):
    for l in range(8):
        got, want = ex.debug_candidates(l, f), ref.cands[l]
        if len(got) != len(want) or any(not np.array_equal(got[k], want[k]) for k in ("x", "y", "response")):
            return False
    return True


def _check_patches(patches, ref, lap):
    """The 37 x 37 blurred pixels k_describe_fused held in LDS around every keypoint == the oracle's GaussianBlur of the keypoint's level (its
    reflection where the patch leaves the level); returns how many keypoints' raw 43 x 43 windows left their level."""
    kps = ref.out[lap][1]
    assert len(patches) == len(kps) > 600
    n_border = 0
    for k in range(len(kps)):
        l = int(kps["octave"][k])
        x, y = int(round(float(kps["x"][k]) / float(ref.scale[l]))), int(round(float(kps["y"][k]) / float(ref.scale[l])))
        want = ref.reflected[l][y:y + 37, x:x + 37]
        assert np.array_equal(patches[k], want), (k, l, x, y, int((patches[k] != want).sum()))
        lw, lh = ref.reflected[l].shape[1] - 36, ref.reflected[l].shape[0] - 36
        n_border += (x < 21 or y < 21 or x > lw - 22 or y > lh - 22)
    return n_border


def _refused(call):
    """`call` fails with ORBX_E_STALE and says why."""
    import orb_slam3_amd as osa
    from orb_slam3_amd import _lib
    with pytest.raises(osa.OrbxError) as e:
        call()
    assert e.value.status == STALE == _lib.ORBX_E_STALE, e.value
    assert b"released" in _lib.lib().orbx_last_error()


def _pinned_outputs(ex, B):
    import torch
    cap = ex.output_capacity(W, H)
    pin = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()
    return dict(kps=pin((B, cap, 28), torch.uint8), desc=pin((B, cap, 32), torch.uint8), cnt=pin(B, torch.int32), mono=pin(B, torch.int32))


def _download_async(ex, hs):
    ex.download_async(hs["kps"].data_ptr(), hs["desc"].data_ptr(), hs["cnt"].data_ptr(), hs["mono"].data_ptr(), 0, 0)


def _same_downloaded(hs, refs, lap):
    for f, ref in enumerate(refs):
        n = int(hs["cnt"][f])
        omono, okps, odesc = ref.out[lap]
        if n != len(okps) or int(hs["mono"][f]) != omono or hs["kps"][f, :n].numpy().tobytes() != okps.tobytes() or not np.array_equal(hs["desc"][f, :n].numpy(), odesc):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# A. strided, offset, gapped device frames
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_strided_frames(canvas, w, h, nf, B, in_place, padding):
    """orbx_extract_batch_device on the view big[:, 10:10+h, 21:21+w] of one (B, h+20, w+59) allocation: the row stride is odd, the base pointer lies 21
    bytes into a row, 20 rows separate the frames and 10 follow the last one (a read a little past a row or a frame stays inside the allocation: nothing
    here relies on a fault).  `padding`: the bytes around the frames are zero or random -- both must give the oracle's results, so a kernel that lets a
    byte from outside a frame into a result (a wrong stride, a reflection computed with the stride in place of the width) fails one of them.
    in_place: ORBX_PYR_STREAM_MIN is set so that k_pyr_stream, k_fast_strip, the FAST list pass and both forms of k_describe_fused read that view; otherwise
    the per-level chain runs and k_pyr_base is the kernel that gets the strides.  The materialised level 0 goes through k_pyr_base in both."""
    import torch
    refs, frames = _refs(canvas, range(B), w, h, nf)
    rs, fs = w + 59, (h + 20) * (w + 59)
    big = np.zeros((B, h + 20, rs), np.uint8) if padding == "zero" else np.random.default_rng(5).integers(0, 256, (B, h + 20, rs), dtype=np.uint8)
    big[:, 10:10 + h, 21:21 + w] = frames
    d = torch.from_numpy(big).cuda()
    base = d.data_ptr() + 10 * rs + 21
    ex = _extractor(nf)
    for lap in ((0, 0), (0, 1000)):
        ex.extract_batch_device(base, B, w, h, rs, fs, lap)
        for f in range(B):
            assert _same_output(ex.download(f), refs[f], lap), (lap, f)
    lap = (0, 1000)
    for f in (0, B - 1):   # level 0 is still unwritten (in place): the fused patches of both frames come from the strided view
        assert _same_candidates(ex, refs[f], f), f
        for l in range(1, 8):
            assert np.array_equal(ex.get_level(l, f), refs[f].padded[l]), (f, l)
        if in_place:
            assert _check_patches(ex.debug_fused_patches(f), refs[f], lap) > 0, f   # windows that leave level 0: the staged form's reflection with row_stride
    for f in (0, B - 1):
        assert np.array_equal(ex.get_level(0, f), refs[f].padded[0]), f   # k_pyr_base with the caller's strides
    # was level 0 of such a batch really read in place?  Then, and only then, orbx_sync hands the frames back and level 0 can no longer be had
    ex.extract_batch_device(base, B, w, h, rs, fs, lap)
    ex.sync()
    if in_place:
        _refused(lambda: ex.get_level(0, 0))
    else:
        assert np.array_equal(ex.get_level(0, B - 1), refs[B - 1].padded[0])
    assert np.array_equal(ex.get_level(3, B - 1), refs[B - 1].padded[3])
    assert _same_output(ex.download(B - 1), refs[B - 1], lap)
    del d
    return sum(len(r.out[lap][1]) for r in refs)


@pytest.mark.parametrize("padding", ["zero", "random"])
@pytest.mark.parametrize("w,h,nf,B,wgs", [(W, H, NF, 3, None), (W, H, NF, 3, 3), (W, H, NF, 5, 20), (752, 480, 1000, 3, 3)],
                         ids=["chain", "in-place-1-band", "in-place-4-bands", "in-place-752x480"])
def test_strided_offset_gapped_device_frames(canvas1, monkeypatch, w, h, nf, B, wgs, padding):
    """check_strided_frames for the per-level chain (k_pyr_base takes the strides) and in place with one and four bands per frame; 752 x 480: the width
    is a multiple of 16, the row stride is not."""
    if wgs is None:
        monkeypatch.delenv("ORBX_PYR_STREAM_MIN", raising=False)
    else:
        monkeypatch.setenv("ORBX_PYR_STREAM_MIN", f"1,{wgs}")
    assert check_strided_frames(canvas1, w, h, nf, B, wgs is not None, padding) > 650 * B


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# B. when the frames of an in-place batch are the caller's again
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_device_route_level0_is_refused_after_sync(canvas1, monkeypatch):
    """orbx_extract_batch_device, in place: before orbx_sync level 0 can be had (and, once written, also after it); after orbx_sync on a batch whose
    level 0 was never written, orbx_get_level(0), orbx_get_level_device(0), orbx_debug_level_blurred, orbx_debug_fused_patches (which would run
    k_describe_fused on the frames again) and orbx_stereo_batch_device are refused with ORBX_E_STALE, while everything that does not need the frames
    still equals the oracle.  The frames stay alive and unmodified throughout: no refusal is tested by reading freed or overwritten memory."""
    import torch
    monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,3")
    B, lap = 3, (0, 1000)
    refs, frames = _refs(canvas1, range(B))
    d = torch.from_numpy(frames).cuda()
    ex = _extractor()
    ex.extract_batch_device(d.data_ptr(), B, W, H, W, W * H, lap)
    assert np.array_equal(ex.get_level(0, 1), refs[1].padded[0])
    ex.sync()
    assert np.array_equal(ex.get_level(0, 2), refs[2].padded[0])   # written before the sync: it is in the slab
    assert np.array_equal(ex.debug_blurred(0, 2), refs[2].blurred[0])

    ex.extract_batch_device(d.data_ptr(), B, W, H, W, W * H, lap)
    ex.sync()
    _refused(lambda: ex.get_level(0, 0))
    _refused(lambda: ex.get_level_device(0, B - 1))
    _refused(lambda: ex.debug_blurred(0, 0))
    _refused(lambda: ex.debug_blurred(3, 1))   # the blurred slab is filled for all levels at once, level 0 included
    _refused(lambda: ex.debug_fused_patches(0))
    _refused(lambda: ex.get_level(0, 0))       # a refusal changes nothing
    for f in range(B):
        assert _same_output(ex.download(f), refs[f], lap), f
        assert _same_candidates(ex, refs[f], f), f
        for l in range(1, 8):
            assert np.array_equal(ex.get_level(l, f), refs[f].padded[l]), (f, l)
        p, pitch = ex.get_level_device(5, f)
        assert p and pitch >= ex.level_size(5)[0] + 38

    exl, exr = _extractor(), _extractor()
    for e in (exl, exr):
        e.extract_batch_device(d.data_ptr(), B, W, H, W, W * H, (0, 0))
        e.sync()
    _refused(lambda: exl.stereo_batch_device(exr, BF, BASELINE))   # the SAD stage needs both padded levels 0
    del d


@pytest.mark.parametrize("waits", [1, 2])
def test_device_route_download_wait_releases_only_a_later_download(canvas1, monkeypatch, waits):
    """batch A, download A, batch B (in place), download B.  The first orbx_download_wait completes A's download, which was issued before B: B's frames
    are still the library's and its level 0 equals the oracle's.  The second completes B's: level 0 is refused, B's downloaded results are the
    oracle's."""
    import torch
    monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,3")
    B, lap = 3, (0, 1000)
    refs_a, frames_a = _refs(canvas1, range(B))
    refs_b, frames_b = _refs(canvas1, range(B, 2 * B))
    da, db = torch.from_numpy(frames_a).cuda(), torch.from_numpy(frames_b).cuda()
    ex = _extractor()
    hs_a, hs_b = _pinned_outputs(ex, B), _pinned_outputs(ex, B)
    ex.extract_batch_device(da.data_ptr(), B, W, H, W, W * H, lap)
    _download_async(ex, hs_a)
    ex.extract_batch_device(db.data_ptr(), B, W, H, W, W * H, lap)
    _download_async(ex, hs_b)
    ex.download_wait()
    assert _same_downloaded(hs_a, refs_a, lap)
    if waits == 1:
        for f in range(B):
            assert np.array_equal(ex.get_level(0, f), refs_b[f].padded[0]), f
        ex.download_wait()
    else:
        ex.download_wait()
        _refused(lambda: ex.get_level(0, 0))
        _refused(lambda: ex.debug_fused_patches(B - 1))
    assert _same_downloaded(hs_b, refs_b, lap)
    assert np.array_equal(ex.get_level(2, 1), refs_b[1].padded[2])
    del da, db


def check_host_route(canvas, how):
    """orbx_extract_batch_host, in place: the frames the kernels read lie in the library's upload slab, which is kept while the batch is the last one.
    After orbx_sync (`how` = "sync"; the caller's pinned frames are then overwritten with 0x5a, as include/orbx.h allows) or after a completed download
    (`how` = "download") level 0, the blurred level 0 and the fused patches can still be had and equal the oracle's; a second host batch on the same
    extractor equals the oracle too (the slab's events were not disturbed)."""
    import torch
    B, lap = 3, (0, 1000)
    refs, frames = _refs(canvas, range(B))
    refs2, frames2 = _refs(canvas, range(B, 2 * B))
    pinned, pinned2 = torch.from_numpy(frames.copy()).pin_memory(), torch.from_numpy(frames2.copy()).pin_memory()
    ex = _extractor()
    ex.extract_batch_host(pinned.data_ptr(), B, W, H, W, W * H, lap)
    if how == "sync":
        ex.sync()
        pinned.fill_(0x5a)
        for f in (0, B - 1):   # first: k_describe_fused once more on the slab, level 0 still unwritten
            assert _check_patches(ex.debug_fused_patches(f), refs[f], lap) > 0, f
    else:
        hs = _pinned_outputs(ex, B)
        _download_async(ex, hs)
        ex.download_wait()
        assert _same_downloaded(hs, refs, lap)
    for f in range(B):
        assert np.array_equal(ex.get_level(0, f), refs[f].padded[0]), f
    for f in (0, B - 1):
        assert np.array_equal(ex.debug_blurred(0, f), refs[f].blurred[0]), f
        assert _check_patches(ex.debug_fused_patches(f), refs[f], lap) > 0, f
        assert _same_output(ex.download(f), refs[f], lap), f
    ex.extract_batch_host(pinned2.data_ptr(), B, W, H, W, W * H, lap)
    for f in range(B):
        assert _same_output(ex.download(f), refs2[f], lap), f
    assert np.array_equal(ex.get_level(0, 1), refs2[1].padded[0])
    del pinned, pinned2
    return sum(len(r.out[lap][1]) for r in refs)


@pytest.mark.parametrize("how", ["sync", "download"])
def test_host_route_level0_survives_sync_and_download_wait(canvas1, monkeypatch, how):
    """check_host_route.  (Before the release rules told the two routes apart, orbx_get_level(0) returned ORBX_E_STALE, -9, here.)"""
    monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,3")
    assert check_host_route(canvas1, how) > 650 * 3


@pytest.mark.parametrize("route", ["device", "host"])
def test_first_stereo_call_after_in_place_batches(canvas1, oracle, monkeypatch, route):
    """The first orbx_stereo_batch_device on two extractors whose batches read level 0 in place materialises both padded levels 0 for the SAD stage
    (device route: before any orbx_sync; host route: also after one); mvuRight / mvDepth == the oracle's ComputeStereoMatches.  From then on both
    extractors alternate between two pyramid slabs and copy level 0: a second pair of batches and stereo call equals the oracle as well."""
    import torch
    monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,3")
    B = 3
    exl, exr = _extractor(), _extractor()
    for rep in range(2):
        pairs = _stereo_refs(canvas1, range(rep * B, rep * B + B))
        left, right = np.stack([p[0].img for p in pairs]), np.stack([p[1].img for p in pairs])
        if route == "device":
            tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            exl.extract_batch_device(tl.data_ptr(), B, W, H, W, W * H, (0, 0))
            exr.extract_batch_device(tr.data_ptr(), B, W, H, W, W * H, (0, 0))
        else:
            tl, tr = torch.from_numpy(left).pin_memory(), torch.from_numpy(right).pin_memory()
            exl.extract_batch_host(tl.data_ptr(), B, W, H, W, W * H, (0, 0))
            exr.extract_batch_host(tr.data_ptr(), B, W, H, W, W * H, (0, 0))
            exl.sync()
            exr.sync()
        exl.stereo_batch_device(exr, BF, BASELINE)
        for t, (rl, rr) in enumerate(pairs):
            nm, ur, depth = exl.stereo_download(t)
            (_, kl, dsl), (_, kr, dsr) = rl.out[(0, 0)], rr.out[(0, 0)]
            pyl = [np.ascontiguousarray(p[19:-19, 19:-19]) for p in rl.padded]
            pyr = [np.ascontiguousarray(p[19:-19, 19:-19]) for p in rr.padded]
            on, our, odepth, _, _ = oracle.compute_stereo_matches(kl, dsl, kr, dsr, rl.scale, rl.inv_scale, pyl, pyr, BF, BASELINE)
            assert nm == on and len(ur) == len(our), (rep, t, nm, on)
            assert ur.tobytes() == our.tobytes() and depth.tobytes() == odepth.tobytes(), (rep, t)
            assert nm > 50
            assert _same_output(exl.download(t), rl, (0, 0)) and _same_output(exr.download(t), rr, (0, 0)), (rep, t)
        exl.sync()
        del tl, tr


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# C. orbx_get_level_device
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _from_device(p, nbytes):
    """`nbytes` at device address `p`, copied with a plain hipMemcpy: it waits for none of the library's (non-blocking) streams."""
    if EMULATOR:   # device memory is host memory
        return np.frombuffer(C.string_at(p, nbytes), np.uint8)
    import torch  # noqa: F401  (the HIP runtime torch has loaded is the one liborbx uses)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(p), nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("in_place", [False, True], ids=["chain", "in-place"])
def test_get_level_device_points_at_the_complete_padded_level(canvas1, monkeypatch, in_place):
    """The (h + 38) x (w + 38) window at the pointer orbx_get_level_device returns, rows `pitch` bytes apart == the oracle's padded level ==
    orbx_get_level, all 8 levels of the first and the last frame.  After an in-place batch level 0 is asked for first and copied by the very next call,
    which waits for no stream of the library: the level must have been written, and the write finished, when the pointer came back.  (For every other
    level and batch the call is a pure getter: the chain batch is synchronised first.)  The copy ends with the window's last byte: the rest of that row
    may lie outside the pyramid slab."""
    import torch
    if in_place:
        monkeypatch.setenv("ORBX_PYR_STREAM_MIN", "1,3")
    else:
        monkeypatch.delenv("ORBX_PYR_STREAM_MIN", raising=False)
    B, lap = 3, (0, 1000)
    refs, frames = _refs(canvas1, range(B))
    d = torch.from_numpy(frames).cuda()
    ex = _extractor()
    ex.extract_batch_device(d.data_ptr(), B, W, H, W, W * H, lap)
    if not in_place:
        ex.sync()
    for f in (0, B - 1):
        for l in range(8):
            w, h = ex.level_size(l)
            p, pitch = ex.get_level_device(l, f)
            flat = _from_device(p, (h + 37) * pitch + w + 38)
            assert p and pitch >= w + 38, (f, l, pitch)
            got = np.lib.stride_tricks.as_strided(flat, (h + 38, w + 38), (pitch, 1))
            assert np.array_equal(got, refs[f].padded[l]), (f, l)
            assert np.array_equal(got, ex.get_level(l, f)), (f, l)
    for f in range(B):
        assert _same_output(ex.download(f), refs[f], lap), f
    # the in-place batch really was one: after orbx_sync its level 0 cannot be had
    ex.extract_batch_device(d.data_ptr(), B, W, H, W, W * H, lap)
    ex.sync()
    if in_place:
        _refused(lambda: ex.get_level_device(0, 0))
    else:
        assert ex.get_level_device(0, 0)[0]
    del d
