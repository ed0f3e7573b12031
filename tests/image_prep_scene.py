"""The reference and the designed inputs of the image-preparation calls (orbx_rectify_batch_device, orbx_rgbd_batch_device_u16): plain numpy integer
arithmetic in the order include/orbx.h restates cv::remap(src, dst, map1, map2, INTER_LINEAR) for 8-bit one-channel images and two CV_32FC1 maps,
BORDER_CONSTANT 0.  No device code runs here.  check_conditions() asserts, on the reference alone, that the designed map classes tell the
plausible wrong implementations from the right one."""
import numpy as np

f32 = np.float32
INT_MIN = -(1 << 31)

# the base shape: 3 frames, source 61 x 17, destination 67 x 13
SW, SH, DW, DH, FRAMES = 61, 17, 67, 13, 3
CLASSES = ("integer", "ties", "fractions_a", "fractions_b", "below_zero", "at_the_far_edge", "saturating", "not_finite", "distortion")


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the reference ----
def fixed(m, rounding="even", nan_as_zero=False):
    """cvRound(m * 32) per entry as int64: nearest, ties to even; INT_MIN for NaN, infinite and anything outside int.
    rounding="half_up" and nan_as_zero=True are the mutants of check_conditions()."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(m, f32) * f32(32)
    ok = (p >= f32(-2147483648.0)) & (p < f32(2147483648.0))   # NaN fails both
    s = np.full(p.shape, INT_MIN, np.int64)
    q = p[ok].astype(np.float64)
    s[ok] = (np.rint(q) if rounding == "even" else np.floor(q + 0.5)).astype(np.int64)
    if nan_as_zero:
        s[np.isnan(p)] = 0
    return s


def reference_remap(src, map_x, map_y, rounding="even", nan_as_zero=False, clamp=False):
    """src (h, w) uint8 -> (map shape) uint8.  clamp=True is a mutant: taps outside the image take the nearest pixel instead of 0."""
    h, w = src.shape
    sx, sy = fixed(map_x, rounding, nan_as_zero), fixed(map_y, rounding, nan_as_zero)
    a, b = sx & 31, sy & 31
    ix, iy = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)

    def tap(x, y):
        if clamp:
            return src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        v = np.zeros(x.shape, np.int64)
        v[inside] = src[y[inside], x[inside]]
        return v

    total = (tap(ix, iy) * ((32 - a) * (32 - b) * 32) + tap(ix + 1, iy) * (a * (32 - b) * 32) + tap(ix, iy + 1) * ((32 - a) * b * 32)
             + tap(ix + 1, iy + 1) * (a * b * 32))
    return ((total + 16384) >> 15).astype(np.uint8)


def float_bilinear(src, map_x, map_y):
    """A mutant: bilinear interpolation with float weights and one final rint (finite coordinates only)."""
    h, w = src.shape
    mx, my = np.asarray(map_x, np.float64), np.asarray(map_y, np.float64)
    x0, y0 = np.floor(mx).astype(np.int64), np.floor(my).astype(np.int64)
    fx, fy = mx - x0, my - y0

    def tap(x, y):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        v = np.zeros(x.shape, np.float64)
        v[inside] = src[y[inside], x[inside]]
        return v

    v = tap(x0, y0) * (1 - fx) * (1 - fy) + tap(x0 + 1, y0) * fx * (1 - fy) + tap(x0, y0 + 1) * (1 - fx) * fy + tap(x0 + 1, y0 + 1) * fx * fy
    return np.rint(v).astype(np.uint8)


# ---- the inputs ----
def sources(sw=SW, sh=SH, frames=FRAMES):
    """Values 1..255 only (a sample from inside the image can never pass for the border's 0): frame 0 random, frame 1 a 1 / 255 checker, the rest a
    ramp with a different step per frame."""
    rng = np.random.default_rng(61)
    yy, xx = np.mgrid[0:sh, 0:sw]
    out = [rng.integers(1, 256, (sh, sw), dtype=np.uint8), np.where((xx + yy) & 1, 255, 1).astype(np.uint8)]
    for f in range(2, frames):
        out.append((1 + (xx * (5 + f) + yy * (11 + 2 * f)) % 255).astype(np.uint8))
    return _frozen(np.stack(out[:frames]))


def _mix(dw, dh, sw, sh, special_x, special_y):
    """Maps whose top third has the special values on x and ordinary ones on y, the middle third the other way round, the rest both."""
    mx, my = np.zeros((dh, dw), f32), np.zeros((dh, dw), f32)
    for y in range(dh):
        for x in range(dw):
            p = y * dw + x
            ox, oy = f32((p * 7) % (sw - 1)) + f32((p * 5) % 32) / f32(32), f32((p * 3) % (sh - 1)) + f32((p * 11) % 32) / f32(32)
            third = 0 if y < (dh + 2) // 3 else 1 if y < (2 * dh + 2) // 3 else 2
            mx[y, x] = special_x[p % len(special_x)] if third != 1 else ox
            my[y, x] = special_y[(p // 2) % len(special_y)] if third != 0 else oy
    return mx, my


def make_maps(cls, dw=DW, dh=DH, sw=SW, sh=SH):
    """(map_x, map_y), float32 (dh, dw), of one designed class for a source of sw x sh."""
    yy, xx = np.mgrid[0:dh, 0:dw]
    p = yy * dw + xx
    if cls == "integer":
        mx, my = ((xx * 7 + yy * 3) % sw).astype(f32), ((yy * 5 + xx) % sh).astype(f32)
    elif cls == "ties":   # k + (2j + 1) / 64: times 32 it ends in .5; all 32 j on each axis, over even and odd k
        jx, kx = xx % 32, 4 + xx // 32 + yy % 2
        jy, ky = (xx + 5 * yy) % 32, 3 + yy % 2 + xx // 32
        mx, my = (kx + (2 * jx + 1) / 64.0).astype(f32), (ky + (2 * jy + 1) / 64.0).astype(f32)
    elif cls in ("fractions_a", "fractions_b"):   # all 32 x 32 (a, b) over the two maps (dw * dh pairs each), meant for the checker frame
        q = p + (dw * dh if cls == "fractions_b" else 0)
        mx, my = (2 + (q // 7) % (sw - 4) + (q % 32) / 32.0).astype(f32), (1 + (q // 5) % (sh - 3) + ((q // 32) % 32) / 32.0).astype(f32)
    elif cls == "below_zero":
        s = [f32(-1), f32(-1) - f32(1) / f32(64), -f32(1) / f32(64), f32(-0.5), f32(-1.25), f32(-1.96875), f32(-1.5)]
        mx, my = _mix(dw, dh, sw, sh, s, s)
    elif cls == "at_the_far_edge":
        sx = [f32(sw - 1), f32(sw - 1) + f32(1) / f32(32), f32(sw) - f32(1) / f32(64), f32(sw), f32(sw - 1) + f32(0.5)]
        sy = [f32(sh - 1), f32(sh - 1) + f32(1) / f32(32), f32(sh) - f32(1) / f32(64), f32(sh), f32(sh - 1) + f32(0.5)]
        mx, my = _mix(dw, dh, sw, sh, sx, sy)
    elif cls == "saturating":   # +-40000: the short saturates; +-2^26: the product leaves int (-2^31 itself is INT_MIN)
        s = [f32(40000), f32(-40000), f32(2.0 ** 26), f32(-(2.0 ** 26)), f32(32767), f32(-32768), f32(1023.96875), f32(2.0 ** 26 - 8)]
        mx, my = _mix(dw, dh, sw, sh, s, s)
    elif cls == "not_finite":
        s = [f32(1e12), f32(-1e12), f32(np.inf), f32(-np.inf), f32(np.nan), f32(3e38), f32(-3e38)]
        mx, my = _mix(dw, dh, sw, sh, s, s)
    elif cls == "distortion":   # a radial-tangential field between the destination's and the source's pinhole, strong enough to leave the source at the corners
        f, k1, k2, p1, p2 = 0.62 * dw, -0.28, 0.07, 0.004, -0.003
        xn, yn = (xx - (dw - 1) / 2.0) / f, (yy - (dh - 1) / 2.0) / f
        r2 = xn * xn + yn * yn
        rad = 1 + k1 * r2 + k2 * r2 * r2
        xd, yd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn), yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
        fs = 0.85 * sw
        mx, my = (fs * xd + (sw - 1) / 2.0 + 0.3).astype(f32), (fs * yd + (sh - 1) / 2.0 - 0.2).astype(f32)
    else:
        raise KeyError(cls)
    return _frozen(np.ascontiguousarray(mx, f32)), _frozen(np.ascontiguousarray(my, f32))


def smooth_maps(dw, dh, sw, sh, strength=1.0):
    """The `distortion` field for any pair of sizes, weak enough to stay inside the source except near the corners: the end-to-end tests' maps."""
    yy, xx = np.mgrid[0:dh, 0:dw]
    f, k1, k2, p1, p2 = 0.9 * dw, -0.12 * strength, 0.02 * strength, 0.001 * strength, -0.0008 * strength
    xn, yn = (xx - (dw - 1) / 2.0) / f, (yy - (dh - 1) / 2.0) / f
    r2 = xn * xn + yn * yn
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd, yd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn), yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    fs = 0.9 * dw * 1.04
    return _frozen((fs * xd + (sw - 1) / 2.0).astype(f32)), _frozen((fs * yd + (sh - 1) / 2.0).astype(f32))


_CACHE = {}


def base_case(cls):
    """(map_x, map_y, want[FRAMES, DH, DW]) of a class on the base shape: computed once, read-only."""
    if cls not in _CACHE:
        mx, my = make_maps(cls)
        _CACHE[cls] = (mx, my, _frozen(np.stack([reference_remap(s, mx, my) for s in sources()])))
    return _CACHE[cls]


def check_conditions():
    """What the classes are for, asserted on the reference alone; returns the differing-pixel counts of the mutants."""
    src = sources()
    counts = {}
    # the weight table's 32767: ((32767 p + q + 16384) >> 15) == p for all bytes p, q
    pp, qq = np.mgrid[0:256, 0:256]
    assert np.array_equal((32767 * pp + qq + 16384) >> 15, pp)
    assert src.min() >= 1
    mx, my, want = base_case("integer")
    assert np.array_equal(want[0], src[0][my.astype(int), mx.astype(int)])
    # ties: all 32 odd numerators on both axes, even and odd integer parts; rounding half up differs
    mx, my, want = base_case("ties")
    for m in (mx, my):
        t = m.astype(np.float64) * 64
        assert np.array_equal(t, np.rint(t)) and set((t.astype(int) % 64).ravel()) == set(range(1, 64, 2))
        assert {0, 1} == set((np.floor(m).astype(int) % 2).ravel())
    counts["half_up"] = int((reference_remap(src[0], mx, my, rounding="half_up") != want[0]).sum())
    assert counts["half_up"] > DW * DH // 4
    # all 32 x 32 (a, b) over the two fraction maps
    pairs = set()
    for cls in ("fractions_a", "fractions_b"):
        mx, my, _ = base_case(cls)
        pairs |= set(zip((fixed(mx) & 31).ravel().tolist(), (fixed(my) & 31).ravel().tolist()))
        assert mx.min() >= 0 and mx.max() < SW - 1 and my.min() >= 0 and my.max() < SH - 1
    assert len(pairs) == 1024
    # float interpolation with one final rint differs on the realistic field
    mx, my, want = base_case("distortion")
    counts["float_bilinear"] = int((float_bilinear(src[0], mx, my) != want[0]).sum())
    assert counts["float_bilinear"] > DW * DH // 4
    assert (want[0] == 0).any() and (want[0] != 0).sum() > DW * DH // 2   # the corners leave the source, most of it does not
    # NaN converted to 0 reads source column / row 0 where the reference reads nothing
    mx, my, want = base_case("not_finite")
    nan = np.isnan(mx) | np.isnan(my)
    got = reference_remap(src[0], mx, my, nan_as_zero=True)
    counts["nan_as_zero"] = int((got != want[0]).sum())
    assert nan.sum() > 20 and counts["nan_as_zero"] > 0 and (want[0][nan] == 0).all() and (got[nan] != 0).any()
    special = ~np.isfinite(mx) | ~np.isfinite(my) | (np.abs(mx) > 1e9) | (np.abs(my) > 1e9)
    assert special.all() and (want[0] == 0).all()   # every pixel has such a coordinate on one axis at least
    # clamped coordinates instead of zeroed taps
    for cls in ("below_zero", "at_the_far_edge"):
        mx, my, want = base_case(cls)
        counts["clamp_" + cls] = int((reference_remap(src[0], mx, my, clamp=True) != want[0]).sum())
        assert counts["clamp_" + cls] > DW * DH // 4
        assert (want[0] == 0).any() and ((want[0] != 0) & ((mx < 0) | (my < 0) | (mx > SW - 1) | (my > SH - 1))).any()   # wholly and partly outside
    # the saturating class: +-40000 and +-2^26 give 0, 2^26 - 8 (in int, far outside short) too
    mx, my, want = base_case("saturating")
    far = (np.abs(mx) >= 32767) | (np.abs(my) >= 32767)
    assert far.sum() > 100 and (want[0][far] == 0).all()
    assert fixed(f32(2.0 ** 26)) == INT_MIN and fixed(f32(-(2.0 ** 26))) == INT_MIN and fixed(f32(2.0 ** 26 - 8)) == (1 << 31) - 256
    return counts


# ---- the 16-bit depth image ----
DEPTH_FACTORS = (f32(1.0) / f32(5000.0), f32(1.0) / f32(1000.0))
DEPTH_RAW = np.array([0, 1, 65535, 3, 7, 4999, 5000, 5001, 12345, 30001, 40961, 54321, 999, 1001, 65533], np.uint16)


def reference_depth(raw, factor):
    """imDepth.convertTo(imDepth, CV_32F, factor): one conversion (exact), one rounded float product."""
    return raw.astype(f32) * f32(factor)


def check_conditions_depth():
    """Some products are inexact for both factors, and dividing in double and rounding once -- (float)((double)raw / 5000.0) -- is another function."""
    for fac in DEPTH_FACTORS:
        exact = DEPTH_RAW.astype(np.float64) * np.float64(fac)
        assert (reference_depth(DEPTH_RAW, fac).astype(np.float64) != exact).sum() >= 5
    assert reference_depth(DEPTH_RAW, DEPTH_FACTORS[0])[0] == 0 and reference_depth(DEPTH_RAW, DEPTH_FACTORS[0])[2] > 13
    n = int(((DEPTH_RAW.astype(np.float64) / 5000.0).astype(f32) != reference_depth(DEPTH_RAW, DEPTH_FACTORS[0])).sum())
    assert n >= 1
    return n
