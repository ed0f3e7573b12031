"""References and designed inputs for the colour, resize and CLAHE stages in front of the extractor (orbx_gray_batch_device, orbx_resize_batch_device,
orbx_clahe_batch_device), as include/orbx.h restates OpenCV 4.x.  No product code is imported: gray and the exact-half resize are numpy integers, the
generic resize is the oracle's resize_linear, CLAHE is written with clahe.cpp's LOOP form of the redistribution and np.float32 operations one at a
time (np.rint rounds to nearest, ties to even, as cvRound does).  check_*_classes() assert, on the references alone, that the inputs reach every class a
wrong kernel would get wrong; tests/test_image_enhance_scene.py runs them without a GPU."""
import functools

import numpy as np

F = np.float32

# ---------------------------------------------------------------------------------------------------------
# gray
# ---------------------------------------------------------------------------------------------------------
CR, CG, CB = 9798, 19235, 3735
GRAY_WIDTHS = (1, 3, 5, 64, 65, 67)
GRAY_H = 7
CODES = ((3, True), (3, False), (4, True), (4, False))   # (channels, rgb): RGB2GRAY, BGR2GRAY, RGBA2GRAY, BGRA2GRAY


def reference_gray(src, rgb):
    """src [..., channels] uint8 -> [...] uint8; a fourth channel is skipped."""
    c = src.astype(np.int64)
    r, b = (c[..., 0], c[..., 2]) if rgb else (c[..., 2], c[..., 0])
    return ((r * CR + c[..., 1] * CG + b * CB + 16384) >> 15).astype(np.uint8)


@functools.lru_cache(None)
def gray_tie_pixels():
    """(R, G, B) triples whose weighted sum, modulo 32768, lies just below 16384, exactly on it (the sum lands on .5 before the + 16384) and just
    above it: eight of each, [3][8][3].  The coefficients sum to 32768, so the remainder depends on (R - B, G - B) alone; the remainders 16383 and
    16385 do not occur for 8-bit pixels (asserted in check_gray_classes), so "one unit either side" is the nearest remainder that does."""
    a, c = np.meshgrid(np.arange(-255, 256), np.arange(-255, 256), indexing="ij")
    rem = (a * CR + c * CG) % 32768
    below, above = int(rem[rem < 16384].max()), int(rem[rem > 16384].min())
    out = []
    for want in (below, 16384, above):
        found = []
        for da, dc in np.argwhere(rem == want) - 255:
            b = int(max(0, -da, -dc))   # the smallest B with R = da + B, G = dc + B inside a byte
            if max(da, dc, 0) + b <= 255:
                found.append((int(da) + b, int(dc) + b, b))
                if b + 40 + max(da, dc, 0) <= 255:
                    found.append((int(da) + b + 40, int(dc) + b + 40, b + 40))
        assert len(found) >= 8, (want, len(found))
        out.append(found[:8])
    return np.array(out, np.uint8)


def gray_remainders():
    """The remainders next to the tie that 8-bit pixels reach: (below, above)."""
    a, c = np.meshgrid(np.arange(-255, 256), np.arange(-255, 256), indexing="ij")
    rem = (a * CR + c * CG) % 32768
    return int(rem[rem < 16384].max()), int(rem[rem > 16384].min())


def gray_frames(n, w, channels, seed=0):
    """[n, GRAY_H, w, channels] random bytes; the designed triples stand first (as R, G, B and as B, G, R, so that both byte orders meet them), then
    saturated pixels; every other fourth channel is 255."""
    rng = np.random.default_rng(100 + seed + 7 * w + channels)
    a = rng.integers(0, 256, (n, GRAY_H, w, channels), dtype=np.uint8)
    special = np.concatenate([gray_tie_pixels().reshape(-1, 3), gray_tie_pixels().reshape(-1, 3)[:, ::-1],
                              np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)])
    flat = a.reshape(n, -1, channels)
    k = min(len(special), flat.shape[1])
    flat[:, :k, :3] = special[:k]
    if channels == 4:
        flat[:, ::2, 3] = 255
    return a


def check_gray_classes():
    t = gray_tie_pixels().astype(np.int64)
    s = t[..., 0] * CR + t[..., 1] * CG + t[..., 2] * CB
    below, above = gray_remainders()
    assert below < 16383 and above > 16385, "no 8-bit pixel is exactly one unit off the tie"
    assert (s[0] % 32768 == below).all() and (s[1] % 32768 == 16384).all() and (s[2] % 32768 == above).all()
    g = reference_gray(gray_tie_pixels(), True).astype(np.int64)
    # on the tie and above it the result is the upper neighbour (half up), one unit below it the lower: a kernel that truncates, or rounds ties to even, differs
    assert (g[0] == s[0] >> 15).all() and (g[1] == (s[1] >> 15) + 1).all() and (g[2] == (s[2] >> 15) + 1).all()
    assert ((s[1] >> 15) % 2 == 0).any(), "a tie above an even value: ties-to-even would differ"
    # one buffer under all four codes: rows of 12 * m bytes are 4 m three-channel or 3 m four-channel pixels
    buf = np.random.default_rng(5).integers(0, 256, (GRAY_H, 12 * 16), dtype=np.uint8)
    buf[:, 3::4] = 255   # the alpha bytes of the four-channel reading
    three, four = buf.reshape(GRAY_H, 64, 3), buf.reshape(GRAY_H, 48, 4)
    outs = [reference_gray(three, True), reference_gray(three, False), reference_gray(four, True), reference_gray(four, False)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert (outs[i][:, :48] != outs[j][:, :48]).mean() > 0.5, (i, j)
    # alpha 255 must not leak: the result is that of the same pixels with alpha 0, and reading the fourth byte as a colour would differ
    zero = four.copy()
    zero[..., 3] = 0
    assert np.array_equal(reference_gray(zero, True), outs[2]) and not np.array_equal(reference_gray(four[..., 1:], True), outs[2])
    f = gray_frames(1, 67, 4)
    assert (f[..., 3] == 255).mean() > 0.4 and (f[..., 3] != 255).mean() > 0.4
    return {"ties": int(s[1].size)}


# ---------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------
# name -> (src_w, src_h, dst_w, dst_h).  The destination widths 1, 3, 5, 64, 65, 67 all occur.
RESIZE_CASES = {
    "exact_half": (130, 22, 65, 11),
    "exact_half_odd_groups": (10, 6, 5, 3),
    "half_in_x_only": (128, 22, 64, 13),
    "half_in_y_only": (67, 26, 67, 13),
    "enlarge": (41, 9, 67, 14),
    "equal_size": (64, 13, 64, 13),
    "to_width_1": (37, 11, 1, 5),
    "to_width_3": (7, 8, 3, 4),
    "reduce_752_like": (94, 60, 65, 41),
    "reduce_non_integer": (77, 19, 64, 15),
    "enlarge_by_one": (2, 2, 3, 5),
}


def resize_offsets(ssize, dsize):
    """floor of OpenCV's source coordinate per destination index, before the horizontal reset (the oracle's linear_tab)."""
    scale = 1.0 / (float(dsize) / ssize)
    return np.array([int(np.floor(F((d + 0.5) * scale - 0.5))) for d in range(dsize)])


def reference_resize(src, dw, dh):
    from oracle import oracle_binding as ob
    sh, sw = src.shape
    if sw == 2 * dw and sh == 2 * dh:
        s = src.astype(np.int32)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return ob.resize_linear(np.ascontiguousarray(src), dw, dh)


def resize_frames(n, sw, sh, seed=0):
    rng = np.random.default_rng(200 + seed + sw * 31 + sh)
    a = rng.integers(0, 256, (n, sh, sw), dtype=np.uint8)
    a[:, :, -1] = 255 - a[:, :, 0]   # the last column, which the tail reads, differs from what a read one further (the next row's first) gives
    return a


def check_resize_classes():
    from oracle import oracle_binding as ob
    seen = set()
    for name, (sw, sh, dw, dh) in RESIZE_CASES.items():
        src = resize_frames(1, sw, sh)[0]
        want = reference_resize(src, dw, dh)
        assert want.shape == (dh, dw)
        seen.add(dw)
        generic = ob.resize_linear(src, dw, dh)
        xo = resize_offsets(sw, dw)
        if name.startswith("exact_half"):
            # the pair kernel's case.  (At exactly 2 both fractions are .5, the coefficients 1024, and the generic arithmetic reduces to the same
            # (a + b + c + d + 2) >> 2: OpenCV's switch changes no byte, and neither may the kernel's.)
            assert sw == 2 * dw and sh == 2 * dh and np.array_equal(want, generic), name
        else:
            assert not (sw == 2 * dw and sh == 2 * dh) and np.array_equal(want, generic), name
        if name == "half_in_x_only":
            assert sw == 2 * dw and sh != 2 * dh
            area_x = ((src[:, 0::2].astype(int) + src[:, 1::2] + 1) >> 1)
            assert area_x.shape[1] == dw   # (a kernel that took the pair path for this case would start from such pairs)
        if name == "half_in_y_only":
            assert sh == 2 * dh and sw == dw
        if name.startswith("enlarge"):
            assert dw > sw and dh > sh and xo[0] < 0 and xo[-1] + 1 >= sw, name   # reset at the left border, the tail at the right
        if name == "equal_size":
            assert np.array_equal(want, src)
        if name.startswith("reduce"):
            assert xo[-1] + 1 < sw and (np.diff(xo) > 1).any(), name   # no tail; columns are skipped
    assert seen >= {1, 3, 5, 64, 65, 67}, seen
    tails = [n for n, (sw, sh, dw, dh) in RESIZE_CASES.items() if resize_offsets(sw, dw)[-1] + 1 >= sw]
    assert "enlarge" in tails and "equal_size" in tails, tails
    return {"tail_cases": tails}


# ---------------------------------------------------------------------------------------------------------
# CLAHE
# ---------------------------------------------------------------------------------------------------------
# name -> (width, height, tiles_x, tiles_y, clip_limit)
CLAHE_CASES = {
    "divisible_8x8": (64, 48, 8, 8, 3.0),
    "width_only_8x8": (67, 48, 8, 8, 3.0),
    "height_only_8x8": (64, 45, 8, 8, 3.0),
    "neither_8x8": (61, 45, 8, 8, 3.0),
    "one_tile": (40, 30, 1, 1, 3.0),
    "grid_2x3": (40, 30, 2, 3, 3.0),
    "grid_3x8": (40, 30, 3, 8, 3.0),
    "no_clip_zero": (40, 30, 2, 3, 0.0),
    "no_clip_negative": (64, 48, 8, 8, -1.0),
    "high_clip_2x3": (40, 30, 2, 3, 40.0),
}


def clahe_geometry(w, h, tiles_x, tiles_y, independent_pads=False):
    """(pad_x, pad_y, tile_w, tile_h).  independent_pads: the WRONG rule that pads each dimension only when that dimension fails to divide."""
    pad_x = pad_y = 0
    if independent_pads:
        pad_x, pad_y = (tiles_x - w % tiles_x) % tiles_x, (tiles_y - h % tiles_y) % tiles_y
    elif w % tiles_x or h % tiles_y:
        pad_x, pad_y = tiles_x - w % tiles_x, tiles_y - h % tiles_y
    return pad_x, pad_y, (w + pad_x) // tiles_x, (h + pad_y) // tiles_y


def clahe_refused(w, h, tiles_x, tiles_y):
    pad_x, pad_y, _, _ = clahe_geometry(w, h, tiles_x, tiles_y)
    return pad_x >= w or pad_y >= h


def _reflect101(n_ext, n):
    i = np.arange(n_ext)
    return np.where(i < n, i, 2 * (n - 1) - i)


def redistribute_loop(hist, clip):
    """clahe.cpp's clipping and redistribution on one histogram (int64 [256]), the loop as written; returns (hist, clipped, residual, step)."""
    hist = hist.copy()
    clipped = int(np.maximum(hist - clip, 0).sum())
    hist = np.minimum(hist, clip)
    batch = clipped // 256
    residual = clipped - batch * 256
    hist += batch
    res0, step = residual, 0
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    return hist, clipped, res0, step


def residual_closed_form(residual):
    """The kernel's form of the residual loop: which bins get + 1."""
    i = np.arange(256)
    if residual == 0:
        return np.zeros(256, bool)
    step = max(256 // residual, 1)
    return (i % step == 0) & (i // step < residual)


def residual_loop(residual):
    hit = np.zeros(256, bool)
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hit[i] = True
            i += step
            residual -= 1
    return hit


def reference_clahe(src, clip_limit, tiles_x, tiles_y, independent_pads=False, clamp_first=False, stats=None):
    """cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply on one image [h, w] uint8.  independent_pads, clamp_first: WRONG variants for the class
    asserts (clamp_first clamps tx1 / ty1 before tx2, xa / ty2, ya are taken from it).  stats: a dict that receives per-tile figures and tie counts."""
    h, w = src.shape
    pad_x, pad_y, tile_w, tile_h = clahe_geometry(w, h, tiles_x, tiles_y, independent_pads)
    assert (pad_x < w and pad_y < h) or independent_pads
    ext = src[np.ix_(_reflect101(h + pad_y, h), _reflect101(w + pad_x, w))]
    area = tile_w * tile_h
    clip = max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0
    lut_scale = F(255.0) / F(area)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    tiles = []
    lut_ties = 0
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = ext[ty * tile_h:(ty + 1) * tile_h, tx * tile_w:(tx + 1) * tile_w]
            hist = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
            info = dict(flat=int(hist.max()) == area, clipped=0, residual=0, step=0)
            if clip > 0:
                hist, info["clipped"], info["residual"], info["step"] = redistribute_loop(hist, clip)
                assert hist.sum() == area
            prod = np.cumsum(hist).astype(F) * lut_scale   # one rounded float product per entry
            lut_ties += int((prod - np.floor(prod) == F(0.5)).sum())
            luts[ty, tx] = np.clip(np.rint(prod), 0, 255).astype(np.uint8)
            tiles.append(info)
    inv_tw, inv_th = F(1.0) / F(tile_w), F(1.0) / F(tile_h)

    def axis(n, inv, count):
        f = np.arange(n).astype(F) * inv - F(0.5)
        t1 = np.floor(f)
        i1 = t1.astype(np.int64)
        c1, c2 = np.maximum(i1, 0), np.minimum(i1 + 1, count - 1)
        a = f - t1
        if clamp_first:   # WRONG: the second tile and the weight taken from the clamped first one
            c2, a = np.minimum(c1 + 1, count - 1), f - c1.astype(F)
        return c1, c2, a, F(1.0) - a, i1

    tx1, tx2, xa, xa1, fx = axis(w, inv_tw, tiles_x)
    ty1, ty2, ya, ya1, fy = axis(h, inv_th, tiles_y)
    v = src.astype(np.int64)
    l11, l12 = luts[ty1[:, None], tx1[None, :], v].astype(F), luts[ty1[:, None], tx2[None, :], v].astype(F)
    l21, l22 = luts[ty2[:, None], tx1[None, :], v].astype(F), luts[ty2[:, None], tx2[None, :], v].astype(F)
    top = l11 * xa1[None, :] + l12 * xa[None, :]
    bot = l21 * xa1[None, :] + l22 * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    assert res.dtype == F
    if stats is not None:
        stats.update(tiles=tiles, clip=clip, area=area, tile=(tile_w, tile_h), pads=(pad_x, pad_y), lut_ties=lut_ties,
                     res_ties=int((res - np.floor(res) == F(0.5)).sum()),
                     left=int((fx < 0).sum()), right=int((fx + 1 > tiles_x - 1).sum()), above=int((fy < 0).sum()), below=int((fy + 1 > tiles_y - 1).sum()),
                     xa_left=xa[fx < 0].copy())
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe_frames(name, n, seed=0):
    """[n, h, w] for a case: a smooth scene with noise, and on top of it, in the cells of the tile grid (the divisible part of it) by turns: a flat
    cell, a cell of all-different values (no bin above 1), a cell of a few neighbouring values (large `clipped`), a two-valued cell, the scene."""
    w, h, tiles_x, tiles_y, _ = CLAHE_CASES[name]
    rng = np.random.default_rng(300 + seed + w * 131 + h * 17 + tiles_x)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint8)
    cw, ch = max(w // tiles_x, 1), max(h // tiles_y, 1)
    for f in range(n):
        img = 128 + 70 * np.sin(xx / 9.0 + f) * np.cos(yy / 7.0) + rng.integers(-25, 26, (h, w))
        k = f
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                cell = (slice(ty * ch, (ty + 1) * ch), slice(tx * cw, (tx + 1) * cw))
                shape = img[cell].shape
                kind = k % 5
                k += 1
                if kind == 0:
                    img[cell] = 17 + 40 * ((tx + ty + f) % 6)
                elif kind == 1:
                    img[cell] = np.resize(rng.permutation(256), shape[0] * shape[1]).reshape(shape)   # (repeated beyond 256 pixels)
                elif kind == 2:
                    img[cell] = 90 + rng.integers(0, 4, shape)
                elif kind == 3:
                    img[cell] = np.where(rng.integers(0, 2, shape) == 1, 250, 3)
        out[f] = np.clip(img, 0, 255).astype(np.uint8)
    return out


@functools.lru_cache(None)
def clahe_case(name, n=1):
    """(frames [n, h, w], reference [n, h, w], stats of frame 0): computed once, read-only."""
    w, h, tiles_x, tiles_y, clip_limit = CLAHE_CASES[name]
    src = clahe_frames(name, n)
    stats = {}
    want = np.stack([reference_clahe(src[f], clip_limit, tiles_x, tiles_y, stats=stats if f == 0 else None) for f in range(n)])
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want, stats


# An interpolated `res` exactly on a .5 tie: the search over the cases' pixels finds them at these sizes (hundreds where the tile is 8 x 6: the weights
# are multiples of 1 / 16 and 1 / 12), none in the 1 x 1 grid, where all four tables are the same; check_clahe_classes() asserts the total.
def check_clahe_classes():
    S = {name: clahe_case(name)[2] for name in CLAHE_CASES}
    # geometry
    assert S["divisible_8x8"]["pads"] == (0, 0) and S["divisible_8x8"]["tile"] == (8, 6)
    assert S["width_only_8x8"]["pads"] == (5, 8) and S["width_only_8x8"]["tile"] == (9, 7)   # a FULL extra tiles_y rows
    assert S["height_only_8x8"]["pads"] == (8, 3) and S["height_only_8x8"]["tile"] == (9, 6)
    assert S["neither_8x8"]["pads"] == (3, 3) and S["neither_8x8"]["tile"] == (8, 6)
    assert S["grid_3x8"]["pads"] == (2, 2) and S["one_tile"]["pads"] == (0, 0) and S["grid_2x3"]["pads"] == (0, 0)
    for name in ("width_only_8x8", "height_only_8x8"):
        w, h, tx, ty, cl = CLAHE_CASES[name]
        src, want, _ = clahe_case(name)
        assert (reference_clahe(src[0], cl, tx, ty, independent_pads=True) != want[0]).mean() > 0.05, name   # a pad of 0 rows / columns differs
    # the clamps with xa, ya taken before them
    for name, s in S.items():
        assert s["left"] > 0 and s["above"] > 0, name
        if s["pads"] == (0, 0):   # (with padding the last tile's centre may lie beyond the image)
            assert s["right"] > 0 and s["below"] > 0, name
        w, h, tx, ty, cl = CLAHE_CASES[name]
        assert (s["xa_left"] > 0).all() and (s["xa_left"] < 1).all()
    for name in ("divisible_8x8", "grid_2x3", "neither_8x8"):
        w, h, tx, ty, cl = CLAHE_CASES[name]
        src, want, _ = clahe_case(name)
        assert (reference_clahe(src[0], cl, tx, ty, clamp_first=True) != want[0]).mean() > 0.02, name
    # clip limits
    assert S["divisible_8x8"]["clip"] == 1 and 3.0 * S["divisible_8x8"]["area"] / 256 < 1   # raised to 1
    assert S["grid_2x3"]["clip"] == 2 and S["one_tile"]["clip"] == 14 and S["high_clip_2x3"]["clip"] == 31
    assert S["no_clip_zero"]["clip"] == 0 and S["no_clip_negative"]["clip"] == 0
    tiles = [t for name, s in S.items() if s["clip"] > 0 for t in s["tiles"]]
    counts = dict(flat=sum(t["flat"] for t in tiles),
                  residual_zero=sum(t["residual"] == 0 for t in tiles),
                  residual_zero_clipped=sum(t["residual"] == 0 and t["clipped"] > 0 for t in tiles),
                  step_one=sum(t["step"] == 1 for t in tiles),
                  step_two_or_more=sum(t["step"] >= 2 for t in tiles),
                  batch=sum(t["clipped"] >= 256 for t in tiles),
                  lut_ties=sum(s["lut_ties"] for s in S.values()), res_ties=sum(s["res_ties"] for s in S.values()))
    assert counts["flat"] >= 10 and counts["residual_zero"] >= 5 and counts["step_one"] >= 2 and counts["step_two_or_more"] >= 50, counts
    assert counts["batch"] >= 1 and counts["lut_ties"] >= 10 and counts["res_ties"] >= 10, counts
    # with step >= 2 the loop ends on `residual`, not on i: the last bin it reaches lies below 256 - step
    for t in tiles:
        if t["step"] >= 2:
            assert (t["residual"] - 1) * t["step"] < 256 - t["step"] or t["residual"] * t["step"] <= 256
    flat_clipped = max(t["clipped"] for t in tiles if t["flat"])
    assert flat_clipped == max(s["area"] - s["clip"] for s in S.values() if s["clip"] > 0 and any(t["flat"] for t in s["tiles"]))
    return counts
