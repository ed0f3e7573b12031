"""tests/image_enhance_scene.py on its own, without a GPU: its designed inputs reach every class that a wrong kernel would get wrong, the kernel's closed
form of CLAHE's residual loop equals the loop, and the references give the known answers."""
import numpy as np

import image_enhance_scene as S


def test_gray_classes():
    assert S.check_gray_classes()["ties"] >= 8


def test_resize_classes():
    tails = S.check_resize_classes()["tail_cases"]
    assert "enlarge" in tails and "reduce_752_like" not in tails


def test_clahe_classes():
    c = S.check_clahe_classes()
    print(c)
    assert c["flat"] and c["residual_zero"] and c["step_one"] and c["step_two_or_more"] and c["lut_ties"] and c["res_ties"]


def test_residual_closed_form_equals_the_loop():
    """Bin i gets + 1 iff i % step == 0 && i / step < residual, for every residual 0 .. 255 (k_clahe_lut's per-bin update)."""
    for residual in range(256):
        loop, closed = S.residual_loop(residual), S.residual_closed_form(residual)
        assert np.array_equal(loop, closed) and int(loop.sum()) == residual, residual
    # and inside the whole redistribution, on histograms of every kind the cases hold
    for name in ("divisible_8x8", "one_tile", "grid_2x3", "high_clip_2x3"):
        w, h, tiles_x, tiles_y, clip_limit = S.CLAHE_CASES[name]
        src = S.clahe_frames(name, 1)[0]
        stats = {}
        S.reference_clahe(src, clip_limit, tiles_x, tiles_y, stats=stats)
        tw, th = stats["tile"]
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                hist = np.bincount(src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
                want, clipped, residual, _ = S.redistribute_loop(hist, stats["clip"])
                got = np.minimum(hist, stats["clip"]) + clipped // 256 + S.residual_closed_form(residual)
                assert np.array_equal(got, want), (name, tx, ty)


def test_constant_images_stay_constant():
    for v in (0, 1, 77, 254, 255):
        for channels, rgb in S.CODES:
            assert (S.reference_gray(np.full((5, 9, channels), v, np.uint8), rgb) == v).all(), (v, channels, rgb)
        for name, (sw, sh, dw, dh) in S.RESIZE_CASES.items():
            assert (S.reference_resize(np.full((sh, sw), v, np.uint8), dw, dh) == v).all(), (v, name)


def test_clahe_without_clipping_on_one_tile_is_histogram_equalisation():
    """clip_limit <= 0, a 1 x 1 grid: all four tables are the one table and the weights sum to 1, so dst = lut[v] with
    lut[v] = round(255 * (pixels <= v) / area) -- plain histogram equalisation by that formula."""
    src = S.clahe_frames("one_tile", 1)[0]
    h, w = src.shape
    cdf = np.cumsum(np.bincount(src.ravel(), minlength=256))
    lut = np.clip(np.rint(cdf.astype(np.float32) * (np.float32(255.0) / np.float32(w * h))), 0, 255).astype(np.uint8)
    for clip_limit in (0.0, -2.5):
        got = S.reference_clahe(src, clip_limit, 1, 1)
        assert np.array_equal(got, lut[src]), clip_limit
    assert lut[255] == 255 and got.max() == 255


def test_refusal_rule():
    assert S.clahe_refused(3, 48, 8, 8) and S.clahe_refused(61, 4, 8, 8) and not S.clahe_refused(61, 45, 8, 8) and not S.clahe_refused(8, 8, 8, 8)
    assert not S.clahe_refused(5, 48, 8, 8)   # pad 3 < 5
