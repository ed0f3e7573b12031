"""The colour, resize and CLAHE calls as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_image_enhance_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/image_enhance_check.cpp: orbx_gray_batch_device (the four codes), orbx_resize_batch_device (exact halves, a half in one dimension,
    enlargement, equal size, reductions) and orbx_clahe_batch_device (the four divisibility classes at 8 x 8, the grids 1 x 1, 2 x 3, 3 x 8 and 64 x 2,
    no clipping, a high limit, in place) for widths 1, 3, 5, 64, 65 and 67 with 1, 3 and 5 frames, sources and destinations at offsets 0 .. 3 of
    their blocks -- against cvtColor, cv::resize and clahe.cpp written out in C++.  Sources and destinations are heap blocks of exactly the bytes the
    calls may touch: a read past a source row's last pixel, a dword store past a destination or a reflected coordinate outside the image ends the
    run."""
    r = _stand_alone_under_sanitizers(tmp_path, "image_enhance_check")
    assert r.returncode == 0 and "image enhance ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
