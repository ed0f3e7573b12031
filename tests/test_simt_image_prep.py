"""The image-preparation calls as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import _stand_alone_under_sanitizers


def test_image_prep_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/image_prep_check.cpp: orbx_rectify_batch_device for destination widths 1, 3, 5, 64, 65 and 67 with 1, 3 and 5 frames, the
    destination at offsets 0 .. 3 of its block, maps that mix a distortion field with the image's last pixel, the borders, saturating and
    non-finite coordinates -- against cv::remap's fixed-point arithmetic written out in C++; orbx_rgbd_batch_device_u16 on an extracted batch of two
    320 x 240 frames (holes of 0, 1 and 65535) against convertTo + Frame::ComputeStereoFromRGBD.  Source, destination and depth images are heap
    blocks of exactly the bytes the calls may touch: a tap read or a dword store past an image ends the run; UBSan sees a float converted outside
    int."""
    r = _stand_alone_under_sanitizers(tmp_path, "image_prep_check")
    assert r.returncode == 0 and "image prep ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
