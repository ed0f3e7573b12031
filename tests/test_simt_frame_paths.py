"""Every path of the resident frame handle, both kinds, as a stand-alone program on the SIMT emulator, under AddressSanitizer and UBSan (no GPU)."""
from test_simt_emulation import ROOT, _stand_alone_under_sanitizers


def test_frame_handle_paths_of_both_kinds_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/frame_paths_check.cpp: per kind (monocular, fisheye-stereo) four handles of one 320 x 240 frame, of one capacity above N -- loaded from
    host arrays, from the batch and counted first, from the batch with the count(s) pending, and from the batch over a handle that just held another
    frame of the OTHER kind (loaded, searched, given BoW) -- reloaded per call and run through the three projection searches with and without an
    occupancy mask, SearchLocalPoints (300 map points, with a mask, none), ComputeBoW (both id buffers, one, none) and SearchByBoW against two host
    key frames and one resident one; an empty host-loaded frame through SearchLocalPoints.  Equal return values and entries [0, N) from all four, the
    counted handle's counts afterwards, the caller's arrays (heap blocks of exactly the needed size, filled with a sentinel) untouched beyond the rows
    in use, and each kind's entry points refuse the other kind's handle before they enqueue anything.  A stand-alone program under the sanitizers
    (test_simt_emulation._stand_alone_under_sanitizers): a copy past the caller's array or a kernel writing past a row ends the run.  The whole output
    -- return values, counts, checksums and the transfer numbers of every load and call -- equals profiles/frame_paths_check_new.txt, which is also
    what the library of the commit before the loaders, result tails and BoW arrays were unified printed (profiles/frame_paths_check_parent.txt); a
    change that means to alter a transfer table or a result stores the program's new output there."""
    r = _stand_alone_under_sanitizers(tmp_path, "frame_paths_check")
    assert r.returncode == 0 and "frame paths ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    want = (ROOT / "profiles" / "frame_paths_check_new.txt").read_text().splitlines()
    got = r.stdout.splitlines()
    diff = [i for i in range(max(len(want), len(got))) if i >= len(want) or i >= len(got) or want[i] != got[i]]
    assert not diff, f"line {diff[0] + 1}: {got[diff[0]] if diff[0] < len(got) else None!r} against the stored {want[diff[0]] if diff[0] < len(want) else None!r}"
