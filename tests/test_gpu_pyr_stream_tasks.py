"""k_pyr_stream's per-wave task lists on small geometries (GPU).

A worker wave walks its own list of pre-decoded 64-byte task descriptors: while task t is computed, the descriptor of t + 1 is in flight (a
hand-placed scalar load) and the column entries of t + 1 are already in registers; the barriers of the row schedule are counts inside the
descriptors.  The shapes here are the ones where that bookkeeping is thinnest: levels of ONE column block (most steps leave several of the
eight workers without a task, so waves start late, sit out steps and end on a run of barriers; the last task's fetch ahead reads the list's
unused last descriptor), lists of zero or one task per step, and one-row / two-row tasks with three and four source rows within a few steps.
test_gpu_extractor.py::test_stream_pyramid_and_level0_in_place_on_small_batches covers waves with several tasks per step (752x480, B = 3).
Every padded level of every frame, the keypoints and the descriptors must equal the oracle.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(w, h, nlevels, nf, B):
    """frames and the oracle's outputs for them: computed once per shape, shared by the cases (read-only)"""
    from orb_slam3_amd import synth
    from oracle import oracle_binding as ob
    canvas = synth.make_canvas(1)
    frames = np.stack([synth.frame_from_canvas(canvas, t, w, h, 3000 + t) for t in range(B)])
    frames.setflags(write=False)
    oex = ob.OracleExtractor(nf, 1.2, nlevels, 20, 7, flags=ob.FLAG_DESC_FMA)
    want = []
    for f in range(B):
        mono, kps, desc = oex.extract(frames[f], lap=(0, 0))
        want.append((mono, kps.tobytes(), desc.copy(), [oex.level_padded(l).copy() for l in range(nlevels)]))
    return frames, want


def _check(monkeypatch, w, h, nlevels, nf, B, hook):
    import torch
    import orb_slam3_amd as osa
    monkeypatch.setenv("ORBX_PYR_STREAM_MIN", hook)   # frames from which k_pyr_stream runs, workgroups the band plan aims at, frame rows per step
    frames, want = _reference(w, h, nlevels, nf, B)
    ex = osa.ORBextractor(nf, 1.2, nlevels, 20, 7)
    d = torch.from_numpy(np.array(frames)).cuda()
    ex.extract_batch_device(d.data_ptr(), B, w, h, w, w * h, (0, 0))
    for f in range(B):
        mono, kps, desc = ex.download(f)
        omono, okps, odesc, olevels = want[f]
        assert len(okps) > 0
        assert mono == omono and kps.tobytes() == okps and np.array_equal(desc, odesc), f
        for l in range(nlevels):
            assert np.array_equal(ex.get_level(l, f), olevels[l]), (f, l)


@pytest.mark.parametrize("rows", [3, 10])
@pytest.mark.parametrize("bands", [1, 2, 4])
def test_single_column_block_levels(monkeypatch, bands, rows):
    """208x160, 5 levels: every level is one column block of 35 - 62 dwords; 1, 2 and 4 bands per frame, 3 and 10 frame rows per step"""
    B = 2
    _check(monkeypatch, 208, 160, 5, 300, B, f"1,{B * bands},{rows}")


def test_many_steps_of_about_one_task(monkeypatch):
    """160x120, 4 levels, one frame, 3 frame rows per step: many steps with about one task each"""
    _check(monkeypatch, 160, 120, 4, 200, 1, "1,1,3")


@pytest.mark.parametrize("bands", [1, 2])
def test_mixed_task_kinds_within_a_few_steps(monkeypatch, bands):
    """320x240, 8 levels: level 1 has two column blocks (64 + 13 dwords), the others one; one-row and two-row tasks with three and four source rows"""
    B = 3
    _check(monkeypatch, 320, 240, 8, 500, B, f"1,{B * bands}")
