"""The far-buffer helpers (tests/far_buffers.py) bite, shown without a GPU: expectations the suite already trusts — the oracle's
slots, the resampler's host build, the waveform restatement — are placed in sentinel-filled CPU tensors the way a correct entry
places them, and then again with the byte offsets truncated at a line scaled down from 2^32 to 2^16 (far_buffers' `line`
parameter). The comparisons the GPU tests use must pass the first and name the slot, row or channel that moved in the second."""
import re

import numpy as np
import pytest

from tests import far_buffers as fb
from tests import resample_ref as rr
from tests import wave_ref as wr

LINE = 1 << 16  # bytes


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def named(err):
    """the indices an assertion message names in its first [...] list"""
    m = re.search(r"\[([^\]]*)\]", str(err.value))
    return [int(x.split()[-1]) for x in m.group(1).replace("'", "").split(",") if x.strip()]


def slot_rows(torch, ref, bpf, offs):
    out, frames, status = ref
    rows = []
    for i, off in enumerate(offs):
        nb = int(frames[i]) * bpf
        ok = status[i] == 0
        rows.append((i, off, torch.from_numpy(out[i, :nb].copy()) if ok else None, nb if ok else out.shape[1]))
    return rows


def test_decoder_slots_that_wrap_are_named(torch, oracle, synth):
    """24 slots of the oracle's PCM (16-bit stereo, 64 frames: 256 bytes), stride 2^13 - 16, so that slot 8 straddles the scaled
    line as slot 128 straddles 2^32 in the GPU test; half a line of lead. Placed right, the comparison passes. With slot
    offsets truncated to the line's width the slots 9 .. 23 land 2^16 or 2^17 bytes lower, 128 or 256 bytes in front of a lower slot,
    and are all named; with one slot truncated, that slot; with offsets sign-extended as well, the slots land in the lead; and a
    slot written both where it belongs and 2^17 lower is found by the sentinel check, which says where."""
    cfg = oracle.make_config(64, 16, 2)
    b = synth.gen_batch(cfg, 24, threads=2)
    ref = oracle.decode_batch(cfg, b.blob, b.offsets, b.sizes, threads=2)
    assert not ref[2].any() and (ref[1] > 0).all()
    n, stride = 24, fb.slot_stride(LINE, 8)
    offs = [i * stride for i in range(n)]
    assert fb.assert_crosses(offs, [int(f) * 4 for f in ref[1]], 1, LINE) == (8, 1, 15)

    def run(place_at, twice=()):
        far = fb.Far(torch, torch.uint8, n * stride + 64, 0xFF, lead=LINE // 2, device="cpu")
        for i, off in enumerate(place_at):
            far.place(off, torch.from_numpy(ref[0][i, :int(ref[1][i]) * 4].copy()))
        for i, off in twice:
            far.place(off, torch.from_numpy(ref[0][i, :int(ref[1][i]) * 4].copy()))
        fb.check_footprints(torch, far, slot_rows(torch, ref, 4, offs), "scaled decode")

    run(offs)
    with pytest.raises(AssertionError) as e:
        run(fb.truncated(offs, 1, LINE))
    assert set(range(9, 24)) <= set(named(e))  # (and the lower slots whose first bytes they landed on)
    one = list(offs)
    one[17] = fb.truncated(offs, 1, LINE)[17]
    with pytest.raises(AssertionError) as e:
        run(one)
    assert 17 in named(e) and len(named(e)) <= 2
    signed = [t - LINE if t >= LINE // 2 else t for t in fb.truncated(offs, 1, LINE)]
    assert min(signed) < 0
    with pytest.raises(AssertionError) as e:
        run(signed)
    assert {i for i in range(n) if signed[i] != offs[i]} <= set(named(e))
    # the same slots through the strided gather the large batches use
    want = torch.full((n, 256), 0xFF, dtype=torch.uint8)
    for i in range(n):
        want[i, :int(ref[1][i]) * 4] = torch.from_numpy(ref[0][i, :int(ref[1][i]) * 4].copy())
    for place_at, moved in ((offs, None), (one, 17)):
        far = fb.Far(torch, torch.uint8, n * stride + 64, 0xFF, lead=LINE // 2, device="cpu")
        for i, off in enumerate(place_at):
            far.place(off, want[i])
        if moved is None:
            fb.check_strided(torch, far, stride, want, "scaled decode")
        else:
            with pytest.raises(AssertionError) as e:
                fb.check_strided(torch, far, stride, want, "scaled decode")
            assert moved in named(e)
    with pytest.raises(AssertionError) as e:
        run(offs, twice=[(20, offs[20] - 2 * LINE)])  # ends where slot 4 begins
    assert "written outside every slot" in str(e.value) and "element %d " % (offs[20] - 2 * LINE) in str(e.value)


def test_resampled_rows_that_wrap_are_named(torch):
    """Three rows of the resampler's host build (2 -> 3, 40 frames in, 60 out) at an output row stride of 9 001 elements: row 2
    begins 72 008 bytes behind the base, beyond the scaled line. Truncated, it lands at byte 6 472, in the gap behind row 0:
    row 2 is named. The same rows cycled with period 7 in a dense body of 300 rows of 64 bytes (the scaled line is at row 1 024
    of them, so the body is cut at 2^14 bytes here): rows 256 .. 299 wrapped onto rows 0 .. 43 are named, first and last."""
    sim = rr.build_resample_sim()
    x = rr.signal(np.random.default_rng(3), 7, 40)
    frames = rr.out_frames(2, 3, 40)
    y = np.zeros((7, frames), np.float32)
    assert sim.resample_sim_run(2, 3, 6, 0.99, x.ctypes.data, 40, 7, 40, y.ctypes.data, frames, 0) == 0
    want = torch.from_numpy(y.view(np.int32).copy())
    fill = rr.SENTINEL - (1 << 32)
    stride = 9001
    offs = [r * stride for r in range(3)]
    assert fb.assert_crosses(offs, [frames] * 3, 4, LINE, straddle=False) == (2, 0, 1)

    def run(place_at):
        far = fb.Far(torch, torch.int32, 3 * stride, fill, lead=5, device="cpu")
        for r, off in enumerate(place_at):
            far.place(off, want[r])
        fb.check_footprints(torch, far, [(r, offs[r], want[r], frames) for r in range(3)], "scaled rows", unit="row")

    run(offs)
    with pytest.raises(AssertionError) as e:
        run(fb.truncated(offs, 4, LINE))
    assert named(e) == [2]

    n, line_rows = 300, 256
    cyc = want[:, :16].repeat(-(-n // 7), 1)[:n].contiguous()
    fb.check_cycled(torch, cyc, want[:, :16], "scaled cycle", unit="row", chunk_bytes=1 << 12)
    wrapped = cyc.clone()
    wrapped[line_rows:] = fill
    wrapped[:n - line_rows] = cyc[line_rows:]
    assert line_rows % 7 != 0
    for chunk in (1 << 12, 1 << 20):
        with pytest.raises(AssertionError) as e:
            fb.check_cycled(torch, wrapped, want[:, :16], "scaled cycle", unit="row", chunk_bytes=chunk)
        assert named(e) == [0, 1, 2, 3, 296, 297, 298, 299] and "%d rows differ" % (2 * (n - line_rows)) in str(e.value)


def test_waveform_channels_that_wrap_are_named(torch):
    """wave_ref's STREAM tensor of 5 hand-written 16-bit stereo slots at channel_stride 2^14 + 5 elements: channel 1 begins 20
    bytes beyond the scaled line. Truncated, channel 1 lands on channel 0's first five columns: both channels are named, and
    the sentinel behind channel 1's place is the evidence that it moved."""
    rng = np.random.default_rng(9)
    fl, n = 33, 5
    frames = wr.frame_counts(rng, n, fl, "short")
    out = wr.hand_slots(rng, n, fl, 16, 2, fl * 4, frames)
    ref, starts = wr.ref_stream(out, frames, None, fl, 16, 2, wr.FLOAT)
    total = int(starts[-1])
    want = torch.from_numpy(ref.view(np.int32).copy())
    cs = (LINE >> 2) + 5
    offs = [0, cs]
    assert fb.assert_crosses(offs, [total] * 2, 4, LINE, straddle=False) == (1, 0, 1)
    fill = wr.SENTINEL - (1 << 32)

    def run(place_at):
        far = fb.Far(torch, torch.int32, cs + n * fl + 8, fill, lead=3, device="cpu")
        for c in (0, 1):
            far.place(place_at[c], want[c])
        fb.check_footprints(torch, far, [(c, offs[c], want[c], total) for c in (0, 1)], "scaled stream", unit="channel")

    run(offs)
    with pytest.raises(AssertionError) as e:
        run(fb.truncated(offs, 4, LINE))
    assert named(e) == [0, 1]
