"""The second launch of the twelve tile passes that go in slices of 2^22 workgroups: alac_resample_rows (k_resample.hip),
alac_clips_gather (k_clips.hip), alac_wave_convert (k_wave.hip), alac_wave_pack (k_wavepack.hip), alac_mel_rows (k_mel.hip),
alac_melfft_rows (k_melfft.hip), alac_fbank_rows (k_fbank.hip), alac_featnorm_partials, alac_featnorm_finish and
alac_featnorm_apply (k_featnorm.hip), alac_stack (k_stack.hip) and alac_specaug (k_specaug.hip). Each launch gets the slice's
first tile as first_tile; only a batch of more than 2^22 tiles has a second slice, and a launch that lost its first_tile would
corrupt such batches alone, silently.

Every test but one runs N = 2^22 + 4 099 items of one tile each, so the second launch starts at first_tile = 2^22 and has 4 099
workgroups. The items' content cycles with period 7 (the clips' with 35), and 2^22 = 2 mod 7 (9 mod 35): a slice that
started at item 0 again, or that read its inputs from the batch's start, would not continue the cycle. The expectation is that
of the 7 (35) items, from the host build or the numpy restatement, repeated; it is compared on the device, and the sentinels in
front of and behind the tensor must be intact. The feature passes read lengths[row] and ids[row] and write stats[row],
out_lengths[row] and draws[row] beside their output: those arrays cycle too and are held to the same comparison, with sentinels of
their own. The tests hold between 150 and 550 MB of device memory; the one that slices the finishing launch alone (two
workgroups per row of 257 bins) holds about 11 GB and skips where that is not to be had.

No test provokes a fault: every pass gets buffers of the sizes its entry asks for."""
import numpy as np
import pytest

from tests import clip_ref as cr
from tests import featnorm_ref as nr
from tests import kaldi_ref as kr
from tests import mel_ref as mr
from tests import melfft_ref as fr
from tests import resample_ref as rr
from tests import specaug_ref as sa
from tests import stack_ref as sr
from tests import wave_ref as wr
from tests import wavepack_ref as pr

pytestmark = pytest.mark.gpu

SLICE = 1 << 22
N = SLICE + 4099
LEAD, TAIL = 9, 8  # elements in front of and behind a tensor: it starts one element behind a 16-byte boundary


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def cycled(torch, block, n):
    """The rows of block [period, k] repeated to n rows, on the device."""
    return to_dev(torch, block).repeat(-(-n // block.shape[0]), 1)[:n].contiguous()


def assert_cycle(torch, body, row, what):
    """body (1-D, on the device) is `row` (numpy, one period) over and over, the last period cut short."""
    row = to_dev(torch, row.reshape(-1))
    period = row.numel()
    full = body.numel() // period
    bad = torch.nonzero((body[:full * period].view(full, period) != row).any(dim=1))[:4].flatten().tolist()
    assert not bad, "%s: periods %s of %d elements differ from the expectation" % (what, bad, period)
    rest = body.numel() - full * period
    assert torch.equal(body[full * period:], row[:rest]), "%s: the last, short period differs" % what


def sentinel_buffer(torch, elems, fill, dtype):
    buf = torch.full((LEAD + elems + TAIL,), fill, dtype=dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    return buf


def assert_guards(buf, elems, fill):
    assert bool((buf[:LEAD] == fill).all()) and bool((buf[LEAD + elems:] == fill).all()), "a sentinel around the tensor is gone"


def test_second_launch_of_alac_resample_rows(torch, pkg):
    """N rows of 2 frames, 2 -> 3: 3 output frames, tiles_per_row = 1, so tile = row and the second launch has first_tile =
    2^22. Row r is class r % 7; the expectation is the host build's output for the 7 rows.

    A launch that ignored first_tile would resample rows 0 .. 4 098 again and leave the rows from 2^22 on unwritten (the
    sentinel); one that wrote to the slice's rows but read from the batch's start would give row 2^22 + j the output of row
    j, whose class j % 7 is not (2^22 + j) % 7."""
    sim = rr.build_resample_sim()
    orig, new, T = 2, 3, 2
    frames = rr.out_frames(orig, new, T)
    rows7 = np.random.default_rng(22).uniform(-1, 1, (7, T)).astype(np.float32)
    rows7[3] = [1.0, -1.0]
    want7 = np.zeros((7, frames), np.float32)
    assert sim.resample_sim_run(orig, new, 6, 0.99, rows7.ctypes.data, T, 7, T, want7.ctypes.data, frames, 0) == 0
    assert frames == 3 and len({w.tobytes() for w in want7}) == 7
    x = cycled(torch, rows7, N)
    fill = rr.SENTINEL - (1 << 32)
    buf = sentinel_buffer(torch, N * frames, fill, torch.int32)
    torch.cuda.synchronize()
    with pkg.NewResampler(orig, new) as rs:
        assert N * -(-(frames + 3) // rs.plan()["tile_out"]) > SLICE
        rs.resample_device(x.data_ptr(), T, N, T, buf.data_ptr() + 4 * LEAD, frames, sync=True)
    assert_cycle(torch, buf[LEAD:LEAD + N * frames], want7.view(np.int32), "rows")
    assert_guards(buf, N * frames, fill)


def test_second_launch_of_alac_clips_gather(torch, pkg):
    """N clips of 3 frames out of 7 raw 16-bit mono slots of 32 frames (no decode in front): tiles_per_clip = 1, so tile = clip
    and the second launch has first_tile = 2^22. begin[j] is a function of j % 35 (clips inside a slot, over slot boundaries
    and over the grid's end); the expectation is clip_ref.ref_clips for the 35 clips.

    A launch that ignored first_tile would gather clips 0 .. 4 098 again and leave the clips from 2^22 on unwritten; one that
    took begin[] from the batch's start would give clip 2^22 + j the frames of clip j, whose begin differs since 2^22 = 9 mod
    35. valid[] and clip_status[] come from alac_clips_meta, which is one launch: they must agree all the same."""
    fl, L, slots = 32, 3, 7
    rng = np.random.default_rng(35)
    pcm = rng.integers(-32768, 32768, (slots, fl)).astype("<i2").view(np.uint8).reshape(slots, 2 * fl)
    frames = np.full(slots, fl, np.uint32)
    status = np.zeros(slots, np.int32)
    begin35 = [(k * 13) % (slots * fl) for k in range(33)] + [slots * fl - 2, slots * fl - 1]  # the last two: over the grid's end
    assert len(set(begin35)) == 35 and max(begin35) + L > slots * fl and any(b % fl > fl - L for b in begin35)
    ref, valid35, cstat35 = cr.ref_clips(pcm, frames, status, fl, 16, 1, wr.FLOAT, begin35, [slots] * 35, L)
    assert sorted(set(valid35.tolist())) == [1, 2, 3] and not cstat35.any()
    d_pcm, d_fr, d_st = to_dev(torch, pcm), to_dev(torch, frames.view(np.int32)), to_dev(torch, status)
    d_begin = cycled(torch, np.array(begin35, np.int64)[:, None], N).flatten()
    d_limit = torch.full((N,), slots, dtype=torch.int64, device="cuda:0")
    fill = wr.SENTINEL - (1 << 32)
    buf = sentinel_buffer(torch, N * L, fill, torch.int32)
    d_valid = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    d_cst = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(pkg.PacketConfig(FrameLength=fl, BitDepth=16, NumChannels=1)) as dec:
        dec.clips_device(d_pcm.data_ptr(), 2 * fl, d_fr.data_ptr(), d_st.data_ptr(), slots, d_begin.data_ptr(), d_limit.data_ptr(), N, L,
                         wr.FLOAT, buf.data_ptr() + 4 * LEAD, L, L, d_valid.data_ptr(), d_cst.data_ptr(), sync=True)
    assert_cycle(torch, buf[LEAD:LEAD + N * L], ref.view(np.int32), "clips")
    assert_guards(buf, N * L, fill)
    assert_cycle(torch, d_valid, valid35.view(np.int32), "valid")
    assert not bool(d_cst.any())


@pytest.mark.parametrize("wtype", [wr.FLOAT, wr.INT], ids=["float", "int"])
@pytest.mark.parametrize("layout", [wr.STREAM, wr.PACKETS], ids=["stream", "packets"])
def test_second_launch_of_alac_wave_convert(torch, pkg, layout, wtype):
    """N raw 16-bit mono slots of one frame (FrameLength 1): tiles_per_packet = 1, so tile = packet and the second launch has
    first_tile = 2^22. Slot i is class i % 7; classes 2 and 5 have frames = 0, so that in the stream layout a packet's column
    is starts[i] = 5 * (i / 7) + (the frames of the classes below i % 7) and not i.

    A launch that ignored first_tile would convert packets 0 .. 4 098 again and leave the columns of the packets from 2^22 on
    unwritten; one that took its slot, frames[] or starts[] from the batch's start would write packet j's sample (class j % 7,
    not (2^22 + j) % 7) or write it to packet j's column."""
    stride = 16
    rng = np.random.default_rng(7)
    slots7 = rng.integers(0, 256, (7, stride), dtype=np.uint8)  # the bytes behind a slot's one sample are garbage
    slots7[:, :2] = np.array([-32768, 32767, 77, -1, 1, -300, 12345], "<i2").view(np.uint8).reshape(7, 2)
    frames7 = np.array([1, 1, 0, 1, 1, 0, 1], np.uint32)
    s_ref, starts7 = wr.ref_stream(slots7, frames7, None, 1, 16, 1, wtype)
    p_ref = wr.ref_packets(slots7, frames7, None, 1, 16, 1, wtype)
    assert s_ref.shape == (1, 5) and int(starts7[7]) == 5 and len(set(p_ref.flatten().tolist())) == 6
    total = 5 * (N // 7) + int(starts7[N % 7])
    d_pcm = torch.cat([cycled(torch, slots7, N).flatten(), torch.zeros(64, dtype=torch.uint8, device="cuda:0")])
    d_fr = cycled(torch, frames7.view(np.int32)[:, None], N).flatten()
    fill = wr.SENTINEL - (1 << 32)
    buf = sentinel_buffer(torch, N, fill, torch.int32)
    d_starts = torch.full((N + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(pkg.PacketConfig(FrameLength=1, BitDepth=16, NumChannels=1)) as dec:
        dec.waveform_device(d_pcm.data_ptr(), stride, d_fr.data_ptr(), None, N, layout, wtype, buf.data_ptr() + 4 * LEAD,
                            N if layout == wr.STREAM else 1, 0 if layout == wr.STREAM else 1, d_starts.data_ptr(), sync=True)
    i = torch.arange(N + 1, dtype=torch.int64, device="cuda:0")
    want_starts = (i // 7) * 5 + to_dev(torch, starts7[:7].astype(np.int64))[i % 7]
    assert torch.equal(d_starts, want_starts), "starts differ from the closed form at %s" % torch.nonzero(d_starts != want_starts)[:4].flatten().tolist()
    if layout == wr.STREAM:
        assert_cycle(torch, buf[LEAD:LEAD + total], s_ref.view(np.int32), "stream")
        assert bool((buf[LEAD + total:] == fill).all()) and bool((buf[:LEAD] == fill).all())
    else:
        assert_cycle(torch, buf[LEAD:LEAD + N], p_ref.view(np.int32), "packets")
        assert_guards(buf, N, fill)


def test_second_launch_of_alac_wave_pack(torch, pkg):
    """N one-frame clips of a float32 waveform in the packets layout (FrameLength 1, 16-bit mono): one segment per clip and
    tiles_per_seg = 1, so tile = clip and the second launch has first_tile = 2^22. Clip i is class i % 7; class 2 is 1.5, which
    saturates, so the clipped count is the number of clips of class 2.

    A launch that ignored first_tile would pack clips 0 .. 4 098 again, leave the samples from 2^22 on unwritten and count the
    saturated ones among the first 4 099 twice; one that read the waveform from the batch's start would write clip j's sample
    (class j % 7, not (2^22 + j) % 7)."""
    x7 = np.array([0.5, -0.25, 1.5, -1.0, 3.0517578125e-05, 0.999, -0.7], np.float32)
    ref, clipped7 = pr.pack_ref(x7[None, :], 16, pr.FLOAT)
    assert clipped7 == 1 and ref.size == 14 and len({ref[2 * k:2 * k + 2].tobytes() for k in range(7)}) == 7
    d_wave = cycled(torch, x7[:, None], N).flatten()
    buf = sentinel_buffer(torch, 2 * N, pr.PCM_SENTINEL, torch.uint8)
    d_clip = torch.full((1,), 0xDEAD, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.NewPacketEncoder(pkg.PacketConfig(FrameLength=1, BitDepth=16, NumChannels=1)) as enc:
        enc.pcm_from_waveform_device(d_wave.data_ptr(), pr.PACKETS, pr.FLOAT, 1, 1, N, buf.data_ptr() + LEAD, d_clip.data_ptr(), sync=True)
    assert_cycle(torch, buf[LEAD:LEAD + 2 * N], ref, "PCM")
    assert_guards(buf, 2 * N, pr.PCM_SENTINEL)
    assert int(d_clip.item()) == N // 7 + (1 if N % 7 > 2 else 0)


def test_second_launch_of_alac_mel_rows(torch, pkg):
    """N rows of 2 samples, n_fft 2, win_length 2, hop 1, centred, no mel stage: 3 frames of 2 bins, tile_frames 64, so
    tiles_per_row = 1, tile = row and the second launch has first_tile = 2^22. Row r is class r % 7; the expectation is the host
    build's output for the 7 rows (34 MB in, 101 MB out).

    A launch that ignored first_tile would compute rows 0 .. 4 098 again and leave the rows from 2^22 on unwritten (the
    sentinel); one that wrote to the slice's rows but read from the batch's start would give row 2^22 + j the spectrogram of
    row j, whose class j % 7 is not (2^22 + j) % 7."""
    sim = mr.build_mel_sim()
    cfg = mr.Cfg(8000, 2, 1, 2)
    T, F, K = 2, 3, 2
    rows7 = np.random.default_rng(14).uniform(-1, 1, (7, T)).astype(np.float32)
    rows7[3] = [1.0, -1.0]
    img, lay = mr.sim_image(sim, cfg, rows7)
    assert mr.out_frames(cfg, T) == F and cfg.K == K
    want7 = mr.rows_of(img, 7, K, F, lay[5], lay[3], lay[4])
    assert want7.shape == (7, K, F) and len({w.tobytes() for w in want7}) == 7
    x = cycled(torch, rows7, N)
    fill = mr.SENTINEL - (1 << 32)
    buf = sentinel_buffer(torch, N * K * F, fill, torch.int32)
    torch.cuda.synchronize()
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        assert ms.out_frames(T) == F and N * -(-F // ms.plan()["tile_frames"]) > SLICE
        ms.mel_device(x.data_ptr(), T, N, T, buf.data_ptr() + 4 * LEAD, K * F, F, sync=True)
    assert_cycle(torch, buf[LEAD:LEAD + N * K * F], np.ascontiguousarray(want7).view(np.int32), "rows")
    assert_guards(buf, N * K * F, fill)


def test_second_launch_of_alac_melfft_rows(torch, pkg):
    """The same with transform="fft": N rows of 3 samples, n_fft 4, win_length 4, hop 2, centred, no mel stage: 2 frames of 3
    bins, tile_frames 64, so tiles_per_row = 1, tile = row and the second launch has first_tile = 2^22; M = 2, so one radix-2 pass
    runs (n_fft 2 has none). Row r is class r % 7; the expectation is the host build's output for the 7 rows (50 MB in, 101 MB
    out).

    A launch that ignored first_tile would compute rows 0 .. 4 098 again and leave the rows from 2^22 on unwritten (the
    sentinel); one that wrote to the slice's rows but read from the batch's start would give row 2^22 + j the spectrogram of
    row j, whose class j % 7 is not (2^22 + j) % 7."""
    sim = fr.build_melfft_sim()
    cfg = mr.Cfg(8000, 4, 2, 4)
    T, F, K = 3, 2, 3
    rows7 = np.random.default_rng(16).uniform(-1, 1, (7, T)).astype(np.float32)
    rows7[3] = [1.0, -1.0, 1.0]
    img, lay = fr.sim_image(sim, cfg, rows7)
    assert mr.out_frames(cfg, T) == F and cfg.K == K
    want7 = mr.rows_of(img, 7, K, F, lay[5], lay[3], lay[4])
    assert want7.shape == (7, K, F) and len({w.tobytes() for w in want7}) == 7
    x = cycled(torch, rows7, N)
    fill = mr.SENTINEL - (1 << 32)
    buf = sentinel_buffer(torch, N * K * F, fill, torch.int32)
    torch.cuda.synchronize()
    with pkg.NewMelSpectrogram(transform="fft", **cfg.kwargs()) as ms:
        fft = ms.fft_plan()
        assert fft["transform"] == 1 and fft["radix"] == [2] and fft["tile_frames"] == 64
        assert ms.out_frames(T) == F and N * -(-F // fft["tile_frames"]) > SLICE
        ms.mel_device(x.data_ptr(), T, N, T, buf.data_ptr() + 4 * LEAD, K * F, F, sync=True)
    assert_cycle(torch, buf[LEAD:LEAD + N * K * F], np.ascontiguousarray(want7).view(np.int32), "rows")
    assert_guards(buf, N * K * F, fill)


def test_second_launch_of_alac_fbank_rows(torch, pkg):
    """N rows of 4 samples, frame length 4, shift 4, one mel bin and the energy column, nothing logged: one frame of 2 columns,
    tile_frames 64, so tiles_per_row = 1, tile = row and the second launch has first_tile = 2^22. Row r is class r % 7; the
    expectation is the host build's output for the 7 rows (67 MB in, 34 MB out).

    A launch that ignored first_tile would compute rows 0 .. 4 098 again and leave the rows from 2^22 on unwritten (the
    sentinel); one that wrote to the slice's rows but read from the batch's start would give row 2^22 + j the features of row
    j, whose class j % 7 is not (2^22 + j) % 7."""
    sim = kr.build_fbank_sim()
    cfg = kr.Cfg(8000, 4, 4, mels=1, energy=True, log=False, log_energy=False)
    T, F, cols = 4, 1, 2
    rows7 = np.random.default_rng(15).uniform(-1, 1, (7, T)).astype(np.float32)
    rows7[3] = [1.0, -1.0, 1.0, -1.0]
    want7 = kr.host_values(sim, cfg, rows7)
    assert kr.out_frames(cfg, T) == F and want7.shape == (7, F, cols)
    assert all(len(set(want7[:, 0, c].tolist())) == 7 for c in range(cols)), "the 7 rows are not distinct in both columns"
    x = cycled(torch, rows7, N)
    fill = mr.SENTINEL - (1 << 32)
    buf = sentinel_buffer(torch, N * cols, fill, torch.int32)
    torch.cuda.synchronize()
    with pkg.NewKaldiFeatures(**cfg.kwargs()) as kf:
        assert kf.out_frames(T) == F and N * -(-F // kf.plan()["tile_frames"]) > SLICE
        kf.features_device(x.data_ptr(), T, N, T, buf.data_ptr() + 4 * LEAD, cols, cols, sync=True)
    assert_cycle(torch, buf[LEAD:LEAD + N * cols], np.ascontiguousarray(want7).view(np.int32), "rows")
    assert_guards(buf, N * cols, fill)


# ---- the feature passes: per-row side arrays beside the output -----------------------------------------------------------
FILL = -0x21524111  # the sentinel of the feature passes' tensors, as int32; 0xDEADBEEF as bits


def assert_classes(rows7, shift, empty):
    """rows7: each class's whole expectation (output and per-row results) as bytes. The seven are pairwise distinct, but for the
    classes in `empty`: rows without a valid frame (a length of 0 and a negative one, which the cycle must hold both) come out as
    padding and zeros whatever they held, so those agree with each other and with nothing else. And class k differs from class
    k + shift, so a slice that began `shift` items late in the cycle would differ in every row."""
    assert len(rows7) == 7
    for i in range(7):
        for j in range(i + 1, 7):
            assert (rows7[i] == rows7[j]) == (i in empty and j in empty), "classes %d and %d" % (i, j)
        assert rows7[i] != rows7[(i + shift) % 7], "class %d and the one %d on" % (i, shift)


def featnorm_slices(torch, pkg, rows, bins, frames, lengths7, empty, sliced, **mode):
    """`rows` rows of [frames, bins] whose content and length are those of class row % 7 through one normalisation pass with the
    statistics requested; output and statistics against the host build's 7 rows as cycles, sentinels around both.
    sliced(chunks, blocks) -> the workgroups per row of each launch that is to go in two slices, read from the handle's plan: they
    agree, so those launches' second slices begin at the same row."""
    sim = nr.build_featnorm_sim()
    x7 = nr.features(np.random.default_rng(70 + bins), 7, frames, bins)
    want7, stats7 = nr.host_values(sim, x7, lengths7, "frames", **mode)
    per_row = frames * bins
    try:
        x = cycled(torch, x7.reshape(7, per_row), rows)
        d_len = cycled(torch, np.asarray(lengths7, np.int32)[:, None], rows).flatten()
        out = sentinel_buffer(torch, rows * per_row, FILL, torch.int32)
        stats = sentinel_buffer(torch, rows * 2 * bins, FILL, torch.int32)
    except RuntimeError as e:
        pytest.skip("no %.1f GiB in four allocations for %d rows of %d bins: %s" % (rows * (2 * per_row + 2 * bins) * 4 / 2.0 ** 30, rows,
                                                                                   bins, str(e).splitlines()[0]))
    torch.cuda.synchronize()
    with pkg.NewFeatureNorm(bins, mode["stat"], None, None, 1e-20, mode.get("range_"), mode["pad"]) as h:
        pl = h.plan()
        per = set(sliced(-(-frames // pl["tile_frames"]), -(-pl["bins"] // 256)))
        assert len(per) == 1, "the launches under test do not share their tiles"
        per = per.pop()
        assert rows * per > SLICE and SLICE % per == 0, "the launches under test have no second slice"
        assert_classes([want7[k].tobytes() + stats7[k].tobytes() for k in range(7)], (SLICE // per) % 7, empty)
        h.norm_device(x.data_ptr(), (per_row, bins, 1), rows, frames, d_len.data_ptr(), out.data_ptr() + 4 * LEAD, (per_row, bins, 1),
                      stats.data_ptr() + 4 * LEAD, sync=True)
    assert_cycle(torch, out[LEAD:LEAD + rows * per_row], want7.view(np.int32), "output")
    assert_guards(out, rows * per_row, FILL)
    assert_cycle(torch, stats[LEAD:LEAD + rows * 2 * bins], stats7.view(np.int32), "stats")
    assert_guards(stats, rows * 2 * bins, FILL)


def test_second_launch_of_the_featnorm_sums(torch, pkg):
    """stat mean_var over N rows of 2 frames x 3 bins: chunks = 1 and one finishing block per row, so alac_featnorm_partials (twice),
    alac_featnorm_finish (twice) and alac_featnorm_apply all have tile = row and a second launch at first_tile = 2^22. Row r has the
    content and the length of class r % 7; the lengths are 2, 1, 0, -4, 5, 2, 1: classes 2 and 3 hold no valid frame.

    A launch that ignored first_tile would leave partial[], stats[] or the output of the rows from 2^22 on as they were (the
    sentinel, or the scratch block's old content); one that narrowed (row * chunks + chunk) * bins or row * 2 * bins would write
    them elsewhere; one that read lengths[], the partials or the statistics from the batch's start would give row 2^22 + j the
    mean, rstd or length of row j, whose class j % 7 is not (2^22 + j) % 7."""
    featnorm_slices(torch, pkg, N, 3, 2, [2, 1, 0, -4, 5, 2, 1], (2, 3), lambda chunks, blocks: (chunks, blocks, chunks),
                    stat="mean_var", pad=-2.0)


def test_second_launch_of_the_featnorm_maximum(torch, pkg):
    """The same with stat max, range 1: the kLargest branch of alac_featnorm_partials (partial[row * chunks + chunk]), the
    one-workgroup-per-row branch of alac_featnorm_finish, which writes all 2 x bins statistics of its row, and the clamp of
    alac_featnorm_apply, which reads stats[row][0][0]."""
    featnorm_slices(torch, pkg, N, 3, 2, [2, 1, 0, -4, 5, 2, 1], (2, 3), lambda chunks, blocks: (chunks, 1, chunks),
                    stat="max", range_=1.0, pad=-2.0)


def test_second_launch_of_alac_featnorm_finish_with_two_blocks_per_row(torch, pkg):
    """R = 2^21 + 2 053 rows of 1 frame x 257 bins, stat mean_var: the finishing launches have two workgroups per row, 2 R > 2^22 in
    all, and are the only ones that go in two slices here. The second starts at first_tile = 2^22 = row 2^21 (= 1 mod 7), block 0,
    behind row 2^21 - 1's block 1, which holds bin 256 alone. With one frame the mean is the value itself, so stats[r][0] is row
    r's input and stats[r][1] the floor's rstd; the lengths are 1, 1, 7, 0, 1, -2, 1: classes 3 and 5 hold no valid frame.

    A launch that took b for the row, or lost first_tile, would write the means of the rows from 2^21 on to other rows or not at
    all. About 2 GB each for input, output and the handle's partial sums and 4 GB for the statistics; skipped where the test's own
    four tensors cannot be allocated."""
    R = (1 << 21) + 2053
    featnorm_slices(torch, pkg, R, 257, 1, [1, 1, 7, 0, 1, -2, 1], (3, 5), lambda chunks, blocks: (blocks,), stat="mean_var", pad=-2.0)


def test_second_launch_of_alac_stack(torch, pkg):
    """N rows of 3 frames x 2 bins, order 1 at window 1, one frame of left context, stride 1: 3 output frames of 8 columns, one tile
    per row, so tile = row and the second launch has first_tile = 2^22. Row r has the content and the length of class r % 7; the
    lengths are 3, 1, 0, -4, 5, 2, 3, and the out lengths are requested.

    A launch that ignored first_tile would leave the output and out_lengths[] of the rows from 2^22 on unwritten (the sentinel);
    one that read the input or lengths[] from the batch's start would give row 2^22 + j the deltas or the length of row j,
    whose class j % 7 is not (2^22 + j) % 7."""
    sim = sr.build_stack_sim()
    ps, bins, frames = (1, 1, 1, 0, 1), 2, 3
    lengths7 = [3, 1, 0, -4, 5, 2, 3]
    x7 = sr.features(np.random.default_rng(71), 7, frames, bins)
    want7, len7 = sr.host_values(sim, x7, lengths7, ps, pad=-2.0)
    G, D = want7.shape[1:]
    x = cycled(torch, x7.reshape(7, frames * bins), N)
    d_len = cycled(torch, np.asarray(lengths7, np.int32)[:, None], N).flatten()
    out = sentinel_buffer(torch, N * G * D, FILL, torch.int32)
    olen = sentinel_buffer(torch, N, FILL, torch.int32)
    torch.cuda.synchronize()
    with pkg.NewFrameStack(bins, *ps, -2.0) as h:
        pl = h.plan()
        per = -(-h.out_frames(frames) // pl["tile_out"])  # the slabs of tile_bins bins are a loop inside the workgroup
        assert (G, D) == (h.out_frames(frames), pl["columns"]) == (3, 8) and per == 1 and N * per > SLICE
        assert_classes([want7[k].tobytes() + len7[k].tobytes() for k in range(7)], SLICE % 7, (2, 3))
        h.stack_device(x.data_ptr(), (frames * bins, bins, 1), N, frames, d_len.data_ptr(), out.data_ptr() + 4 * LEAD, (G * D, D, 1),
                       olen.data_ptr() + 4 * LEAD, sync=True)
    assert_cycle(torch, out[LEAD:LEAD + N * G * D], want7.view(np.int32), "output")
    assert_guards(out, N * G * D, FILL)
    assert_cycle(torch, olen[LEAD:LEAD + N], len7.view(np.int32), "out lengths")
    assert_guards(olen, N, FILL)


def test_second_launch_of_alac_specaug(torch, pkg):
    """N rows of 4 frames x 2 bins, one frequency mask of at most 1 bin, one time mask of at most 2 frames, a warp of 1: tile_out
    64, so tile = row and the second launch has first_tile = 2^22. Row r has the content and the length of class r % 7; the
    lengths are -3, 0, 1, 2, 3, 4, 13, so rows 4, 5 and 6 of a cycle are warped and the others are not.

    Pass 1: ids[r] = 1000 + r % 7 on the device, so the draws cycle too; output and draws against the host build's 7 rows. A
    launch that ignored first_tile would leave the output and draws[] of the rows from 2^22 on unwritten; one that read the
    input, lengths[] or ids[] from the batch's start would give row 2^22 + j the draws and frames of row j.

    Pass 2: no ids and row_base = 2^32 - 2^22 - 1, so row 2^22 has the identity 2^32 - 1 and row 2^22 + 1 the identity 2^32: the
    counter's low word wraps into its high word one row into the second slice. The draws and the output of the rows 0, 2^22 - 1,
    2^22, 2^22 + 1 and N - 1 against specaug_ref.draws_of and the host build run with those identities as ids: a row number
    narrowed to 32 bits, or a low word that did not carry, would draw other masks."""
    sim = sa.build_specaug_sim()
    ps, bins, frames, seed = (1, 1, 1, 2, 65536, 1), 2, 4, 25
    lengths7 = [-3, 0, 1, 2, 3, 4, 13]
    ids7 = [1000 + k for k in range(7)]
    x7 = sa.features(np.random.default_rng(72), 7, frames, bins)
    want7, draws7 = sa.host_values(sim, x7, lengths7, ps, seed, ids=ids7, mask_value=-7.0, pad_value=-2.0)
    P = draws7.shape[1]
    assert [bool(d[1]) for d in draws7] == [False, False, False, False, True, True, True], "which classes are warped"
    per_row = frames * bins
    x = cycled(torch, x7.reshape(7, per_row), N)
    d_len = cycled(torch, np.asarray(lengths7, np.int32)[:, None], N).flatten()
    d_ids = 1000 + torch.arange(N, dtype=torch.int64, device="cuda:0") % 7
    out = sentinel_buffer(torch, N * per_row, FILL, torch.int32)
    draws = sentinel_buffer(torch, N * P, FILL, torch.int32)
    torch.cuda.synchronize()
    with pkg.NewSpecAugment(bins, ps[0], ps[1], ps[2], ps[3], ps[4] / 65536.0, ps[5], -7.0, -2.0) as h:
        pl = h.plan()
        per = -(-frames // pl["tile_out"])
        assert pl["draws"] == P == 6 and per == 1 and N * per > SLICE
        assert_classes([want7[k].tobytes() + draws7[k].tobytes() for k in range(7)], SLICE % 7, ())
        run = lambda row_base, ids: h.specaug_device(x.data_ptr(), (per_row, bins, 1), N, frames, d_len.data_ptr(), seed,
                                                     out.data_ptr() + 4 * LEAD, (per_row, bins, 1), row_base, ids,
                                                     draws.data_ptr() + 4 * LEAD, sync=True)
        run(0, d_ids.data_ptr())
        assert_cycle(torch, out[LEAD:LEAD + N * per_row], want7.view(np.int32), "output")
        assert_guards(out, N * per_row, FILL)
        assert_cycle(torch, draws[LEAD:LEAD + N * P], draws7, "draws")
        assert_guards(draws, N * P, FILL)
        out.fill_(FILL)
        draws.fill_(FILL)
        torch.cuda.synchronize()
        base = (1 << 32) - SLICE - 1
        run(base, 0)
    assert_guards(out, N * per_row, FILL)
    assert_guards(draws, N * P, FILL)
    spots = [0, SLICE - 1, SLICE, SLICE + 1, N - 1]
    idents = [base + r for r in spots]
    assert idents[2] == (1 << 32) - 1 and idents[3] == 1 << 32
    cls = [r % 7 for r in spots]
    want, want_draws = sa.host_values(sim, x7[cls], [lengths7[k] for k in cls], ps, seed, ids=idents, mask_value=-7.0, pad_value=-2.0)
    for j, r in enumerate(spots):
        n = min(max(lengths7[cls[j]], 0), frames)
        assert want_draws[j].tolist() == sa.draws_of(ps, bins, n, seed, idents[j])
        got_draws = draws[LEAD + r * P:LEAD + (r + 1) * P].cpu().numpy()
        assert np.array_equal(got_draws, want_draws[j]), "row %d (identity %d): draws %s, not %s" % (r, idents[j], got_draws, want_draws[j])
        got = out[LEAD + r * per_row:LEAD + (r + 1) * per_row].cpu().numpy()
        assert np.array_equal(got, want[j].reshape(-1).view(np.int32)), "row %d (identity %d): output" % (r, idents[j])
    assert not bool((out[LEAD:LEAD + N * per_row] == FILL).any()) and not bool((draws[LEAD:LEAD + N * P] == FILL).any()), "a row was left unwritten"
    assert len({tuple(d) for d in want_draws.tolist()}) > 1
