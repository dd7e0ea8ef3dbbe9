"""alacgpu_clips_device on the GPU: crops at arbitrary frame offsets gathered behind an unsynchronized device decode, bit
for bit what the numpy restatement of tests/clip_ref.py makes of the ORACLE's decode of the same packets; and the Python
entries over it: decode_clips, load(frame_offset, num_frames) and load_clips.

Every gather writes into a buffer filled with a sentinel, with slack in channel_stride / clip_stride and elements in front
of and behind the tensor, and the WHOLE buffer is compared: the values, the zeros, and every element outside the rows still
the sentinel. No test provokes a fault: damaged packets are data errors the decoder reports as status, and the hostile
descriptors are out-of-range values the kernel clamps."""
import importlib

import numpy as np
import pytest

from tests import clip_ref as cr
from tests import m4a
from tests import wave_ref as wr

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def u64_tensor(torch, values, dev):
    return torch.from_numpy(np.array([int(v) for v in values], np.uint64).view(np.int64)).to(dev)


def descriptors(n, fl, L):
    """Clips all over the batch: every begin % 4, slot boundaries and the frames around them, the batch's end and the frames
    around it, limits that cut a clip, and the hostile values: begin past the batch and at the top of 64 bits, limit 0 and
    above n."""
    total = n * fl
    begin = [0, 1, 2, 3, fl - 1, fl, fl + 1, 2 * fl + 2, total // 2, total // 3 + 1, max(total - L, 0), max(total - L, 0) + 1, total - 1,
             total, total + 1, total + L, U64, U64 - L + 1, 1 << 63, (1 << 32) + 1, 0, 0, 0, fl + 3, 5]
    limit = [n] * 20 + [0, n + 7, U64, 2, 1]
    assert len(begin) == len(limit)
    return begin, limit


def gather(torch, dec, b, begin, limit, L, wtype, base, slack):
    """Decode (sync = 0) and gather (sync = 1) on the handle's stream; the clips tensor `base` elements behind a 16-byte
    boundary inside a sentinel-filled buffer -> (image uint32, lead, cs, ps, valid, clip_status, frames, status)."""
    cfg, n = b.cfg, b.n
    fl, ch = cfg.frame_length, cfg.num_channels
    stride = (fl * ch * wr.BPS[cfg.bit_depth] + 15) // 16 * 16
    dev = b.d_blob.device
    d_out = torch.full((n * stride,), 0x5A, dtype=torch.uint8, device=dev)
    d_fr = torch.full((n,), 12345, dtype=torch.int32, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    B = len(begin)
    cs = L + slack
    ps = ch * cs + 3
    lead = 8 + base
    buf = torch.full((lead + B * ps + 8,), wr.SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    d_begin, d_limit = u64_tensor(torch, begin, dev), u64_tensor(torch, limit, dev)
    d_valid = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_cst = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dec.decode_batch_device(b.d_blob.data_ptr(), b.d_blob.numel(), b.d_off.data_ptr(), b.d_sz.data_ptr(), n, d_out.data_ptr(), stride,
                            d_fr.data_ptr(), d_st.data_ptr(), sync=False)
    dec.clips_device(d_out.data_ptr(), stride, d_fr.data_ptr(), d_st.data_ptr(), n, d_begin.data_ptr(), d_limit.data_ptr(), B, L, wtype,
                     buf.data_ptr() + 4 * lead, cs, ps, d_valid.data_ptr(), d_cst.data_ptr(), sync=True)
    return (buf.cpu().numpy().view(np.uint32), lead, cs, ps, d_valid.cpu().numpy().view(np.uint32), d_cst.cpu().numpy(),
            d_fr.cpu().numpy().view(np.uint32), d_st.cpu().numpy())


def assert_image(img, want, lead):
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("element %d of the buffer (tensor starts at %d): got %#x, want %#x (%d differ)"
                             % (bad[0], lead, img[bad[0]], want[bad[0]], len(bad)))


@pytest.mark.parametrize("depth,ch,fl,n,Ls", [(16, 2, 4096, 12, (5000, 257)), (24, 6, 33, 40, (1000,)), (32, 1, 7, 60, (256,)),
                                               (20, 8, 256, 10, (255,))])
def test_gather_behind_an_unsynchronized_decode(torch, pkg, oracle, synth, helpers, depth, ch, fl, n, Ls):
    cfg = oracle.make_config(fl, depth, ch)
    b = cr.Batch(torch, oracle, helpers, cfg, cr.packet_list(synth, helpers, cfg, n, depth + fl, damaged=3))
    out, r_frames, r_status = b.ref
    assert (r_status != 0).any() and (r_frames < fl).any()
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg), 0) as dec:
        for L in Ls:
            begin, limit = descriptors(b.n, fl, L)
            for wtype in (wr.FLOAT, wr.INT):
                ref, r_valid, r_cst = cr.ref_clips(out, r_frames, r_status, fl, depth, ch, wtype, begin, limit, L)
                assert r_valid.max() > L // 2 and r_valid.min() == 0 and r_cst.any()
                for base in range(4):
                    img, lead, cs, ps, valid, cst, frames, status = gather(torch, dec, b, begin, limit, L, wtype, base,
                                                                           slack=1 + L % 2 if base else 0)
                    assert np.array_equal(status, r_status) and np.array_equal(frames, r_frames)
                    assert_image(img, cr.expected_image(ref, img.size, lead, cs, ps), lead)
                    assert np.array_equal(valid, r_valid) and np.array_equal(cst, r_cst)
        assert dec.clips_last_ms() > 0 and dec.last_kernel_ms() > 0


def test_argument_checks(torch, pkg):
    cfg = pkg.PacketConfig(FrameLength=64, BitDepth=16, NumChannels=2)
    dev = torch.device("cuda:0")
    n, fb, B, L = 4, 64 * 4, 3, 50
    pcm = torch.zeros(n * fb, dtype=torch.uint8, device=dev)
    fr = torch.zeros(n, dtype=torch.int32, device=dev)
    bg = torch.zeros(B, dtype=torch.int64, device=dev)
    lm = torch.full((B,), n, dtype=torch.int64, device=dev)
    clips = torch.full((B * 2 * L + 4,), 7.0, dtype=torch.float32, device=dev)
    valid = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(cfg, 0) as dec:
        P, F, G, M, C = pcm.data_ptr(), fr.data_ptr(), bg.data_ptr(), lm.data_ptr(), clips.data_ptr()
        bad = [
            (None, fb, F, None, n, G, M, B, L, 0, C, L, 2 * L),      # NULL buffers
            (P, fb, None, None, n, G, M, B, L, 0, C, L, 2 * L),
            (P, fb, F, None, n, None, M, B, L, 0, C, L, 2 * L),
            (P, fb, F, None, n, G, None, B, L, 0, C, L, 2 * L),
            (P, fb, F, None, n, G, M, B, L, 0, None, L, 2 * L),
            (P, fb, F, None, n, G, M, B, L, 2, C, L, 2 * L),         # unknown type
            (P, fb, F, None, n, G, M, B, 0, 0, C, L, 2 * L),         # clip_frames = 0
            (P, fb, F, None, n, G, M, B, L, 0, C + 2, L, 2 * L),     # d_clips not on an element boundary
            (P, fb, F, None, n, G, M, B, L, 0, C, L - 1, 2 * L),     # channel_stride < clip_frames
            (P, fb, F, None, n, G, M, B, L, 0, C, L, 2 * L - 1),     # clip_stride < channels * channel_stride
            (P, fb - 1, F, None, n, G, M, B, L, 0, C, L, 2 * L),     # pcm_stride below the frame bytes
            (P, fb, F, None, n, G, M, B, L, 0, C, L, 1 << 62),       # sizes that overflow
        ]
        for a in bad:
            with pytest.raises(ValueError):
                dec.clips_device(*a, None, None, True)
        with pytest.raises(ValueError):
            dec.clips_last_ms()  # no gather yet on this configuration
        dec.clips_device(None, 0, None, None, 0, None, None, 0, L, 0, None, 0, 0, None, None, True)  # no clips: nothing is touched
        assert bool((clips == 7.0).all().item())
        dec.clips_device(P, fb, F, None, 0, G, M, B, L, 0, C, L, 2 * L, valid.data_ptr(), None, True)  # no packets: zeros
        assert not clips[:B * 2 * L].any().item() and bool((clips[B * 2 * L:] == 7.0).all().item()) and not valid.any().item()


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 6, 512)])
def test_decode_clips_numpy_and_cuda_inputs(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    cfg = oracle.make_config(fl, depth, ch)
    packets = cr.packet_list(synth, helpers, cfg, 14, fl, damaged=4)
    blob, offs, sizes = helpers.pack_dense(packets)
    out, r_frames, r_status = oracle.decode_batch(cfg, np.concatenate([blob, np.zeros(64, np.uint8)]), offs, sizes, threads=8)
    offs1 = np.concatenate([offs, [offs[-1] + sizes[-1]]]).astype(np.uint64)
    n, L = len(packets), 3000
    begin = [0, fl - 1, 3 * fl + 7, (n - 1) * fl + 5, n * fl]
    limit = [n, n, 4, n, n]
    dev = torch.device("cuda:0")
    i64 = lambda v: torch.from_numpy(np.array(v, np.int64)).to(dev)  # noqa: E731
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg), 0) as dec:
        inputs = [
            (blob, offs, sizes, np.array(begin, np.uint64), np.array(limit, np.uint64)),
            (blob.tobytes(), offs1, None, begin, limit),
            (torch.from_numpy(blob).to(dev), i64(offs.astype(np.int64)), torch.from_numpy(sizes.astype(np.int32)).to(dev), i64(begin), i64(limit)),
        ]
        for bl, of, sz, bg, lm in inputs:
            for dtype, wtype in ((torch.float32, wr.FLOAT), (torch.int32, wr.INT)):
                clips, valid, cst, frames, status = dec.decode_clips(bl, of, sz, begin=bg, limit=lm, num_frames=L, dtype=dtype)
                assert clips.is_cuda and clips.dtype is dtype and valid.is_cuda and cst.is_cuda and tuple(clips.shape) == (5, ch, L)
                assert np.array_equal(status.cpu().numpy(), r_status) and np.array_equal(frames.cpu().numpy().view(np.uint32), r_frames)
                ref, r_valid, r_cst = cr.ref_clips(out, r_frames, r_status, fl, depth, ch, wtype, begin, limit, L)
                assert np.array_equal(clips.view(torch.int32).cpu().numpy().view(np.uint32), ref)
                assert np.array_equal(valid.cpu().numpy().view(np.uint32), r_valid) and np.array_equal(cst.cpu().numpy(), r_cst)
        # limit=None is n for every clip
        clips, valid, _, _, _ = dec.decode_clips(blob, offs, sizes, begin=begin, num_frames=L)
        ref, r_valid, _ = cr.ref_clips(out, r_frames, r_status, fl, depth, ch, wr.FLOAT, begin, [n] * 5, L)
        assert np.array_equal(clips.view(torch.int32).cpu().numpy().view(np.uint32), ref) and np.array_equal(valid.cpu().numpy(), r_valid)
        empty, valid, _, _, _ = dec.decode_clips(blob, offs, sizes, begin=[], num_frames=L)
        assert tuple(empty.shape) == (0, ch, L) and valid.numel() == 0
        with pytest.raises(ValueError):
            dec.decode_clips(blob, offs, sizes, begin=[0], num_frames=0)
        with pytest.raises(ValueError):
            dec.decode_clips(blob, offs, sizes, begin=[0, 1], limit=[1], num_frames=4)


# ---- load(frame_offset, num_frames) ------------------------------------------------------------------------------------------
FL = 4096


@pytest.fixture(scope="module")
def files(oracle, synth):
    """Three 16-bit stereo files of different lengths, each with a short last packet, and one of another bit depth."""
    cfg = oracle.make_config(FL, 16, 2)
    made = {}
    for name, n in (("a", 9), ("b", 4), ("c", 6)):
        packets = cr.file_packets(oracle, synth, cfg, n, n)
        made[name] = (packets, m4a.write_m4a(cfg, packets, per_chunk=[3, 2], gap=5))
    cfg24 = oracle.make_config(FL, 24, 2)
    made["d24"] = (None, m4a.write_m4a(cfg24, cr.file_packets(oracle, synth, cfg24, 3, 1)))
    return cfg, made


def same(torch, got, want):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype is want.dtype and got.is_cuda
    assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def ranges(total, n):
    """(frame_offset, num_frames): packet boundaries and those plus or minus one, the last frame, the end, past the end, -1."""
    last = (n - 1) * FL  # the short packet's first frame
    return [(0, 1), (0, FL), (0, FL + 1), (FL - 1, 1), (FL - 1, 2), (FL, FL), (FL + 1, FL - 1), (FL - 1, FL + 2), (3 * FL, 2 * FL + 1),
            (1, -1), (FL, -1), (last - 1, -1), (last, -1), (last + 1, 7), (total - 1, 1), (total - 1, 5), (total - 1, -1), (total, 1),
            (total, -1), (total + 1, 10), (n * FL, 3), (n * FL + 5, -1), (7, total - 7), (7, total), (0, total + FL), (5, 0)]


def test_ranged_load_equals_the_slice_of_the_full_load(torch, pkg, files, tmp_path):
    _, made = files
    packets, data = made["a"]
    path = tmp_path / "a.m4a"
    path.write_bytes(data)
    for dtype in (torch.float32, torch.int32):
        full, rate = pkg.load(data, dtype=dtype)
        total = full.shape[1]
        assert total % FL and total // FL == len(packets) - 1  # the last packet is short
        for a, b in ranges(total, len(packets)):
            want = full[:, a:] if b < 0 else full[:, a:a + b]
            got, sr = pkg.load(data, dtype=dtype, frame_offset=a, num_frames=b)
            assert sr == rate
            same(torch, got, want)
        same(torch, pkg.load(str(path), dtype=dtype, frame_offset=FL + 3, num_frames=2 * FL)[0], full[:, FL + 3:3 * FL + 3])
    with pytest.raises(ValueError):
        pkg.load(data, frame_offset=-1)
    with pytest.raises(ValueError):
        pkg.load(data, num_frames=-2)


def test_only_the_covering_packets_are_decoded(torch, pkg, files):
    cfg, made = files
    packets = list(made["a"][0])
    k = 5
    packets[k] = packets[k][:len(packets[k]) // 2]  # truncated: a bitstream overrun
    data = m4a.write_m4a(cfg, packets)
    good, _ = pkg.load(made["a"][1])
    with pytest.raises(pkg.ErrDecode) as full_err:
        pkg.load(data)
    assert "decoding packet %d" % k in str(full_err.value)
    # the damage lies outside these ranges
    same(torch, pkg.load(data, frame_offset=FL + 1, num_frames=4 * FL - 1)[0], good[:, FL + 1:5 * FL])
    same(torch, pkg.load(data, frame_offset=6 * FL, num_frames=-1)[0], good[:, 6 * FL:])
    # and inside these: the packet's index in the file, and the error load() raises
    for a, b in ((FL, 4 * FL + 1), (5 * FL + 100, 10), (6 * FL - 1, -1), (3, -1)):
        with pytest.raises(pkg.ErrDecode) as err:
            pkg.load(data, frame_offset=a, num_frames=b)
        assert str(err.value) == str(full_err.value) and err.value.status == full_err.value.status
    # a covering packet that lies outside the file (the mdat is the file's last box): what load() does about it
    cut = data[:len(data) - 10]
    with pytest.raises(pkg.AlacError, match="reading sample 9: unexpected EOF"):
        pkg.load(cut, frame_offset=6 * FL, num_frames=-1)
    same(torch, pkg.load(cut, frame_offset=6 * FL, num_frames=FL)[0], good[:, 6 * FL:7 * FL])


# ---- load_clips ---------------------------------------------------------------------------------------------------------------
def padded(torch, full, a, L):
    out = torch.zeros((full.shape[0], L), dtype=full.dtype, device=full.device)
    piece = full[:, a:a + L]
    out[:, :piece.shape[1]] = piece
    return out, piece.shape[1]


def clip_plan(fulls):
    """(source key, frame offset) per clip: three files, "a" repeated, boundaries, a clip over a file's end and one past it."""
    ta, tb, tc = (fulls[k].shape[1] for k in "abc")
    return [("a", 0), ("b", FL - 1), ("a", 3 * FL + 5), ("c", tc - 100), ("a", ta - 1), ("b", tb), ("b", tb + 3 * FL), ("c", 1),
            ("a", 2 * FL), ("c", 6 * FL + 1)]


def test_load_clips_over_files_of_different_lengths(torch, pkg, files, tmp_path):
    _, made = files
    path = tmp_path / "c.m4a"
    path.write_bytes(made["c"][1])
    L = FL + 1000
    for dtype in (torch.float32, torch.int32):
        fulls = {k: pkg.load(made[k][1], dtype=dtype)[0] for k in "abc"}
        plan = clip_plan(fulls)
        srcs = {"a": made["a"][1], "b": made["b"][1], "c": str(path)}
        clips, lengths, rate = pkg.load_clips([srcs[k] for k, _ in plan], [a for _, a in plan], L, dtype=dtype)
        assert tuple(clips.shape) == (len(plan), 2, L) and clips.dtype is dtype and clips.is_cuda
        assert lengths.is_cuda and lengths.dtype is torch.int32 and rate == 44100
        for j, (k, a) in enumerate(plan):
            want, real = padded(torch, fulls[k], a, L)
            same(torch, clips[j], want)
            assert int(lengths[j].item()) == real
        assert [int(x) for x in lengths.cpu()[[5, 6]]] == [0, 0] and 0 < int(lengths[3].item()) < L
    with pytest.raises(pkg.ErrConfig, match="source 2"):
        pkg.load_clips([made["a"][1], made["b"][1], made["d24"][1]], [0, 0, 0], 100)
    with pytest.raises(ValueError):
        pkg.load_clips([made["a"][1]], [0, 1], 100)


def test_load_clips_names_the_clip_and_the_packet_that_failed(torch, pkg, files):
    cfg, made = files
    packets = list(made["c"][0])
    packets[4] = packets[4][:len(packets[4]) // 2]
    bad = m4a.write_m4a(cfg, packets)
    good = made["a"][1]
    clips, lengths, _ = pkg.load_clips([good, bad, bad], [0, FL, 5 * FL + 1], 2 * FL)  # the damage lies between the clips
    assert [int(x) for x in lengths.cpu()][:2] == [2 * FL, 2 * FL]
    with pytest.raises(pkg.ErrDecode, match="clip 2: decoding packet 4: ") as err:
        pkg.load_clips([good, bad, bad, bad], [0, FL, 3 * FL + 9, 4 * FL], 2 * FL)
    assert err.value.status != 0 and err.value.sentinel == pkg.ErrBitstreamOverrun


def test_windows_of_a_few_packets(torch, pkg, files, monkeypatch):
    """The multi-window paths at small size: window_packets patched to 3 packets, as save()'s _window does for the encoder."""
    _, made = files
    stream = importlib.import_module("saprobe-alac_amd.stream")
    data = made["a"][1]
    full, _ = pkg.load(data)
    total = full.shape[1]
    fulls = {k: pkg.load(made[k][1])[0] for k in "abc"}
    plan = clip_plan(fulls)
    L = FL + 1000
    monkeypatch.setattr(stream, "window_packets", lambda frame_bytes: 3)
    for a, b in ((FL - 1, 7 * FL + 5), (5, -1), (3 * FL, 3 * FL), (2 * FL + 1, total), (total - 1, -1), (FL, 3 * FL)):
        same(torch, pkg.load(data, frame_offset=a, num_frames=b)[0], full[:, a:] if b < 0 else full[:, a:a + b])
    clips, lengths, _ = pkg.load_clips([made[k][1] for k, _ in plan], [a for _, a in plan], L)
    for j, (k, a) in enumerate(plan):
        want, real = padded(torch, fulls[k], a, L)
        same(torch, clips[j], want)
        assert int(lengths[j].item()) == real
    # one clip that alone is more than a window
    clips, lengths, _ = pkg.load_clips([data], [FL + 1], 5 * FL)
    same(torch, clips[0], full[:, FL + 1:6 * FL + 1])
    assert int(lengths[0].item()) == 5 * FL


def test_load_clips_refuses_a_truncated_file_anywhere_in_the_batch(torch, pkg, files):
    """A file whose last packet lies outside its bytes: clips that do not cover that packet are served; one that does raises
    load()'s EOF error with the clip in front, also when it is the first clip of the batch (its bytes must never run into
    the next clip's)."""
    _, made = files
    whole, other = made["a"][1], made["b"][1]
    cut = whole[:len(whole) - 10]  # packet 9 leaves the file
    got, lengths, _ = pkg.load_clips([cut, other, cut], [0, FL, 7 * FL], FL + 5)
    want, w_lengths, _ = pkg.load_clips([whole, other, whole], [0, FL, 7 * FL], FL + 5)
    same(torch, got, want)
    assert torch.equal(lengths, w_lengths)
    for srcs, where in (([cut, other, other], 0), ([other, cut, other], 1), ([other, other, cut], 2)):
        with pytest.raises(pkg.AlacError, match="clip %d: reading sample 9: unexpected EOF" % where):
            pkg.load_clips(srcs, [8 * FL + 7 if k == where else 0 for k in range(3)], FL)


def test_ranged_load_refuses_a_short_packet_in_front_of_the_last(torch, pkg, oracle, synth, files):
    """Frame offsets are packet arithmetic, which a short packet in the middle of a file breaks: ranges in front of it are
    served, a range that covers it raises instead of returning frames with other numbers than load()'s."""
    cfg, made = files
    packets = list(made["a"][0])
    packets[3] = cr.short_packet(synth, cfg, 1000, 3, escape=False)
    data = m4a.write_m4a(cfg, packets)
    full, _ = pkg.load(data)
    same(torch, pkg.load(data, frame_offset=5, num_frames=3 * FL - 5)[0], full[:, 5:3 * FL])
    for a, b in ((FL, 3 * FL), (3 * FL + 10, 5), (0, 4 * FL), (1, -1)):
        with pytest.raises(pkg.AlacError, match="packet 3 holds 1000 of 4096 frames"):
            pkg.load(data, frame_offset=a, num_frames=b)
