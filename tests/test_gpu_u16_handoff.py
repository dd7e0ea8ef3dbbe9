"""The half-word U hand-off and the whole-chunk writer of 16-bit pairs (alac_duo.h, alac_decode_16q) on the GPU, against the
oracle: PCM bytes, frame counts and status words, always through the C ABI's device entry.

The sets (tests/u16_handoff_cases.py) are 64-512 packets. ALACGPU_PPW=64 fills the wave slots with them (the library's own
choice for so few packets is one packet per slot), so that the 64 lanes of a workgroup hold the mixture a set is about:
matrixed lanes beside mixRes 0 lanes, short packets beside full ones, a damaged packet beside good ones. One batch of 40
packets runs with slots of 32 and of one packet: there the predictor waves take four lanes per packet."""
import numpy as np
import pytest

from tests import u16_handoff_cases as cases

pytestmark = pytest.mark.gpu

LEAD, TAIL = 64, 320


@pytest.fixture(scope="module")
def torch(pkg):
    import importlib
    t = importlib.import_module("torch")
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)


def decode_and_check(torch, pkg, oracle, helpers, cfg, packets, what, stride=None, offset=0, expect_16q=True, lanes=0):
    """Decode into a buffer filled with a pattern: status, frame counts and the frames' PCM are the oracle's; every other
    byte (behind a packet's frames, between the slots, in front of the first and behind the last) is the pattern's. A
    failing packet's own slot is unspecified. -> the oracle's (out, frames, status)."""
    blob, offs, sizes = helpers.pack_dense(packets)
    ref = oracle.decode_batch(cfg, *helpers.pack_packets(packets), threads=8)
    out, rframes, rstatus = ref
    n, fb = out.shape
    stride = stride or fb
    lead = LEAD + offset
    pat = pattern(lead + n * stride + TAIL)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
    d_off = torch.from_numpy(np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.int64)).to(dev)
    d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)
    d_buf = torch.from_numpy(pat).to(dev)
    d_fr = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        dec.decode_batch_device(d_blob.data_ptr(), len(blob), d_off.data_ptr(), d_sz.data_ptr(), n, d_buf.data_ptr() + lead,
                                stride, d_fr.data_ptr(), d_st.data_ptr(), sync=True)
        disp = dec.last_dispatch()
    got, frames, status = d_buf.cpu().numpy(), d_fr.cpu().numpy().view(np.uint32), d_st.cpu().numpy()
    if expect_16q:
        assert disp["narrow_kernel"] == "alac_decode_16q" and disp["narrow_slots"] > 0, disp
        assert disp["lanes_per_packet"] == lanes, disp  # which form of the predictor wave wrote the tile
    assert np.array_equal(status, rstatus), "%s: status differs at %s" % (what, np.nonzero(status != rstatus)[0][:8])
    assert np.array_equal(frames, rframes), "%s: frame count differs at %s" % (what, np.nonzero(frames != rframes)[0][:8])
    exp = pat.copy()
    e = exp[lead:lead + n * stride].reshape(n, stride)
    g = got[lead:lead + n * stride].reshape(n, stride)
    have = np.arange(fb)[None, :] < (rframes.astype(np.int64) * 4)[:, None]
    e[:, :fb] = np.where(have, out, e[:, :fb])
    bad = rstatus != 0
    e[bad, :fb] = g[bad, :fb]
    diff = np.nonzero(got != exp)[0]
    if len(diff):
        i, c = divmod(int(diff[0]) - lead, stride)
        raise AssertionError("%s: %d bytes differ, first at slot %d byte %d (%d frames, status %#x): %d, want %d" % (
            what, len(diff), i, c, rframes[i] if 0 <= i < n else -1, rstatus[i] if 0 <= i < n else -1, got[diff[0]], exp[diff[0]]))
    return ref


@pytest.fixture
def full_slots(monkeypatch):
    monkeypatch.setenv("ALACGPU_PPW", "64")
    # one lane per packet in the predictor wave (duo_phase), the form large batches run: so few slots would otherwise get
    # predictor waves on several lanes per packet (k_decode_body.inc: lanes_ok) for every order from 4 up
    monkeypatch.setenv("ALACGPU_LANES_MIN", "17")
    monkeypatch.delenv("ALACGPU_FIT", raising=False)
    return monkeypatch


@pytest.mark.parametrize("order", [4, 6, 8, 12])
def test_u_outside_int16(torch, pkg, oracle, synth, helpers, full_slots, order):
    """Anti-phase full-scale pairs, mixRes 0 / 1 / 2 / 255 with mixBits 0 / 1 / 2, all of one key (128 packets): U needs 17
    bits and only its low halves cross the tile; L and R wrap through the 16-bit boundary both ways."""
    cfg = oracle.make_config(4096, 16, 2)
    packets = cases.antiphase_set(synth, cfg, order=order, per_mix=10)
    assert len(packets) == 128
    ref = decode_and_check(torch, pkg, oracle, helpers, cfg, packets, "antiphase order %d" % order)
    assert (ref[2] == 0).all()
    wide = sum(int((u > 32767).any() and (u < -32768).any())
               for res in (2, -1) for i in range(len(packets))
               for u in [cases.u_samples(ref[0][i].tobytes(), 4096, res, 0)])
    assert wide >= 2


@pytest.mark.parametrize("order", [4, 12])
def test_both_lane_forms_write_the_tile(torch, pkg, oracle, synth, helpers, full_slots, order):
    """ALACGPU_LANES_MIN=3: every key of these sets gets predictor waves on several lanes per packet: two with full slots,
    four with slots of 32 packets and of one (a batch of 40)."""
    full_slots.setenv("ALACGPU_LANES_MIN", "3")
    cfg = oracle.make_config(4096, 16, 2)
    packets = cases.frame_count_set(synth, cfg, order=order, n=128)
    decode_and_check(torch, pkg, oracle, helpers, cfg, packets, "two lanes, order %d" % order, lanes=2)
    full_slots.setenv("ALACGPU_PPW", "32")
    decode_and_check(torch, pkg, oracle, helpers, cfg, packets[:40], "four lanes, slots of 32, order %d" % order, lanes=4)
    full_slots.delenv("ALACGPU_PPW")
    decode_and_check(torch, pkg, oracle, helpers, cfg, packets[:40], "four lanes, one packet per slot, order %d" % order, lanes=4)


def test_small_batch_with_the_default_lanes(torch, pkg, oracle, synth, helpers, full_slots):
    """40 packets as the library lays them out by itself (ppw < 64; order 12: four lanes per packet)."""
    full_slots.delenv("ALACGPU_PPW")
    full_slots.delenv("ALACGPU_LANES_MIN")
    cfg = oracle.make_config(4096, 16, 2)
    decode_and_check(torch, pkg, oracle, helpers, cfg, cases.frame_count_set(synth, cfg, order=12, n=40), "40 packets", lanes=4)


@pytest.mark.parametrize("fl", [4096, 1000])
def test_frame_counts_in_one_workgroup(torch, pkg, oracle, synth, helpers, full_slots, fl):
    """1, 2, 7, 8, 9, 15, 16, 17, fl - 1 and fl frames, short and full packets in the same workgroup (odd step counts: the
    lone last U store; frames that end at an odd index, inside, at the end of and one past the writer's chunk), at a
    stride larger than the frame bytes; and a set without any full packet."""
    cfg = oracle.make_config(fl, 16, 2)
    fb = fl * 4
    ref = decode_and_check(torch, pkg, oracle, helpers, cfg, cases.frame_count_set(synth, cfg, n=128), "frame counts fl %d" % fl,
                           stride=(fb + 15) // 16 * 16 + 16)
    assert (ref[2] == 0).all() and len(np.unique(ref[1])) >= 10
    decode_and_check(torch, pkg, oracle, helpers, cfg, cases.all_short_set(synth, cfg), "short packets fl %d" % fl)


def test_mixed_matrix_lanes(torch, pkg, oracle, synth, helpers, full_slots):
    cfg = oracle.make_config(4096, 16, 2)
    for order in (6, 8):
        decode_and_check(torch, pkg, oracle, helpers, cfg, cases.mixed_matrix_set(synth, cfg, order=order), "mixed, order %d" % order)


def test_output_footprint(torch, pkg, oracle, synth, helpers, full_slots):
    """The buffer is pre-filled; stride larger than the frame bytes. At a 16-byte aligned base the four-wave kernel runs and
    leaves the bytes behind each packet's frames and between the slots alone; at a misaligned base (offset 4) the batch
    takes the irregular kernels (alac_regular.h: classify_regular) and the same holds."""
    cfg = oracle.make_config(1000, 16, 2)
    packets = cases.frame_count_set(synth, cfg, order=6, n=192)
    decode_and_check(torch, pkg, oracle, helpers, cfg, packets, "aligned, gap 32", stride=4000 + 32)
    # slots that start 16, 48, 80 ... bytes into a 128-byte line: the writer's 128-byte row pieces straddle the lines
    decode_and_check(torch, pkg, oracle, helpers, cfg, packets, "aligned base + 16, stride 4000 + 48", stride=4000 + 48, offset=16)
    decode_and_check(torch, pkg, oracle, helpers, cfg, packets, "misaligned base", stride=4000 + 16, offset=4, expect_16q=False)


def test_damaged_packet_beside_good_ones(torch, pkg, oracle, synth, helpers, full_slots):
    cfg = oracle.make_config(4096, 16, 2)
    ref = decode_and_check(torch, pkg, oracle, helpers, cfg, cases.damaged_set(synth, cfg), "damaged")
    assert (ref[2] != 0).sum() >= 5 and (ref[2] == 0).sum() >= 50
