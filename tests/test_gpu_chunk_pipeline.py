"""The chunk pipeline of the wave workgroups on the GPU (alac_duo.h: queue buffers, the lags of the predictor and writer
waves, tails, the int16-wrap countdown), against the oracle: PCM bytes, frame counts and status words, always through the C
ABI's device entry.

The sets (tests/chunk_pipeline_cases.py) are 64-256 packets of 40 or 56 frames. ALACGPU_PPW=64 fills the wave slots with
them (the library's own choice for so few packets is one packet per slot), so that the 64 lanes of a workgroup hold the
mixture a set is about. Every set of a case goes through ONE handle, back to back."""
import numpy as np
import pytest

from tests import chunk_pipeline_cases as cases

pytestmark = pytest.mark.gpu

LEAD, TAIL = 64, 256


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


class Job:
    """One batch on the device: inputs, a pattern-filled output buffer, and the oracle's answer."""

    def __init__(self, torch, oracle, helpers, cfg, packets, what):
        self.what, self.cfg = what, cfg
        blob, offs, sizes = helpers.pack_dense(packets)
        self.ref = oracle.decode_batch(cfg, *helpers.pack_packets(packets), threads=8)
        self.n, self.fb = self.ref[0].shape
        self.stride = (self.fb + 15) // 16 * 16  # (a slot that is not 16-byte aligned sends the batch to the irregular kernels)
        self.nbytes = len(blob)
        self.pat = ((np.arange(LEAD + self.n * self.stride + TAIL, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)
        dev = torch.device("cuda:0")
        self.d_blob = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
        self.d_off = torch.from_numpy(np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.int64)).to(dev)
        self.d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)
        self.d_buf = torch.from_numpy(self.pat).to(dev)
        self.d_fr = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.d_st = torch.full((self.n,), -1, dtype=torch.int32, device=dev)

    def launch(self, dec, sync):
        dec.decode_batch_device(self.d_blob.data_ptr(), self.nbytes, self.d_off.data_ptr(), self.d_sz.data_ptr(), self.n,
                                self.d_buf.data_ptr() + LEAD, self.stride, self.d_fr.data_ptr(), self.d_st.data_ptr(), sync=sync)

    def check(self):
        """Status, frame counts and the frames' PCM are the oracle's; every other byte of the buffer is the pattern's."""
        out, rframes, rstatus = self.ref
        assert (rstatus == 0).all(), self.what
        got, frames, status = self.d_buf.cpu().numpy(), self.d_fr.cpu().numpy().view(np.uint32), self.d_st.cpu().numpy()
        assert np.array_equal(status, rstatus), "%s: status differs at %s" % (self.what, np.nonzero(status != rstatus)[0][:8])
        assert np.array_equal(frames, rframes), "%s: frame count differs at %s" % (self.what, np.nonzero(frames != rframes)[0][:8])
        bpf = self.cfg.num_channels * {16: 2, 20: 3, 24: 3, 32: 4}[self.cfg.bit_depth]
        exp = self.pat.copy()
        e = exp[LEAD:LEAD + self.n * self.stride].reshape(self.n, self.stride)
        have = np.arange(self.fb)[None, :] < (rframes.astype(np.int64) * bpf)[:, None]
        e[:, :self.fb] = np.where(have, out, e[:, :self.fb])
        diff = np.nonzero(got != exp)[0]
        if len(diff):
            i, c = divmod(int(diff[0]) - LEAD, self.stride)
            raise AssertionError("%s: %d bytes differ, first at slot %d byte %d (%d frames): %d, want %d" % (
                self.what, len(diff), i, c, rframes[i] if 0 <= i < self.n else -1, got[diff[0]], exp[diff[0]]))


def run_sets(torch, pkg, oracle, helpers, cfg, sets, kernel=None, lanes=None):
    """Every (name, packets) of `sets` through one handle: the first two batches without a host synchronisation between
    them, the rest one by one."""
    jobs = [Job(torch, oracle, helpers, cfg, packets, what) for what, packets in sets]
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        for k, job in enumerate(jobs):
            job.launch(dec, sync=k != 0 or len(jobs) == 1)
        dec.synchronize()
        disp = dec.last_dispatch()
    if kernel is not None:
        assert disp["narrow_kernel"] == kernel and disp["narrow_slots"] > 0, disp
    if lanes is not None:
        assert disp["lanes_per_packet"] == lanes, disp
    for job in jobs:
        job.check()


@pytest.fixture
def slots(monkeypatch):
    """Full wave slots from small batches; one lane per packet in the predictor wave unless a test asks otherwise."""
    monkeypatch.setenv("ALACGPU_PPW", "64")
    monkeypatch.setenv("ALACGPU_LANES_MIN", "17")
    monkeypatch.delenv("ALACGPU_FIT", raising=False)
    return monkeypatch


def tiled(synth, cfg, counts, order_u, order_v=None):
    """count_set with at most 14 different packets, repeated to the length of `counts` (a slot of 64 equal frame counts does
    not need 64 encodes)."""
    distinct = list(dict.fromkeys(counts))
    if len(distinct) > 2:
        return cases.count_set(synth, cfg, counts, order_u, order_v)
    made = {k: cases.count_set(synth, cfg, [k] * 4, order_u, order_v, seed=k) for k in distinct}
    seen = {k: 0 for k in distinct}
    out = []
    for k in counts:
        out.append(made[k][seen[k] % 4])
        seen[k] += 1
    return out


ORDER_KEYS = [(o, None) for o in cases.ORDERS] + [(12, 5), (4, 16)]
KERNELS = {16: "alac_decode_16q", 20: "alac_decode_24q", 24: "alac_decode_24q", 32: "alac_decode_32q"}


@pytest.mark.parametrize("depth,ch", [(16, 2), (16, 1), (20, 2), (24, 2), (24, 1), (32, 2)])
def test_frame_counts_around_the_chunks(torch, pkg, oracle, synth, helpers, slots, depth, ch):
    """Slots of 64 packets with 1 .. 33 frames each — every residue of the step count modulo 8 on both sides of one to four
    chunks; slots that hold 0, 1, 2 or 3 whole chunks, so that the predictor's and the writer's lag are longer than the
    stream — alone, mixed inside one slot, and one single-frame lane beside lanes with 33; every order class and pairs whose
    U and V orders differ; 64 packets per batch, and four slots at once for the mixed set."""
    cfg = oracle.make_config(40, depth, ch)
    for order_u, order_v in ORDER_KEYS:
        if order_v is not None and ch == 1:
            continue
        sets = [("%s, orders %d/%s" % (name, order_u, order_v), tiled(synth, cfg, counts, order_u, order_v))
                for name, counts in cases.slot_sets(64)]
        sets.append(("four slots, orders %d/%s" % (order_u, order_v), tiled(synth, cfg, cases.slot_sets(256)[-2][1], order_u, order_v)))
        run_sets(torch, pkg, oracle, helpers, cfg, sets, kernel=KERNELS[depth], lanes=0)


@pytest.mark.parametrize("ppw,lanes", [("64", 2), ("32", 4)])
@pytest.mark.parametrize("ch", [2, 1])
def test_frame_counts_with_several_lanes_per_packet(torch, pkg, oracle, synth, helpers, slots, ppw, lanes, ch):
    """The same slots with the two-lane and the four-lane predictor waves forced on for every order from 3 up
    (ALACGPU_LANES_MIN=3; four lanes: slots of 32 packets)."""
    slots.setenv("ALACGPU_LANES_MIN", "3")
    slots.setenv("ALACGPU_PPW", ppw)
    cfg = oracle.make_config(40, 16, ch)
    for order_u, order_v in [(4, None), (5, None), (6, None), (8, None), (12, None), (16, None), (12, 5)]:
        if order_v is not None and ch == 1:
            continue
        sets = [("%s, orders %d/%s, %d lanes" % (name, order_u, order_v, lanes), tiled(synth, cfg, counts, order_u, order_v))
                for name, counts in cases.slot_sets(int(ppw))]
        run_sets(torch, pkg, oracle, helpers, cfg, sets, kernel="alac_decode_16q", lanes=lanes)


def test_two_lane_waves_in_a_batch_of_full_slots(torch, pkg, oracle, synth, helpers, monkeypatch):
    """The same slots in batches of 16 500 packets, just over the 16 384 from which the library fills its slots with 64
    packets and every workgroup has both two-lane predictor waves at work: the frame counts of slot_sets (mixed, and one
    single-frame lane beside lanes with 33) for three keys, short packets and tails in every slot; then the wrap streams of
    order 12 beside far packets, at 56 frames."""
    monkeypatch.setenv("ALACGPU_LANES_MIN", "3")
    monkeypatch.delenv("ALACGPU_PPW", raising=False)
    monkeypatch.delenv("ALACGPU_FIT", raising=False)
    cfg = oracle.make_config(40, 16, 2)
    pool = []
    for order_u, order_v in [(4, None), (12, None), (12, 5)]:
        for _, counts in cases.slot_sets(64)[-2:]:
            pool += tiled(synth, cfg, counts, order_u, order_v)
    run_sets(torch, pkg, oracle, helpers, cfg, [("16 500 packets of slot_sets", [pool[(i * 5) % len(pool)] for i in range(16500)])],
             kernel="alac_decode_16q", lanes=2)
    cfg = oracle.make_config(cases.WRAP_FRAMES, 16, 2)
    near, _ = cases.wrap_set(synth, cfg, 12)
    pool = near + cases.far_packets(synth, cfg, 12, 40, cases.WRAP_FRAMES)
    run_sets(torch, pkg, oracle, helpers, cfg, [("16 500 wrap and far packets", [pool[(i * 7) % len(pool)] for i in range(16500)])],
             kernel="alac_decode_16q", lanes=2)


@pytest.mark.parametrize("order", [5, 7, 12])
@pytest.mark.parametrize("ch", [2, 1])
def test_coefficients_through_the_int16_limits(torch, pkg, oracle, synth, helpers, slots, order, ch):
    """Streams whose coefficient starts 1, 7, 8, 9, 16, 40 (and a few more) steps from +32767 / -32768 and moves one step
    towards it per sample: the wrap falls in the first, the last and a middle step of a chunk, and in the chunk behind a
    stretch the countdown skipped. All of them in one slot; one such lane beside 63 whose coefficients are far from the
    limits; 63 such lanes beside one far one; and the same through the two- and four-lane predictor waves. The lane beside
    63 far ones is the only check anywhere of the countdown's wave-wide maximum (alac_gpu.h: max_u32): the host simulation
    has one lane, and its maximum is the identity."""
    cfg = oracle.make_config(cases.WRAP_FRAMES, 16, ch)
    near, where = cases.wrap_set(synth, cfg, order)
    if order != 5:
        assert {0, 7, 8, 15} <= where
    far = cases.far_packets(synth, cfg, order, 63, cases.WRAP_FRAMES)
    sets = [("wrap streams, order %d" % order, near),
            ("one near lane, order %d" % order, far[:20] + [near[3]] + far[20:]),
            ("one far lane, order %d" % order, [near[i % len(near)] for i in range(40)] + [far[0]] + [near[(i * 5) % len(near)] for i in range(23)])]
    run_sets(torch, pkg, oracle, helpers, cfg, sets, kernel="alac_decode_16q", lanes=0)
    slots.setenv("ALACGPU_LANES_MIN", "3")
    run_sets(torch, pkg, oracle, helpers, cfg, sets, kernel="alac_decode_16q", lanes=2)
    slots.setenv("ALACGPU_PPW", "32")
    run_sets(torch, pkg, oracle, helpers, cfg, [(w, p[:32]) for w, p in sets], kernel="alac_decode_16q", lanes=4)


@pytest.mark.parametrize("depth", [24, 32])
@pytest.mark.parametrize("order", [7, 12])
def test_wrap_streams_in_the_wider_kernels(torch, pkg, oracle, synth, helpers, slots, depth, order):
    """The same streams carried in the high bytes of 24- and 32-bit pairs (one and two shift bytes per sample): the wrap in
    alac_decode_24q / _32q, which keep the per-chunk test; near lanes alone, and one near lane beside 63 far ones."""
    cfg = oracle.make_config(cases.WRAP_FRAMES, depth, 2)
    near, where = cases.wrap_set(synth, cfg, order)
    assert {0, 7, 8, 15} <= where
    far = cases.far_packets(synth, cfg, order, 63, cases.WRAP_FRAMES)
    sets = [("wrap streams, %d-bit, order %d" % (depth, order), near),
            ("one near lane, %d-bit, order %d" % (depth, order), far[:20] + [near[3]] + far[20:])]
    run_sets(torch, pkg, oracle, helpers, cfg, sets, kernel=KERNELS[depth], lanes=0)


def test_wrap_streams_in_the_wave_pairs(torch, pkg, oracle, synth, helpers, monkeypatch):
    """The wrap in the kernels without a writer wave (per-chunk test): a batch large enough for the gated twin of 16-bit pairs
    (alac_decode_16g), its slots filled with the wrap streams of order 12 and far packets of the same key."""
    monkeypatch.delenv("ALACGPU_PPW", raising=False)
    monkeypatch.delenv("ALACGPU_FIT", raising=False)
    cfg = oracle.make_config(cases.WRAP_FRAMES, 16, 2)
    near, _ = cases.wrap_set(synth, cfg, 12)
    far = cases.far_packets(synth, cfg, 12, 40, cases.WRAP_FRAMES)
    pool = near + far
    packets = [pool[(i * 7) % len(pool)] for i in range(70000)]
    jobs = [Job(torch, oracle, helpers, cfg, packets, "70 000 packets")]
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        jobs[0].launch(dec, sync=True)
        disp = dec.last_dispatch()
    assert disp["narrow_kernel"] == "alac_decode_16g", disp
    jobs[0].check()
