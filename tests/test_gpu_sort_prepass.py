"""The sort pre-pass in two kernels (k_sort.hip): alac_classify ranks the packets inside their keys and its last block to
finish makes the plan from a histogram that lives in the handle's workspace from decode to decode; alac_scatter places the
packets by rank and zeroes the claim words. Checked here: batch sizes around the 256-thread block and the 64-packet wave slot,
batches with nothing to sort and with one key, the state a handle carries from one decode to the next (histogram, ticket, claim
and gate words), and the split pipeline's second sort. PCM, frame counts and status words are the oracle's, as in
tests/test_gpu_parity.py; every call goes through the C ABI."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FL = 64
ERR_RANGE = 7  # ALACGPU_ERR_RANGE
# (U order, V order): the benchmark batch's five keys and two with orders of their own per channel
ORDERS = [(4, 4), (5, 5), (6, 6), (8, 8), (12, 12), (4, 8), (12, 5)]


def _packets(synth, cfg, n, orders, seed, escape_every=0):
    """n 16-bit stereo packets whose keys cycle through `orders`; every escape_every-th is an escape packet (irregular)"""
    out = []
    for i in range(n):
        pcm = synth.signal(cfg, synth.PROFILE_MUSIC, seed * 100003 + i, cfg.frame_length)
        ou, ov = orders[i % len(orders)]
        esc = 1 if escape_every and i % escape_every == escape_every - 1 else 0
        e = synth.default_elem(order=ou, order_v=ov, force_escape=esc)
        out.append(synth.encode_packet(cfg, [e], pcm))
    return out


class _Job:
    """One device decode: the packets laid out densely, optional broken descriptors, the tensors it reads and writes"""

    def __init__(self, helpers, packets, far=(), fill=0xA5):
        import torch
        self.n = n = len(packets)
        blob, offs, sizes = helpers.pack_dense(packets, lead=1)
        self.far = list(far)
        for k in self.far:  # a descriptor that starts behind the blob
            offs[k] = len(blob) + 17
        dev = torch.device("cuda:0")
        self.blob_bytes = len(blob)
        self.d_blob = torch.from_numpy(blob).to(dev)
        self.d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        self.d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)
        self.stride = FL * 4
        self.fill = fill
        self.d_out = torch.full((n, self.stride), fill, dtype=torch.uint8, device=dev)
        self.d_fr = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def run(self, dec, sync=True):
        dec.decode_batch_device(self.d_blob.data_ptr(), self.blob_bytes, self.d_off.data_ptr(), self.d_sz.data_ptr(), self.n,
                                self.d_out.data_ptr(), self.stride, self.d_fr.data_ptr(), self.d_st.data_ptr(), sync=sync)

    def check(self, helpers, cfg, ref, what):
        """ref: the oracle's (out, frames, status) for the same packets, in order"""
        out, fr, st = self.d_out.cpu().numpy(), self.d_fr.cpu().numpy().astype(np.uint32), self.d_st.cpu().numpy()
        keep = np.ones(self.n, bool)
        keep[self.far] = False
        assert (st[~keep] == ERR_RANGE).all() and (fr[~keep] == 0).all(), what
        helpers.assert_same_decode(cfg, tuple(a[keep] for a in ref), (out[keep], fr[keep], st[keep]), 4, what)
        for i in np.nonzero(fr == 0)[0]:  # a packet without frames: nobody wrote to its slot
            assert (out[i] == self.fill).all(), "%s: packet %d has no frames, but bytes of its slot were written" % (what, i)


@pytest.fixture(scope="module")
def cfg16(oracle):
    return oracle.make_config(FL, 16, 2)


@pytest.fixture(scope="module")
def mixed(synth, oracle, helpers, cfg16):
    """1 000 packets of seven keys with escape packets among them and an empty one, and the oracle's decode of them; a batch of
    n packets is the first n (the tests leave both unchanged)"""
    packets = _packets(synth, cfg16, 1000, ORDERS, seed=1, escape_every=11)
    packets[2] = b""
    ref = oracle.decode_batch(cfg16, *helpers.pack_packets(packets), threads=8)
    assert ref[2][2] != 0 and (np.delete(ref[2], 2) == 0).all()
    return packets, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 1000])
def test_batch_sizes_around_the_block_and_the_wave_slot(gpu_decoder_factory, helpers, cfg16, mixed, n):
    packets, ref = mixed
    far = [n // 2] if n >= 63 else []  # (n // 2 is never the empty packet's index)
    job = _Job(helpers, packets[:n], far=far)
    with gpu_decoder_factory(cfg16) as dec:
        job.run(dec)
        disp = dec.last_dispatch()
    job.check(helpers, cfg16, tuple(a[:n] for a in ref), "n=%d" % n)
    if n >= 63:
        assert disp["keys"] >= 6 and disp["irregular_slots"] >= 1, disp


def test_nothing_to_sort_and_a_single_key(gpu_decoder_factory, synth, oracle, helpers, cfg16, mixed):
    packets, ref = mixed
    empty_status = int(ref[2][2])
    n = 300
    job = _Job(helpers, [packets[i] if i % 3 else b"" for i in range(n)], far=[i for i in range(n) if i % 3])
    with gpu_decoder_factory(cfg16) as dec:
        job.run(dec)
        disp = dec.last_dispatch()
        assert disp["keys"] == 0 and disp["slots"] == 0, disp
        st, fr = job.d_st.cpu().numpy(), job.d_fr.cpu().numpy()
        want = np.where(np.arange(n) % 3 != 0, ERR_RANGE, empty_status)
        assert np.array_equal(st, want) and (fr == 0).all()
        assert (job.d_out.cpu().numpy() == job.fill).all()  # no kernel wrote PCM
        # ... and the same handle right behind it, with a batch whose packets all share one key
        one = _packets(synth, cfg16, 300, [(6, 6)], seed=2)
        job1 = _Job(helpers, one)
        job1.run(dec)
        disp = dec.last_dispatch()
        assert disp["keys"] == 1 and disp["slots"] == disp["narrow_slots"] > 0, disp
    job1.check(helpers, cfg16, oracle.decode_batch(cfg16, *helpers.pack_packets(one), threads=8), "one key")


def test_state_carried_between_decodes_on_one_handle(pkg, gpu_decoder_factory, synth, oracle, helpers, cfg16):
    """Batches whose key sets differ, back to back without a synchronisation between them: a count, a ticket, a claim or a gate
    word that one decode left behind would show as a wrong pkt_start or an undecoded wave slot in the next."""
    batches = [_packets(synth, cfg16, 300, [(4, 4), (5, 5)], seed=3),
               _packets(synth, cfg16, 513, [(8, 8), (12, 12), (4, 8)], seed=4, escape_every=9),
               _packets(synth, cfg16, 100, [(6, 6), (12, 5)], seed=5, escape_every=4)]
    refs = [oracle.decode_batch(cfg16, *helpers.pack_packets(p), threads=8) for p in batches]
    order = [0, 1, 2, 0]
    with gpu_decoder_factory(cfg16) as dec:
        jobs = [_Job(helpers, batches[k]) for k in order]
        for job in jobs:
            job.run(dec, sync=False)
        dec.synchronize()
        for j, (k, job) in enumerate(zip(order, jobs)):
            job.check(helpers, cfg16, refs[k], "decode %d of four (batch %d)" % (j, k))
        # a call that is refused for its arguments, then a decode
        bad = _Job(helpers, batches[1])
        bad.stride = 8  # less than a frame's bytes
        with pytest.raises(Exception):
            bad.run(dec)
        again = _Job(helpers, batches[1])
        again.run(dec)
        again.check(helpers, cfg16, refs[1], "behind a refused call")
    with gpu_decoder_factory(cfg16) as dec:  # the handle taken back from the pool
        job = _Job(helpers, batches[2])
        job.run(dec)
        job.check(helpers, cfg16, refs[2], "pooled handle")
        job = _Job(helpers, batches[0])
        job.run(dec)
        job.check(helpers, cfg16, refs[0], "pooled handle, second decode")


@pytest.mark.parametrize("depth,ch,n", [(24, 8, 300), (16, 6, 300)])
def test_split_pipeline_second_sort(gpu_decoder_factory, synth, oracle, helpers, depth, ch, n):
    """More than two channels: the channel tasks are sorted by a second pass of the same two kernels, through the same
    histogram and ranks as the packets'. Twice on one handle, then a smaller batch."""
    cfg = oracle.make_config(128, depth, ch)
    bpf = ch * oracle.bytes_per_sample(depth)
    b = synth.gen_batch(cfg, n, profile=synth.PROFILE_STRESS, threads=8)
    ref = oracle.decode_batch(cfg, b.blob, b.offsets, b.sizes, threads=8)
    pk = [b.packet(i) for i in range(b.n)]

    def host_entry(dec, packets):  # alacgpu_decode_batch on the packets back to back
        offs = np.zeros(len(packets) + 1, np.uint64)
        offs[1:] = np.cumsum([len(p) for p in packets], dtype=np.uint64)
        return dec.decode_batch(np.frombuffer(b"".join(packets), np.uint8), offs)

    with gpu_decoder_factory(cfg) as dec:
        for rnd in range(2):
            helpers.assert_same_decode(cfg, ref, host_entry(dec, pk), bpf, "%d channels, decode %d" % (ch, rnd))
        helpers.assert_same_decode(cfg, tuple(a[:70] for a in ref), host_entry(dec, pk[:70]), bpf, "%d channels, 70 packets" % ch)
