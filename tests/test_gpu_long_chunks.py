"""The long-chunk form of the four-wave 16-bit decoder (k_dec16l.hip: alac_decode_16l, queue buffers of 32 steps) on the GPU,
against the oracle: PCM bytes, frame counts and status words, always through the C ABI's device entry, into a buffer filled
with a pattern (every byte outside the frames stays the pattern's).

The kernel takes the "fit 4" launch of batches that fill the device (alacgpu.hip: long_chunks): full 64-packet wave slots,
at least one per CU, one predictor wave per workgroup. The smallest such batch is 16 384 packets, where the library fills its
slots with 64 packets by itself; ALACGPU_LANES_MIN=17 keeps the predictor waves on one lane per packet there, the form every
larger batch runs (a batch of up to 9/8 slots per CU would otherwise give the keys with long predictors two predictor waves,
which is alac_decode_16q's business). The frame lengths are small — 96, 100 and 136 frames are three or four whole 32-step
chunks of the U phase and a tail — and the packets come from small pools (tests/long_chunk_cases.py, the sets the host model
decodes in tests/test_long_chunks_host.py), repeated with a stride so that every slot holds a mixture."""
import numpy as np
import pytest

from tests import chunk_pipeline_cases as base
from tests import long_chunk_cases as cases

pytestmark = pytest.mark.gpu

LEAD, TAIL = 64, 256
N = 16384
LONG, SHORT = "alac_decode_16l", "alac_decode_16q"


@pytest.fixture(scope="module")
def torch(pkg):
    import importlib
    t = importlib.import_module("torch")
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture
def one_predictor_wave(monkeypatch):
    monkeypatch.setenv("ALACGPU_LANES_MIN", "17")
    for name in ("ALACGPU_PPW", "ALACGPU_FIT", "ALACGPU_CHUNK"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


class Job:
    """One batch on the device: inputs, a pattern-filled output buffer, and the oracle's answer."""

    def __init__(self, torch, oracle, cfg, blob, offs, sizes, what):
        self.what, self.cfg = what, cfg
        self.ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=16)
        self.n, self.fb = self.ref[0].shape
        self.stride = (self.fb + 15) // 16 * 16 + 16  # a gap behind every slot: nothing may be written there
        self.nbytes = len(blob)
        self.pat = ((np.arange(LEAD + self.n * self.stride + TAIL, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)
        dev = torch.device("cuda:0")
        self.d_blob = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
        self.d_off = torch.from_numpy(np.concatenate([np.asarray(offs, np.uint64)[:self.n], [np.uint64(len(blob))]]).astype(np.int64)).to(dev)
        self.d_sz = torch.from_numpy(np.asarray(sizes).astype(np.int32)).to(dev)
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
        bpf = self.cfg.num_channels * 2
        exp = self.pat.copy()
        e = exp[LEAD:LEAD + self.n * self.stride].reshape(self.n, self.stride)
        have = np.arange(self.fb)[None, :] < (rframes.astype(np.int64) * bpf)[:, None]
        e[:, :self.fb] = np.where(have, out, e[:, :self.fb])
        diff = np.nonzero(got != exp)[0]
        if len(diff):
            i, c = divmod(int(diff[0]) - LEAD, self.stride)
            raise AssertionError("%s: %d bytes differ, first at slot %d byte %d (%d frames): %d, want %d" % (
                self.what, len(diff), i, c, rframes[i] if 0 <= i < self.n else -1, got[diff[0]], exp[diff[0]]))


def tiled_job(torch, oracle, helpers, cfg, pool, n, step, what):
    """n packets: pool[(i * step) % len(pool)] (step coprime to the pool's length: every slot of 64 gets a mixture)."""
    assert np.gcd(step, len(pool)) == 1
    blob, offs, sizes = helpers.pack_dense([pool[(i * step) % len(pool)] for i in range(n)])
    return Job(torch, oracle, cfg, blob, offs, sizes, what)


def run_jobs(torch, pkg, jobs, kernel, per_cu=None, irregular=False):
    """Every job through ONE handle: the first two back to back without a host synchronisation between them. -> the dispatch
    of the last one, which must name `kernel`."""
    torch.cuda.synchronize()
    disps = []
    with pkg.NewPacketDecoder(pkg_cfg(pkg, jobs[0].cfg)) as dec:
        for k, job in enumerate(jobs):
            job.launch(dec, sync=k != 0 or len(jobs) == 1)
            if k != 0 or len(jobs) == 1:
                disps.append(dec.last_dispatch())
        dec.synchronize()
        disps.append(dec.last_dispatch())
    for disp in disps:
        assert disp["narrow_kernel"] == kernel and disp["narrow_slots"] > 0 and not disp["gated"], disp
        assert disp["lanes_per_packet"] == 0 and (irregular or disp["irregular_slots"] == 0), disp
        if kernel == LONG:
            assert disp["packets_per_slot"] == 64 and disp["workgroups_per_cu"] == 4, disp
        if per_cu is not None:
            assert disp["workgroups_per_cu"] == per_cu, disp
    for job in jobs:
        job.check()
    return disps[-1]


def count_pool(synth, cfg, orders, counts):
    pool = []
    for order_u, order_v in orders:
        pool += base.count_set(synth, cfg, counts, order_u, order_v)
    return pool


@pytest.mark.parametrize("fl", [96, 100])
def test_frames_that_end_inside_a_chunk_beside_frames_that_fill_it(torch, pkg, oracle, synth, helpers, one_predictor_wave, fl):
    """Frame length 96: three whole 32-step chunks (six 16-step ones in the last channel); 100: a tail of 4 behind them. In
    every slot, packets with all their frames beside packets that end in the first, a middle and the last step of a chunk of
    either length, after one frame, and one step short of the frame length; every order class, and a pair whose orders
    differ. Two decodes back to back through one handle, then a third."""
    cfg = oracle.make_config(fl, 16, 2)
    counts = (fl, fl, fl, 1) + cases.CHUNK_ENDS[32] + cases.CHUNK_ENDS[16] + (fl - 1, 65, 70, 95)
    orders = [(o, None) for o in cases.ORDERS] + [(12, 5)]
    pool = count_pool(synth, cfg, orders, counts)
    jobs = [tiled_job(torch, oracle, helpers, cfg, pool, N, step, "fl %d, step %d" % (fl, step)) for step in (5, 11)]
    jobs.append(tiled_job(torch, oracle, helpers, cfg, pool[::-1], N, 13, "fl %d, reversed pool" % fl))
    disp = run_jobs(torch, pkg, jobs, LONG)
    assert disp["keys"] >= len(orders), disp
    assert (jobs[0].ref[1] == fl).sum() > N // 8 and (jobs[0].ref[1] < fl).sum() > N // 2


def test_mono(torch, pkg, oracle, synth, helpers, one_predictor_wave):
    """Single channels: no U phase; the writer wave's chunks are 16 steps of the only channel."""
    cfg = oracle.make_config(100, 16, 1)
    counts = (100, 100, 1) + cases.CHUNK_ENDS[16] + (33, 48, 99)
    pool = count_pool(synth, cfg, [(o, None) for o in cases.ORDERS], counts)
    run_jobs(torch, pkg, [tiled_job(torch, oracle, helpers, cfg, pool, N, 5, "mono")], LONG)


@pytest.mark.parametrize("ch", [2, 1])
def test_coefficients_through_the_int16_limits(torch, pkg, oracle, synth, helpers, one_predictor_wave, ch):
    """The wrap streams of tests/long_chunk_cases.py (a coefficient 1 .. 40, 57, 72, 100 steps from either int16 limit, orders
    7 and 12) in slots they share with packets of the same keys whose coefficients stay far from the limits: the countdown's
    distance is the wave's maximum, so a near lane among far ones must still stop it."""
    cfg = oracle.make_config(cases.LONG_WRAP_FRAMES, 16, ch)
    pool = []
    for order in (7, 12):
        near, where = cases.wrap_set(synth, cfg, order)
        assert where
        far = base.far_packets(synth, cfg, order, 23, cases.LONG_WRAP_FRAMES)
        pool += near + far
    jobs = [tiled_job(torch, oracle, helpers, cfg, pool, N, step, "wrap streams, %d ch, step %d" % (ch, step)) for step in (1, 5)]
    run_jobs(torch, pkg, jobs, LONG)


def test_the_five_keys_of_the_benchmark(torch, pkg, oracle, synth, helpers, one_predictor_wave):
    """The benchmark's packet mix (the synthesiser's music profile: predictors of 4, 5, 6, 8 and 12 taps) at 96 frames, twice
    through one handle."""
    cfg = oracle.make_config(96, 16, 2)
    jobs = []
    for seed in (11, 12):
        b = synth.gen_batch(cfg, N, profile=synth.PROFILE_MUSIC, base_seed=seed, threads=16, want_pcm=False)
        jobs.append(Job(torch, oracle, cfg, b.blob, b.offsets, b.sizes, "music profile, seed %d" % seed))
    disp = run_jobs(torch, pkg, jobs, LONG, irregular=True)  # (the profile has a few escape packets)
    assert disp["keys"] >= 5 and disp["irregular_slots"] <= 8, disp


def test_more_than_four_rounds_keep_the_short_chunks(torch, pkg, oracle, synth, helpers, one_predictor_wave):
    """131 072 packets of 40 frames: eight wave slots per CU of an MI355X run five workgroups per CU, which needs the 26 KB
    of alac_decode_16q: the dispatch names it, and the PCM is the oracle's."""
    n = 131072
    cfg = oracle.make_config(40, 16, 2)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * (n // 64) > 15 * n_cu, "the batch is sized for a device of up to 273 CUs"
    b = synth.gen_batch(cfg, n, profile=synth.PROFILE_MUSIC, base_seed=5, threads=16, want_pcm=False)
    run_jobs(torch, pkg, [Job(torch, oracle, cfg, b.blob, b.offsets, b.sizes, "131 072 packets")], SHORT, per_cu=5, irregular=True)


def test_small_batches_keep_the_short_chunks(torch, pkg, oracle, synth, helpers, one_predictor_wave):
    """Fewer wave slots than CUs: alac_decode_16q, as before (its predictor waves on several lanes per packet are not part of
    the long-chunk unit)."""
    cfg = oracle.make_config(100, 16, 2)
    one_predictor_wave.setenv("ALACGPU_PPW", "64")
    pool = count_pool(synth, cfg, [(12, None)], (100, 33, 64))
    run_jobs(torch, pkg, [tiled_job(torch, oracle, helpers, cfg, pool, 4096, 1, "4 096 packets")], SHORT, per_cu=4)
