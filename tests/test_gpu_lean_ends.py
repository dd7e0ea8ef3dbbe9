"""The entropy wave at a packet's ends (alac_regular.h: ALAC_LEAN_ENDS, on in k_dec16l.hip) on the GPU, against the oracle:
status words, frame counts and PCM bytes, through the C ABI's device entry into a pattern-filled guarded buffer, in the manner
of tests/test_gpu_long_chunks.py (whose Job and run_jobs these tests use). Every dispatch names alac_decode_16l.

What only a wave of 64 lanes shows: the form of a chunk's steps (FAR, or END with the exact overrun test) is chosen by ANY
lane that still decodes coming within reach of its packet's end, so lanes far from theirs run the END form beside lanes that
end; lanes end in different steps of a group and at different top-ups; a lane's ring block takes the tail form (eight fetches,
one wait, the masks) while its neighbours' do not. Batches of 16 384 packets, the smallest the kernel takes, with ALACGPU_LANES_MIN=17; pools
(tests/lean_ends_cases.py, the sets tests/test_lean_ends_host.py decodes on the host) tiled with a coprime stride, so that
every slot holds a mixture."""
import numpy as np
import pytest

from tests import lean_ends_cases as cases
from tests import test_gpu_long_chunks as lc

pytestmark = pytest.mark.gpu

N = lc.N
torch = lc.torch
one_predictor_wave = lc.one_predictor_wave


class FaultJob(lc.Job):
    """A batch that holds faulty packets: every status and frame count is the oracle's, the frames of every packet that
    decoded are the oracle's PCM, and nothing is written outside the slots (inside the slot of a packet that failed, the
    frames written before the fault was met are nobody's business)."""

    def check(self):
        out, rframes, rstatus = self.ref
        got, frames, status = self.d_buf.cpu().numpy(), self.d_fr.cpu().numpy().view(np.uint32), self.d_st.cpu().numpy()
        assert np.array_equal(status, rstatus), "%s: status differs at %s" % (self.what, np.nonzero(status != rstatus)[0][:8])
        assert np.array_equal(frames, rframes), "%s: frame count differs at %s" % (self.what, np.nonzero(frames != rframes)[0][:8])
        bpf = self.cfg.num_channels * 2
        exp = self.pat.copy()
        e = exp[lc.LEAD:lc.LEAD + self.n * self.stride].reshape(self.n, self.stride)
        g = got.copy()[lc.LEAD:lc.LEAD + self.n * self.stride].reshape(self.n, self.stride)
        have = np.arange(self.fb)[None, :] < (rframes.astype(np.int64) * bpf)[:, None]
        e[:, :self.fb] = np.where(have, out, e[:, :self.fb])
        failed = rstatus != 0
        e[failed, :self.fb] = g[failed, :self.fb]
        diff = np.nonzero(got != exp)[0]
        if len(diff):
            i, c = divmod(int(diff[0]) - lc.LEAD, self.stride)
            raise AssertionError("%s: %d bytes differ, first at slot %d byte %d: %d, want %d" % (
                self.what, len(diff), i, c, got[diff[0]], exp[diff[0]]))


def dense_job(torch, oracle, helpers, cfg, packets, what, lead=0, job=lc.Job):
    blob, offs, sizes = helpers.pack_dense(packets, lead=lead)
    assert len(blob) == int(offs[-1]) + int(sizes[-1])  # the blob tensor ends with the last packet's last byte
    return job(torch, oracle, cfg, blob, offs, sizes, what)


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("fl", [96, 136])
def test_valid_packets_of_mixed_endings(torch, pkg, oracle, synth, helpers, one_predictor_wave, fl, ch):
    """Frame counts fl - 7 .. fl (every step of the last group), quiet and loud signals, zero runs that start at the last
    samples or run to the end, escape codes as the last codes, bytes behind the END tag, V channels shorter than the reach:
    lanes of one wave come within reach at different top-ups and end in different steps of a group. Stereo and mono; two
    decodes back to back through one handle without a host synchronisation, then a third."""
    cfg = oracle.make_config(fl, 16, ch)
    pool = cases.crafted(synth, cfg, range(fl - 7, fl + 1))
    steps = [s for s in (5, 11, 13, 17, 19, 23) if np.gcd(s, len(pool)) == 1][:2]
    jobs = [dense_job(torch, oracle, helpers, cfg, cases.tile(pool, N, s), "fl %d, %d ch, stride %d" % (fl, ch, s), lead=k)
            for k, s in enumerate(steps)]
    jobs.append(dense_job(torch, oracle, helpers, cfg, cases.tile(pool[::-1], N, steps[0]), "fl %d, %d ch, reversed" % (fl, ch), lead=3))
    disp = lc.run_jobs(torch, pkg, jobs, lc.LONG, irregular=True)  # (the shortest packets of short_v are not regular)
    assert disp["narrow_slots"] > 200, disp  # of 256
    fr = jobs[0].ref[1]
    assert {int(f) % 8 for f in fr if f > fl - 8} == set(range(8))


@pytest.mark.parametrize("profile", ["PROFILE_MUSIC", "PROFILE_QUIET"])
def test_long_packets_run_far_from_their_end_first(torch, pkg, oracle, synth, helpers, one_predictor_wave, profile):
    """1 024-frame packets of the synthesiser's music and quiet profiles (the packets of the other tests are shorter than the
    FAR form's reach and run the END form from their first chunk): dozens of chunks in the FAR form, the change to the END
    form where the first lane of a wave comes within a chunk of its packet's end, lanes with fewer frames beside them."""
    cfg = oracle.make_config(1024, 16, 2)
    b = synth.gen_batch(cfg, N, profile=getattr(synth, profile), base_seed=21, threads=16, want_pcm=False)
    assert np.median(b.sizes) * 8 > 4 * 72 * 32
    job = lc.Job(torch, oracle, cfg, b.blob, b.offsets, b.sizes, "1 024 frames, %s" % profile)
    lc.run_jobs(torch, pkg, [job], lc.LONG, irregular=True)  # (the profiles have a few escape packets)


@pytest.mark.parametrize("ch", [2, 1])
def test_faulty_packets_among_valid_ones(torch, pkg, oracle, synth, helpers, lane_sim, one_predictor_wave, ch):
    """The prefixes that cut the last 64 bytes of a few valid packets and the one-bit faults of their last 8 bytes, those that
    classify_regular (the host build's) still calls regular, one in four among valid packets: every status is the oracle's
    and every valid neighbour's PCM intact."""
    cfg = oracle.make_config(96, 16, ch)
    pool = cases.crafted(synth, cfg, (89, 93, 96))
    faults = cases.end_faults(pool[::11])
    blob, offs, sizes = helpers.pack_dense(faults)
    keys = lane_sim(cfg, blob, offs, sizes, variant=-1, want_classes=True)[3]
    faults = [p for p, k in zip(faults, keys) if k < 2048]
    assert len(faults) > 500
    mixed = []
    for i in range(N):
        mixed.append(faults[(i // 4 * 7) % len(faults)] if i % 4 == 1 else pool[(i * 5) % len(pool)])
    job = dense_job(torch, oracle, helpers, cfg, mixed, "faults among valid packets, %d ch" % ch, lead=2, job=FaultJob)
    assert (job.ref[2] != 0).sum() > N // 16 and (job.ref[2] == 0).sum() > N // 2
    lc.run_jobs(torch, pkg, [job], lc.LONG, irregular=True)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_alignment_of_the_last_packet(torch, pkg, oracle, synth, helpers, one_predictor_wave, lead):
    """Dense blobs whose first packet starts at every byte misalignment (and, the sizes being mixed, every other one at all
    of them); the blob tensor is exactly as long as the blob and its last packet is among the shortest: its tail blocks'
    clamped fetches end at the tensor's last dword."""
    cfg = oracle.make_config(96, 16, 2)
    pool = cases.crafted(synth, cfg, (90, 96))
    packets = cases.tile(pool, N - 1, 7 if np.gcd(7, len(pool)) == 1 else 11)
    shortest = sorted(cases.short_v(synth, cfg), key=len)
    packets.append(next(p for p in shortest if len(p) >= 16))
    job = dense_job(torch, oracle, helpers, cfg, packets, "lead %d" % lead, lead=lead)
    assert {int(o) % 4 for o in np.asarray(job.d_off.cpu())[:-1]} == {0, 1, 2, 3}
    lc.run_jobs(torch, pkg, [job], lc.LONG, irregular=True)


def test_small_batches_keep_alac_decode_16q(torch, pkg, oracle, synth, helpers, one_predictor_wave):
    """4 096 packets of the same pools: fewer wave slots than CUs, the kernel without the switch, the same answers."""
    cfg = oracle.make_config(96, 16, 2)
    one_predictor_wave.setenv("ALACGPU_PPW", "64")
    pool = cases.zero_run_endings(synth, cfg, (89, 96)) + cases.escape_endings(synth, cfg, (89, 96))
    job = dense_job(torch, oracle, helpers, cfg, cases.tile(pool, 4096, 5 if np.gcd(5, len(pool)) == 1 else 7), "4 096 packets")
    lc.run_jobs(torch, pkg, [job], lc.SHORT, per_cu=4)
