"""The chunk pipeline of the wave workgroups on the host: alac_duo.h's duo_phase with one lane playing entropy, predictor
and writer role in turn (variant -1: the four-wave workgroups' instantiations, -3: the wave pairs'), against the oracle: PCM
bytes, frame counts and status. Two builds of the same text: tests/host_sim/chunk_sim.cpp with the int16-wrap test by
countdown (ALAC_WRAP_COUNTDOWN 1, k_dec16q.hip's setting) and tests/host_sim/lane_sim.cpp with the per-chunk test of the
other units. The same packet sets as tests/test_gpu_chunk_pipeline.py (tests/chunk_pipeline_cases.py): frame counts on both
sides of one to four chunks for every order class, and coefficients driven through the int16 limits. One lane: the
countdown's wave-wide maximum is the identity here; what it does with lanes near and far from the limits side by side is
checked on the GPU only."""
import ctypes

import numpy as np
import pytest

from tests import chunk_pipeline_cases as cases
from tests import host_build


def build_chunk_sim():
    return host_build.shared("chunk_sim.cpp", "libchunk_sim.so", host_build.SIM)


@pytest.fixture(scope="module")
def chunk_sim(oracle):
    """Host build with the countdown (tests/host_sim/chunk_sim.cpp), called like conftest's lane_sim."""
    L = build_chunk_sim()
    vp = ctypes.c_void_p
    L.lane_sim_decode_batch.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp,
                                        ctypes.c_int, ctypes.c_int, vp, ctypes.c_int]

    def run(cfg, blob, offsets, sizes, variant=-1, guard=False):
        n = len(offsets)
        stride = (oracle.frame_bytes(cfg) + 15) // 16 * 16
        out = np.zeros((n, stride), np.uint8)
        classes = np.zeros(n, np.uint32)
        fr = np.zeros(n, np.uint32)
        st = np.zeros(n, np.int32)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        rc = L.lane_sim_decode_batch(ctypes.byref(cfg), blob.ctypes.data, len(blob), offsets.ctypes.data, sizes.ctypes.data, n,
                                     out.ctypes.data, stride, fr.ctypes.data, st.ctypes.data, 1, variant, classes.ctypes.data,
                                     1 if guard else 0)
        assert rc == 0
        return out, fr, st

    return run


@pytest.fixture
def sims(lane_sim, chunk_sim):
    return (("countdown", chunk_sim), ("per-chunk test", lane_sim))


def check(oracle, helpers, sims, cfg, packets, what):
    for name, sim in sims:
        check_one(oracle, helpers, sim, cfg, packets, "%s, %s" % (what, name))


def check_one(oracle, helpers, lane_sim, cfg, packets, what):
    blob, offs, sizes = helpers.pack_packets(packets)
    ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=4)
    assert (ref[2] == 0).all(), what
    bpf = cfg.num_channels * oracle.bytes_per_sample(cfg.bit_depth)
    helpers.assert_same_decode(cfg, ref, lane_sim(cfg, blob, offs, sizes, guard=True), bpf, what)
    if cfg.bit_depth == 16:
        helpers.assert_same_decode(cfg, ref, lane_sim(cfg, blob, offs, sizes, variant=-3), bpf, what + " (wave pair)")
    return ref


@pytest.mark.parametrize("depth,ch", [(16, 2), (16, 1), (20, 2), (24, 2), (32, 2), (32, 1)])
def test_frame_counts_around_the_chunks(oracle, synth, helpers, sims, depth, ch):
    """1 .. 33 frames (a stream shorter than the predictor's and the writer's lag; tails of every length behind one to four
    whole chunks) for every order class, and pairs whose U and V orders differ."""
    cfg = oracle.make_config(40, depth, ch)
    for order in cases.ORDERS:
        check(oracle, helpers, sims, cfg, cases.count_set(synth, cfg, cases.COUNTS, order), "order %d" % order)
    if ch == 2:
        check(oracle, helpers, sims, cfg, cases.count_set(synth, cfg, cases.COUNTS, 12, 5), "orders 12 / 5")
        check(oracle, helpers, sims, cfg, cases.count_set(synth, cfg, cases.COUNTS, 4, 16), "orders 4 / 16")


def test_long_packets_count_down_and_test_again(oracle, synth, helpers, sims):
    """Hundreds of chunks: the countdown runs out and the distance is looked at again, many times over a packet (coefficients
    a few thousand steps from the limits answer for a few hundred chunks of 8)."""
    for ch in (1, 2):
        cfg = oracle.make_config(4096, 16, ch)
        for order in (7, 12):
            check(oracle, helpers, sims, cfg, cases.count_set(synth, cfg, (4096, 4095, 4089, 1025), order), "order %d" % order)


@pytest.mark.parametrize("order", [5, 7, 12])
@pytest.mark.parametrize("depth,ch", [(16, 1), (16, 2), (24, 2), (32, 2)])
def test_coefficients_through_the_int16_limits(oracle, synth, helpers, sims, order, depth, ch):
    """A coefficient that starts 1 .. 40 steps below +32767 / above -32768 and moves one step towards it per sample: the
    wrap (orders 7 and 12; order 5 keeps int32 coefficients and walks on) falls in the first, the last and a middle step of
    a chunk of 8 and of 16 steps, in the first steady chunk and in the one behind a stretch the countdown skipped. The
    generator's own model of where the wraps fall is checked against the reference's trace."""
    cfg = oracle.make_config(cases.WRAP_FRAMES, depth, ch)
    packets, where = cases.wrap_set(synth, cfg, order, check_trace=True)
    if order != 5:
        assert {0, 7, 8, 15} <= where and len(where) >= 6, where
    check(oracle, helpers, sims, cfg, packets, "order %d wrap streams" % order)
