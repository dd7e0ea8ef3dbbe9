"""The long-chunk form of the four-wave workgroups on the host: alac_duo.h's duo_phase with queue buffers of 32 steps
(ALAC_DUO_CHUNK 32, the setting of k_dec16l.hip; tests/host_sim/long_chunk_sim.cpp), one lane playing entropy, predictor and
writer role in turn, against the oracle: PCM bytes, frame counts and status. What depends on the chunk length is the whole-chunk
test of every role (steady_end, golomb_chunk, predict_chunk, emit_chunk16, fetch_u16), the writer's arrays, the lags of the
predictor and writer roles behind the entropy role, and the int16-wrap countdown (wrap_safe = D / CH). The packet sets are
tests/long_chunk_cases.py's, the same ones tests/test_gpu_long_chunks.py puts through the kernel."""
import ctypes

import numpy as np
import pytest

from tests import chunk_pipeline_cases as base
from tests import host_build
from tests import long_chunk_cases as cases


def build_long_chunk_sim():
    return host_build.shared("long_chunk_sim.cpp", "liblong_chunk_sim.so", host_build.SIM)


@pytest.fixture(scope="module")
def long_sim(oracle):
    """Host build with chunks of 32 steps, called like conftest's lane_sim (variant -1: the four-wave workgroups' roles)."""
    L = build_long_chunk_sim()
    vp = ctypes.c_void_p
    L.lane_sim_decode_batch.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp,
                                        ctypes.c_int, ctypes.c_int, vp, ctypes.c_int]

    def run(cfg, blob, offsets, sizes):
        n = len(offsets)
        stride = (oracle.frame_bytes(cfg) + 15) // 16 * 16
        out = np.zeros((n, stride), np.uint8)
        classes = np.zeros(n, np.uint32)
        fr = np.zeros(n, np.uint32)
        st = np.zeros(n, np.int32)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        rc = L.lane_sim_decode_batch(ctypes.byref(cfg), blob.ctypes.data, len(blob), offsets.ctypes.data, sizes.ctypes.data, n,
                                     out.ctypes.data, stride, fr.ctypes.data, st.ctypes.data, 1, -1, classes.ctypes.data, 1)
        assert rc == 0
        assert (classes < 2048).all()  # every packet took the wave workgroups' decoder (a regular key), none the whole-packet one
        return out, fr, st

    return run


def check(oracle, helpers, long_sim, cfg, packets, what):
    blob, offs, sizes = helpers.pack_packets(packets)
    ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=4)
    assert (ref[2] == 0).all(), what
    bpf = cfg.num_channels * oracle.bytes_per_sample(cfg.bit_depth)
    helpers.assert_same_decode(cfg, ref, long_sim(cfg, blob, offs, sizes), bpf, what)
    return ref


def test_the_build_has_chunks_of_32(long_sim):
    """The library under test is the 32-step form: a second copy of chunk_sim would pass every comparison below too."""
    L = build_long_chunk_sim()
    L.long_chunk_sim_steps.restype = ctypes.c_uint32
    assert L.long_chunk_sim_steps() == 32


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("order", cases.ORDERS)
def test_frame_counts_1_to_70(oracle, synth, helpers, long_sim, order, ch):
    """Partial frames of 1 .. 70: streams shorter than the predictor's and the writer's lag, zero, one and two whole 32-step
    chunks and up to four whole 16-step ones with tails of every length behind them; frames that end in the first, a middle
    and the last step of a chunk of either length."""
    for ends in cases.CHUNK_ENDS.values():
        assert set(ends) <= set(cases.COUNTS)
    cfg = oracle.make_config(cases.FRAMES, 16, ch)
    ref = check(oracle, helpers, long_sim, cfg, base.count_set(synth, cfg, cases.COUNTS, order), "order %d, %d ch" % (order, ch))
    assert list(ref[1]) == list(cases.COUNTS)


def test_pairs_whose_orders_differ(oracle, synth, helpers, long_sim):
    cfg = oracle.make_config(cases.FRAMES, 16, 2)
    for order_u, order_v in [(12, 5), (4, 16), (7, 31), (0, 12)]:
        check(oracle, helpers, long_sim, cfg, base.count_set(synth, cfg, cases.COUNTS, order_u, order_v), "orders %d / %d" % (order_u, order_v))


def test_long_packets_count_down_and_test_again(oracle, synth, helpers, long_sim):
    """Hundreds of chunks: the countdown runs out and the distance is looked at again, many times over a packet; frame counts
    that leave a tail of 31, 25 and 1 steps behind the last whole 32-step chunk."""
    for ch in (1, 2):
        cfg = oracle.make_config(4096, 16, ch)
        for order in (7, 12):
            check(oracle, helpers, long_sim, cfg, base.count_set(synth, cfg, (4096, 4095, 4089, 1025), order), "order %d" % order)


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("order", [5, 7, 12])
def test_coefficients_through_the_int16_limits(oracle, synth, helpers, long_sim, order, ch):
    """A coefficient that starts 1 .. 40 (and 57, 72, 100) steps from +32767 / -32768 and moves one step towards it per sample
    (tests/long_chunk_cases.py: wrap_specs): the wrap falls in every step of a 16-step chunk and in steps of the second, third
    and fourth 32-step chunk, behind stretches of one and two chunks that the countdown skipped. Order 5 keeps int32
    coefficients and walks on."""
    cfg = oracle.make_config(cases.LONG_WRAP_FRAMES, 16, ch)
    packets, where = cases.wrap_set(synth, cfg, order)
    if order == 12:
        assert {w % 16 for w in where} == set(range(16)) and {w // 32 for w in where} >= {1, 2, 3}, where
        assert {70, 85, 113} <= where  # behind the chunks the U phase's countdown skipped
    if order == 7:
        assert {w % 16 for w in where} == set(range(16)) and {65} <= where, where
    check(oracle, helpers, long_sim, cfg, packets, "order %d wrap streams" % order)
