"""The half-word U hand-off and the whole-chunk writer of 16-bit pairs (alac_duo.h) as the host compiler builds them
(tests/host_sim/lane_sim.cpp: one lane plays entropy, predictor and writer wave in turn) against the oracle, on the packet
sets of tests/u16_handoff_cases.py. tests/test_gpu_u16_handoff.py runs the same sets through the kernels."""
import numpy as np
import pytest

from tests import u16_handoff_cases as cases


def run(oracle, lane_sim, helpers, cfg, packets, what, variant=-1):
    blob, offs, sizes = helpers.pack_packets(packets)
    ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=4)
    got = lane_sim(cfg, blob, offs, sizes, variant=variant, guard=True)
    helpers.assert_same_decode(cfg, ref, got, 4, what)
    return ref


@pytest.mark.parametrize("order", [4, 6, 8, 12])
def test_u_outside_int16(oracle, synth, lane_sim, helpers, order):
    """Anti-phase full-scale pairs for every mixRes / mixBits of the set: U needs 17 bits, L and R wrap through the 16-bit
    boundary both ways; only the low halves of U reach the writer."""
    cfg = oracle.make_config(4096, 16, 2)
    packets = cases.antiphase_set(synth, cfg, order=order, per_mix=3)
    ref = run(oracle, lane_sim, helpers, cfg, packets, "antiphase order %d" % order)
    assert (ref[2] == 0).all() and (ref[1] == 4096).all()
    # the generator reaches what it is for: with mixRes 2 / -1 and mixBits 0 the decoder's U leaves the int16 range
    wide = 0
    for res, sh in ((2, 0), (-1, 0)):
        for i in range(len(packets)):
            u = cases.u_samples(ref[0][i].tobytes(), 4096, res, sh)
            wide += int((u > 32767).any() and (u < -32768).any())
    assert wide >= 2


@pytest.mark.parametrize("fl", [4096, 1000])
def test_frame_counts_and_mixed_matrix(oracle, synth, lane_sim, helpers, fl):
    cfg = oracle.make_config(fl, 16, 2)
    ref = run(oracle, lane_sim, helpers, cfg, cases.frame_count_set(synth, cfg, n=64), "frame counts fl %d" % fl)
    assert (ref[2] == 0).all() and len(np.unique(ref[1])) >= 10
    run(oracle, lane_sim, helpers, cfg, cases.all_short_set(synth, cfg), "short packets fl %d" % fl)
    run(oracle, lane_sim, helpers, cfg, cases.mixed_matrix_set(synth, cfg, n=32), "mixed matrix fl %d" % fl)


def test_damaged_packets(oracle, synth, lane_sim, helpers):
    cfg = oracle.make_config(4096, 16, 2)
    ref = run(oracle, lane_sim, helpers, cfg, cases.damaged_set(synth, cfg, n=36), "damaged")
    assert (ref[2] != 0).sum() >= 3 and (ref[2] == 0).sum() >= 30


@pytest.mark.parametrize("fl", [4096, 1000])
def test_pair_form_without_a_writer_wave(oracle, synth, lane_sim, helpers, fl):
    """The same sets through variant -3 (alac_decode_16g's form: no writer wave, int32 U cells): the predictor wave writes the
    pairs at fixed places in chunks that every lane keeps whole, and a lane whose frames end inside a chunk writes its tail out
    right behind it."""
    cfg = oracle.make_config(fl, 16, 2)
    ref = run(oracle, lane_sim, helpers, cfg, cases.frame_count_set(synth, cfg, n=64), "frame counts fl %d" % fl, variant=-3)
    assert (ref[2] == 0).all() and len(np.unique(ref[1])) >= 10
    run(oracle, lane_sim, helpers, cfg, cases.all_short_set(synth, cfg), "short packets fl %d" % fl, variant=-3)
    run(oracle, lane_sim, helpers, cfg, cases.mixed_matrix_set(synth, cfg, n=32), "mixed matrix fl %d" % fl, variant=-3)
    ref = run(oracle, lane_sim, helpers, cfg, cases.damaged_set(synth, cfg, n=36), "damaged fl %d" % fl, variant=-3)
    assert (ref[2] != 0).sum() >= 3 and (ref[2] == 0).sum() >= 30
