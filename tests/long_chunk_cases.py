"""Packet sets for the long-chunk form of the four-wave workgroups (alac_duo.h: ALAC_DUO_CHUNK 32, k_dec16l.hip: 32 steps
per chunk in the U phase, 16 where the writer wave takes half of each queue buffer), 16-bit streams: shared by
tests/test_long_chunks_host.py (tests/host_sim/long_chunk_sim.cpp) and tests/test_gpu_long_chunks.py (the kernel). Built on
the generators of tests/chunk_pipeline_cases.py.

Every generator returns a list of packets (bytes) of one configuration; what they should decode to comes from the oracle."""
from tests import chunk_pipeline_cases as base

FRAMES = 72              # frame length of the count sets: partial frames of 1 .. 70
COUNTS = tuple(range(1, 71))
# frames that end in the first, a middle and the last step of a 32-step chunk (the second one: steps 32 .. 63) and of a
# 16-step chunk of the last channel (steps 16 .. 31), and one step on either side of the 32-step chunk
CHUNK_ENDS = {32: (33, 48, 64), 16: (17, 24, 32)}
ORDERS = (0, 31, 4, 5, 6, 8, 7, 12)  # copy, delta, the four int32 orders, a wrapping short one, a wrapping long one

LONG_WRAP_FRAMES = 136   # four whole 32-step chunks and a tail of 8: the longest stream order 12 keeps inside 16 bits both ways


def wrap_specs(order):
    """(start, upper, frames) of the wrap streams of an order: a coefficient 1 .. 40 steps from +32767 (upper) / -32768 when
    the warm-up ends, one step nearer with every sample. The wrap of start s falls at step order + 1 + s.

    In the U phase a chunk is 32 steps and the first whole steady one starts at step 32, where the coefficient is
    D = s - (31 - order) steps away: the countdown answers for D / 32 chunks. Starts 57, 72 and 100 (order 12: D = 38, 53,
    81) make it skip one chunk, one chunk, two chunks, and wrap in the chunk behind: a countdown that skips one chunk too
    many runs the wrapping step without the sign extension. In the last channel a chunk is 16 steps, the first steady one
    starts at step 16 (order 12) and starts from 35 on are skipped over in the same way. Streams of LONG_WRAP_FRAMES where
    the driven channel stays inside 16 bits that long (order 12 both ways, order 7 towards the lower limit up to 57), of
    WRAP_FRAMES otherwise: there the U phase has no whole steady chunk and the wrap meets the step-by-step path."""
    near = list(range(1, 41))
    if order == 12:
        return [(s, up, LONG_WRAP_FRAMES) for up in (True, False) for s in near + [57, 72, 100]]
    if order == 7:
        return [(s, False, LONG_WRAP_FRAMES) for s in near + [57]] + [(s, True, base.WRAP_FRAMES) for s in near]
    assert order in (4, 5, 6, 8)  # int32 coefficients: they walk on through the limit
    return [(s, up, base.WRAP_FRAMES) for up in (True, False) for s in (1, 8, 17, 40)]


def wrap_set(synth, cfg, order):
    """wrap_packet for every entry of wrap_specs(order); cfg.frame_length is LONG_WRAP_FRAMES, the shorter streams are
    partial frames. -> (packets, the wrapping steps)."""
    assert cfg.frame_length == LONG_WRAP_FRAMES and cfg.bit_depth == 16
    packets, where = [], set()
    for start, upper, frames in wrap_specs(order):
        pkt, wraps = base.wrap_packet(synth, cfg, order, start, upper, frames)
        if order in (4, 5, 6, 8):
            assert wraps == []
        else:
            assert wraps and wraps[0] == order + 1 + start, (order, start, upper, wraps)
        where |= set(wraps)
        packets.append(pkt)
    return packets, where
