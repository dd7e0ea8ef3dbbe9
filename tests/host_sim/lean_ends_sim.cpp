/*
 * lean_ends_sim.cpp — TEST-ONLY host build of the kernel's decode logic with long_chunk_sim.cpp's settings (the ones of
 * k_dec16l.hip) plus ALAC_LEAN_ENDS (alac_regular.h): the FAR form of the Golomb step while the packet's end is a chunk away,
 * the END form (the exact overrun test) from there on, the exact sample-end term, and the tail blocks of the bitstream ring
 * fetched whole before they are masked. Same entry point (lane_sim_decode_batch), another library:
 * tests/test_lean_ends_host.py runs its cases through it. One lane playing every role in turn, so "any lane within reach" is
 * this lane: which lanes of a wave choose the form of a chunk, and lanes that end in different steps of a group, are the GPU
 * tests' business (tests/test_gpu_lean_ends.py).
 */
#define ALAC_WRAP_COUNTDOWN 1
#define ALAC_DUO_CHUNK 32
#define ALAC_RING_START_AHEAD 1
#define ALAC_LEAN_ENDS 7
#include "lane_sim.cpp"

/* what the build was made with (the test asserts it: a copy of long_chunk_sim would pass every comparison too) */
extern "C" uint32_t lean_ends_sim_switch(void) { return ALAC_LEAN_ENDS; }
extern "C" uint32_t lean_ends_sim_steps(void) { return alac::DUO_CHUNK; }
