/*
 * long_chunk_sim.cpp — TEST-ONLY host build of the kernel's decode logic, as chunk_sim.cpp (the int16-wrap test by countdown),
 * with queue buffers of 32 steps (alac_duo.h: ALAC_DUO_CHUNK 32, as k_dec16l.hip sets it): 32 steps per chunk where the
 * predictor role hands U over, 16 where a writer role takes half of each buffer. Same entry point (lane_sim_decode_batch),
 * another library: tests/test_long_chunks_host.py runs its cases through it. One lane playing every role in turn: the
 * barriers are no-ops and the stager writes straight to the PCM slot, so the rows, the rendezvous and the wave-wide maximum
 * of the countdown are the GPU tests' business (tests/test_gpu_long_chunks.py).
 */
#define ALAC_WRAP_COUNTDOWN 1
#define ALAC_DUO_CHUNK 32
#define ALAC_RING_START_AHEAD 1 /* (alac_regular.h: RingRd::start asks for its three blocks at once, as in k_dec16l.hip) */
#include "lane_sim.cpp"

/* what the build was made with (the test asserts it: a second copy of chunk_sim would pass every comparison too) */
extern "C" uint32_t long_chunk_sim_steps(void) { return alac::DUO_CHUNK; }
