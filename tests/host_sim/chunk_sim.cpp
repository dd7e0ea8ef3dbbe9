/*
 * chunk_sim.cpp — TEST-ONLY host build of the kernel's decode logic, as lane_sim.cpp, with the int16-wrap test of the
 * wrapping predictor orders run by countdown (alac_duo.h: ALAC_WRAP_COUNTDOWN 1, as k_dec16q.hip sets it). lane_sim.cpp
 * itself builds the per-chunk test the other units keep. Same entry point (lane_sim_decode_batch), another library:
 * tests/test_chunk_pipeline_host.py runs its cases through both. One lane: the wave-wide maximum of the countdown's
 * distance is the identity here; lanes near and far from the limits side by side are the GPU tests' business.
 */
#define ALAC_WRAP_COUNTDOWN 1
#include "lane_sim.cpp"
