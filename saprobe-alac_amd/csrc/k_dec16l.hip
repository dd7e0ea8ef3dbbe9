/*
 * k_dec16l.hip — 16-bit streams, chanBits <= 23: the four-wave workgroups of k_dec16q.hip with queue buffers of 32 steps
 * instead of 16 (alac_duo.h: ALAC_DUO_CHUNK). The waves of a workgroup meet once per buffer (GpuWave::duo_sync: the LDS
 * counter drained, the barrier, the per-chunk entry tests of every role): 128 + 256 times per 4 096-frame pair instead of
 * 256 + 512. Same protocol, same double buffering, same groups of 8 steps and the same top-up period inside a chunk; the
 * writer wave holds 16 samples and 8 half-word U cells per chunk instead of 8 and 4.
 *
 * The queue is 16 KB here (2 buffers x 32 steps x 64 lanes x 4 bytes), the static LDS 34 KB: four of these workgroups fit a
 * CU and no fifth, nearly without a pad. So this kernel takes the "fit 4" launch of the batches that fill the device once,
 * one to four wave slots per CU (alacgpu.hip: long_chunks), and nothing else: the "fit 5" shape needs the 26 KB of
 * alac_decode_16q, and the batches of a workgroup or less per CU run predictor waves on several lanes per packet
 * (duo_phase_lanes), which hold a whole chunk's residuals in registers and are not instantiated here (ALAC_DECODE_NO_LANES).
 * A translation unit of its own: it compiles beside k_dec16q.hip, whose code object stays what it was.
 */
#define ALAC_LDS_ROWS 32
#define ALAC_LDS_FLUSH 32
#define ALAC_WRAP_COUNTDOWN 1
#define ALAC_DUO_CHUNK 32
/* the bitstream ring's three blocks at a channel's start in one trip to memory (alac_regular.h: RingRd::start) */
#define ALAC_RING_START_AHEAD 1
/* the entropy wave off the slow path at a packet's ends (alac_regular.h: ALAC_LEAN_ENDS; all three parts. A build with
 * EXTRA=-DALAC_LEAN_ENDS=<bits> has some of them, for A/Bs) */
#ifndef ALAC_LEAN_ENDS
#define ALAC_LEAN_ENDS 7
#endif
#include "alac_gpu.h"

#define ALAC_DECODE_KERNEL alac_decode_16l
#define ALAC_DECODE_WIDE 0
#define ALAC_DECODE_DEPTH 16
#define ALAC_DECODE_GATED 0
#define ALAC_DECODE_ROLES 4
#define ALAC_DECODE_WAVES 4 /* __launch_bounds__: waves per SIMD the register budget must allow */
#define ALAC_DECODE_NO_LANES 1 /* one predictor wave per workgroup, whatever the key */

namespace alack {

#include "k_decode_body.inc"

} /* namespace alack */
