/*
 * alacgpu.h — C ABI of the MI355X (gfx950) batch ALAC packet decoder.
 *
 * This is the drop-in boundary for the reference's packet layer
 * (mycophonic/saprobe-alac, paths relative to the reference tree):
 *
 *   reference (Go)                                   this ABI
 *   ------------------------------------------------ ---------------------------
 *   PacketConfig            config.go:27-38          alacgpu_config
 *   PCMFormat               format.go:20-24          alacgpu_format
 *   NewPacketDecoder        decoder.go:90-109        alacgpu_create
 *   (*PacketDecoder).Format decoder.go:112-114       alacgpu_get_format
 *   (*PacketDecoder).DecodePacket  decoder.go:117-128  alacgpu_decode_packet
 *   decodePacketInto        decoder.go:133-207       alacgpu_decode_packet (caller buffer)
 *   DecodePackets (new batch entry, north star)      alacgpu_decode_batch / _device
 *   ErrDecode + internal sentinels errors.go:22-34,  alacgpu_status (per packet)
 *                           internal/alac/errors.go:24-33
 *
 * Plain pointers and sizes only; no C++ or torch types. All functions are
 * re-entrant across different handles; one handle is single-caller, like a
 * PacketDecoder (decoder.go:79-87 holds mutable scratch).
 *
 * There is NO CPU decode path behind this ABI: every decode entry runs the HIP
 * kernels on the handle's device and returns ALACGPU_E_HIP if that fails.
 */
#ifndef ALACGPU_H
#define ALACGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Mirrors PacketConfig (config.go:27-38) field for field. */
typedef struct alacgpu_config {
    uint32_t frame_length;    /* FrameLength   */
    uint8_t  bit_depth;       /* BitDepth: 16, 20, 24 or 32 */
    uint8_t  num_channels;    /* NumChannels: 1..8 */
    uint8_t  pb;              /* PB */
    uint8_t  mb;              /* MB */
    uint8_t  kb;              /* KB */
    uint8_t  reserved0;
    uint16_t max_run;         /* MaxRun (stored, never read by decode) */
    uint32_t max_frame_bytes; /* MaxFrameBytes */
    uint32_t avg_bit_rate;    /* AvgBitRate */
    uint32_t sample_rate;     /* SampleRate */
} alacgpu_config;

/* Mirrors PCMFormat (format.go:20-24). */
typedef struct alacgpu_format {
    int32_t sample_rate;
    int32_t bit_depth;
    int32_t channels;
} alacgpu_format;

/*
 * Per-packet status word (int32).
 *   bits 0..7   code      (alacgpu_code) — which internal sentinel
 *   bits 8..11  context   (alacgpu_ctx)  — the wrapping string the reference adds
 *   bits 12..13 stage     (alacgpu_stage)— "entropy decode" / "entropy decode U|V"
 * 0 means success. The Go shim rebuilds the reference's error chain from it:
 *   fmt.Errorf("%w: <ctx>: <stage>: %w", ErrDecode, <sentinel>)
 */
typedef enum alacgpu_code {
    ALACGPU_OK                     = 0,
    ALACGPU_ERR_BITSTREAM_OVERRUN  = 1, /* ErrBitstreamOverrun   internal/alac/errors.go:30 */
    ALACGPU_ERR_SAMPLE_OVERRUN     = 2, /* ErrSampleOverrun      internal/alac/errors.go:31 */
    ALACGPU_ERR_INVALID_HEADER     = 3, /* ErrInvalidHeader      internal/alac/errors.go:28 */
    ALACGPU_ERR_INVALID_SHIFT      = 4, /* ErrInvalidShift       internal/alac/errors.go:29 */
    ALACGPU_ERR_UNSUPPORTED_ELEMENT= 5, /* ErrUnsupportedElement internal/alac/errors.go:27 */
    ALACGPU_ERR_MALFORMED          = 6, /* input on which the Go reference panics (slice bounds);
                                           it has no defined result there, we return a status */
    ALACGPU_ERR_RANGE              = 7  /* batch entries only: the packet's offset / size does not lie inside the
                                           blob (no reference counterpart: a Go slice cannot be out of range) */
} alacgpu_code;

typedef enum alacgpu_ctx {
    ALACGPU_CTX_NONE = 0,
    ALACGPU_CTX_SCE  = 1, /* "SCE/LFE" decoder.go:156 */
    ALACGPU_CTX_CPE  = 2, /* "CPE"     decoder.go:173 */
    ALACGPU_CTX_DSE  = 3, /* "DSE"     decoder.go:184 */
    ALACGPU_CTX_FIL  = 4  /* "FIL"     decoder.go:189 */
} alacgpu_ctx;

typedef enum alacgpu_stage {
    ALACGPU_STAGE_NONE      = 0,
    ALACGPU_STAGE_ENTROPY   = 1, /* "entropy decode"   decoder.go:303 */
    ALACGPU_STAGE_ENTROPY_U = 2, /* "entropy decode U" decoder.go:468 */
    ALACGPU_STAGE_ENTROPY_V = 3  /* "entropy decode V" decoder.go:482 */
} alacgpu_stage;

#define ALACGPU_STATUS(code, ctx, stage) ((int32_t)((code) | ((ctx) << 8) | ((stage) << 12)))
#define ALACGPU_STATUS_CODE(s)  ((s) & 0xff)
#define ALACGPU_STATUS_CTX(s)   (((s) >> 8) & 0xf)
#define ALACGPU_STATUS_STAGE(s) (((s) >> 12) & 0x3)

/* Call-level return values (negative = the call itself failed). */
#define ALACGPU_E_OK        0
#define ALACGPU_E_CONFIG   -1  /* ErrConfig: unsupported bit depth (decoder.go:91-93) or
                                  NumChannels outside 1..8 (the reference index-panics at decoder.go:140) */
#define ALACGPU_E_ARG      -2  /* null pointer / capacity too small */
#define ALACGPU_E_HIP      -3  /* HIP runtime failure; see alacgpu_last_error */
#define ALACGPU_E_DECODE   -4  /* alacgpu_decode_packet only: packet failed, *status_out holds the word */

/* Packets may lie DENSELY in a blob, back to back and at any alignment — an mdat as it is in the file
 * (internal/mp4/mp4.go:382-420). The kernels treat every byte behind a packet's last one as zero (the reference pads
 * each packet with 4 zero bytes, bitbuffer.go:33) and never touch memory outside [blob, blob + blob_bytes) rounded out
 * to 4-byte words. Round 1 required 64 zero bytes behind every packet; padding is harmless but no longer needed. */
#define ALACGPU_PACKET_PAD 0

typedef struct alacgpu_decoder alacgpu_decoder;

/* NewPacketDecoder (decoder.go:90). device = HIP ordinal; one stream per handle. */
int alacgpu_create(const alacgpu_config* cfg, int device, alacgpu_decoder** out);
/* A destroyed handle's streams, events and small buffers are kept for the next alacgpu_create on the same device: a file
 * decoder makes and drops a handle per file (decode.go:50-80), and building one from nothing costs several times the
 * decode of a short file. Kept per handle: at most 2 GB of device memory (a handle's workspace is mostly the U hand-off
 * tiles, (frame_length + 1) x 256 bytes per wave slot: 1 GB for the 1 024-packet windows of a 24-bit file decoder, and
 * letting go of it means hipFree, which waits for the whole device) and 64 MB of pinned host memory (the largest buffers are
 * dropped first); four handles per device, so at most 8 GB of the device's 288 GB. alacgpu_trim() frees what is kept. */
void alacgpu_destroy(alacgpu_decoder* dec);
void alacgpu_trim(void);

/* Pinned (page-locked) host memory for the buffers a caller hands to alacgpu_decode_batch: what that entry finds in pinned
 * memory it transfers in place instead of through its own staging copies (a third of the time of a file decode goes into
 * those). NULL when the runtime refuses. Freed buffers of up to 64 MB are kept for the next alacgpu_host_alloc (the eight
 * newest, 192 MB in all; alacgpu_trim() frees them). */
void* alacgpu_host_alloc(size_t bytes);
void alacgpu_host_free(void* p);

/* (*PacketDecoder).Format (decoder.go:112). */
int alacgpu_get_format(const alacgpu_decoder* dec, alacgpu_format* fmt);

/* Bytes of one full decoded frame: FrameLength*NumChannels*BytesPerSample (decoder.go:120). */
size_t alacgpu_frame_bytes(const alacgpu_decoder* dec);

/*
 * DecodePacket / decodePacketInto (decoder.go:117,133): one packet, host buffers,
 * through the same HIP kernel as the batch entry (batch of 1). out_cap must be
 * >= alacgpu_frame_bytes(). *out_len = numSamples*numChan*bps (decoder.go:206).
 * Returns ALACGPU_E_DECODE and sets *status_out when the packet fails.
 */
int alacgpu_decode_packet(alacgpu_decoder* dec, const uint8_t* packet, size_t packet_len,
                          uint8_t* out, size_t out_cap, size_t* out_len, int32_t* status_out);

/*
 * DecodePackets, host buffers. Packet i is blob[offsets[i] .. offsets[i+1]) (dense, e.g. a whole mdat).
 * PCM of packet i is written at out + i*out_stride (out_stride >= frame bytes);
 * frames_out[i] = the packet's sample-frame count (0 on failure), status[i] = status word.
 * A failing packet's slot and the bytes of a slot behind a partial frame read as zero (decoder.go:120,127: DecodePacket
 * hands back a prefix of a zeroed frame buffer); a failing packet does not affect others. Only [0, frame bytes) of a slot
 * is written: the bytes [frame bytes, out_stride) of every slot, and everything in front of the first slot or behind the
 * last one, stay the caller's.
 * The batch is cut into chunks that are uploaded, decoded and downloaded on three streams at once; the bytes go to
 * the device as they are. Pageable memory is staged through pinned buffers by a few copy threads
 * (ALACGPU_COPY_THREADS); blob / out / frames_out / status that the caller allocated with hipHostMalloc or registered
 * with hipHostRegister are transferred in place. Blocking: returns when everything is in the caller's buffers.
 * blob_bytes = readable bytes at blob. The offsets are untrusted (a sample table from a file, internal/mp4/mp4.go:382-420):
 * a packet that does not lie inside [0, blob_bytes), or that ends before it starts, is never read and gets status
 * ALACGPU_ERR_RANGE, like in the device entry (alacgpu 0.4: the argument is new; 0.3 read whatever the offsets named).
 */
int alacgpu_decode_batch(alacgpu_decoder* dec, const uint8_t* blob, size_t blob_bytes, const uint64_t* offsets,
                         size_t n_packets, uint8_t* out, size_t out_stride,
                         uint32_t* frames_out, int32_t* status);

/* The same decode on a thread of the library's own: _start returns at once, _wait blocks until the decode is done and
 * returns what alacgpu_decode_batch would have (its error text becomes the waiting thread's alacgpu_last_error). One
 * decode in flight per handle; nothing else may be called on the handle in between (alacgpu_destroy waits by itself), and
 * all buffers stay the caller's to keep alive and untouched until _wait returns. What a read-ahead file decoder needs:
 * window k + 1 is decoded while the caller drains window k (host/stream_decoder.hpp, stream.py, go/alacgpu_decoder.go): the
 * batch form of the reference's Read loop, which decodes the packet it is about to hand out (decode.go:157-186). */
int alacgpu_decode_batch_start(alacgpu_decoder* dec, const uint8_t* blob, size_t blob_bytes, const uint64_t* offsets,
                               size_t n_packets, uint8_t* out, size_t out_stride, uint32_t* frames_out, int32_t* status);
int alacgpu_decode_batch_wait(alacgpu_decoder* dec);

/*
 * DecodePackets, device-resident (the benchmark path). All pointers are device pointers on the handle's device.
 * Packet i is d_blob[d_offsets[i] .. +d_sizes[i]); d_sizes may be NULL, then d_offsets has n_packets+1 entries and
 * packet i ends where packet i+1 starts. blob_bytes = readable bytes at d_blob: a packet that does not lie inside
 * [0, blob_bytes) gets status ALACGPU_ERR_RANGE and is not read. Asynchronous on the handle's stream
 * (alacgpu_stream()) unless sync != 0: the inputs must be complete, or ordered on that stream, before the call, and
 * the outputs are complete after alacgpu_synchronize() (the stream is non-blocking: it does not order against the
 * legacy default stream or torch's current stream by itself). Some of a decode's kernels (those of the irregular
 * packets of 1-2 channel streams) run on a second stream inside the handle; it leaves the handle's stream after the
 * sort and joins it again before the decode's last event, so work a caller orders behind the handle's stream (an
 * event, a copy enqueued on alacgpu_stream()) is ordered behind those kernels as well.
 * Footprint: packet i writes [0, d_frames_out[i] * bytes per frame) of its slot and nothing else: the bytes of a slot behind
 * a partial frame, the bytes [frame bytes, out_stride) of every slot, and everything in front of the first slot or behind
 * the last one are left untouched. A failing packet's slot holds unspecified bytes in [0, frame bytes): the wave pairs may
 * have written PCM of its first samples before the error (the host entry zeroes such slots).
 * d_out and out_stride both multiples of 16 is the fast layout. Anything else (a misaligned d_out, or a stride such as frame
 * bytes that is not a multiple of 16) is decoded correctly, with the same bytes, but EVERY packet takes the irregular kernels
 * (alac_scan, then alac_interleave / alac_interleave4 with byte stores, then the whole-packet decoder) and no wave-pair
 * kernel runs; alacgpu_last_dispatch() shows narrow_slots = wide_slots = 0. That route's cost has not been measured.
 */
int alacgpu_decode_batch_device(alacgpu_decoder* dec, const uint8_t* d_blob, size_t blob_bytes,
                                const uint64_t* d_offsets, const uint32_t* d_sizes,
                                size_t n_packets, uint8_t* d_out, size_t out_stride,
                                uint32_t* d_frames_out, int32_t* d_status, int sync);

/* Device scratch the handle needs for a batch of n packets. The batch entries grow it on demand — and growing means
 * hipFree + hipMalloc, which wait for the DEVICE to go idle: an alacgpu_decode_batch_device(..., sync = 0) whose batch is
 * larger than any the handle has seen (or reserved) therefore BLOCKS until earlier work on the device is done, although
 * it is documented as asynchronous. Callers that rely on asynchrony reserve for their largest batch first. */
int alacgpu_reserve(alacgpu_decoder* dec, size_t n_packets);

/* Duration of the last decode on this handle in milliseconds: HIP events on the handle's stream around ALL the
 * kernels of the decode, the sort pre-pass included (valid after a sync). Used by bench.py's roofline. */
int alacgpu_last_kernel_ms(alacgpu_decoder* dec, float* ms);

/* Per-decode durations: every decode (all its kernels) is bracketed by a HIP event pair on the handle's
 * stream (ring of 64). alacgpu_kernel_times synchronizes the stream and returns the durations of the
 * min(max_n, launches since reset, 64) most recent launches, oldest first. */
int alacgpu_timing_reset(alacgpu_decoder* dec);
int alacgpu_kernel_times(alacgpu_decoder* dec, float* ms, size_t max_n, size_t* n_out);

/* Diagnostics: who decoded which wave slot of the last device decode on this handle, and when. Four words per wave
 * slot of the launch plan (irregular packets first, then wide keys, then narrow ones, slowest first; n_out counts
 * slots, max_n words): [0] is 0 for slots that no wave pair owns (the irregular ones), else bit 31 | SIMD of the
 * predictor wave << 19 | SIMD of the entropy wave << 17 | CU number << 8 | the pair's arrival number on its CU << 4 |
 * bit 0 set when the pair took the slot after finishing another; [1], [2] the low words of the wave's
 * s_memtime counter (about 2.1 GHz on MI355X) when the pair began and ended the slot; [3] unused. tests/test_gpu_parity.py checks the spread over
 * the CUs, tools/pair_placement.py prints it. */
int alacgpu_pair_placement(alacgpu_decoder* dec, uint32_t* tags, size_t max_n, size_t* n_out);
/* Diagnostics: what the last device decode on this handle dispatched, read back from the launch plan the device built
 * (the host only knows upper bounds when it launches): wave slots by class and the kernel that decoded the narrow
 * regular ones — the four-wave kernel of the handle's sample width or, for 16-bit batches between the rounds, its gated
 * twin (the device decides with the function the host repeats here on the plan's numbers). bench.py names the roofline's
 * kernel with it. Synchronizes the handle's stream. */
typedef struct alacgpu_dispatch {
    uint32_t packets_per_slot;   /* 64, less for small batches */
    uint32_t slots;              /* wave slots of the plan = irregular + wide + narrow */
    uint32_t irregular_slots, wide_slots, narrow_slots;
    uint32_t keys;               /* sort keys present */
    uint32_t gated;              /* 1: the gated twin took the narrow slots */
    uint32_t lanes_per_packet;   /* 2 / 4: predictor waves on that many lanes per packet for the long predictors; 0: none */
    char narrow_kernel[32], wide_kernel[32], irregular_kernels[96]; /* "" when the class is empty */
    uint32_t workgroups_per_cu;  /* four-wave kernels: 4 or 5 of their workgroups share a CU (the LDS footprint of the launch that worked); 0: gated twin / none */
} alacgpu_dispatch;
int alacgpu_last_dispatch(alacgpu_decoder* dec, alacgpu_dispatch* out);
/* Placement relies on the gfx950 layout of two hardware registers read with s_getreg_b32: HW_ID (SIMD [5:4], CU [11:8],
 * shader engine [14:13]) and XCC_ID ([3:0]); the index built from them stays below 512 and a CU the census of
 * alacgpu_create() missed only loses its fixed place in the item order, so a different layout costs speed, not
 * correctness. Measured and tested on an unpartitioned MI355X (SPX: 256 CUs in 8 XCDs) only; on a partitioned device
 * (CPX) the CU count per device and the XCD assumptions of the numbering (item i on XCD i mod 8) are untested. */

/* The handle's hipStream_t as an opaque pointer (for callers that enqueue copies). */
void* alacgpu_stream(alacgpu_decoder* dec);

int alacgpu_synchronize(alacgpu_decoder* dec);

/*
 * WAVEFORMS (0.7.0): the decoder's PCM slots as planar float32 / int32 tensors, one pass of its own behind a decode (it
 * does not touch the decode kernels or their outputs). Input is what alacgpu_decode_batch_device wrote: d_pcm / pcm_stride
 * (its d_out / out_stride), d_frames, and d_status, which may be NULL. With
 *     f[i]     = (d_status && d_status[i] != 0) ? 0 : min(d_frames[i], frame_length)
 *     start[i] = f[0] + ... + f[i - 1],   total = start[n_packets]
 * and d_wave counted in 4-byte elements:
 *   ALACGPU_WAVE_STREAM   d_wave is [channels][channel_stride]: frame t of packet i, channel c, goes to
 *                         d_wave[c * channel_stride + start[i] + t] — the concatenation a file reader produces, failed packets
 *                         contributing nothing. Nothing outside [0, total) of each channel row is written.
 *   ALACGPU_WAVE_PACKETS  d_wave is [n_packets][channels] rows: d_wave[i * packet_stride + c * channel_stride + t]; the columns
 *                         [f[i], frame_length) of every row are written as zero (a failed packet is a silent clip), nothing behind
 *                         column frame_length or between the rows is touched.
 *   ALACGPU_WAVE_FLOAT    float32 = the sample as a signed integer x 2^-(w - 1), w = 16 / 24 / 24 / 32 at depth 16 / 20 / 24 / 32
 *                         (a 20-bit sample is the 24-bit value its three bytes hold). The integer is converted with one
 *                         rounding to nearest even and the scale is a power of two: exact up to 24 bits, rounded once at 32.
 *   ALACGPU_WAVE_INT      int32 = the same integer, unscaled, exact at every depth.
 * d_starts (uint64, n_packets + 1 entries, may be NULL) receives start[]; d_starts[n_packets] = total. n_packets = 0
 * succeeds and writes d_starts[0] = 0.
 * ALACGPU_E_ARG before any HIP call: a NULL handle, d_pcm, d_frames or d_wave; an unknown layout or type; d_wave not
 * 4-byte aligned; pcm_stride below the frame bytes; STREAM with channel_stride < n_packets * frame_length (the bound that,
 * with the clamp of f[i], makes a hostile d_frames harmless); PACKETS with channel_stride < frame_length or packet_stride <
 * channels * channel_stride.
 * Every alignment of d_pcm, pcm_stride, d_wave and the strides gives the same values; d_pcm and pcm_stride multiples of 16
 * is what the decode wants (see above), the pass itself loads and stores 16 bytes at a time at every alignment.
 * Asynchronous on the handle's stream unless sync != 0, with the ordering contract of alacgpu_decode_batch_device: called
 * behind a decode with sync = 0 it runs behind that decode, no host synchronisation in between. The scan's scratch (8 bytes
 * per packet) is the handle's; alacgpu_reserve covers it.
 */
typedef enum alacgpu_wave_layout { ALACGPU_WAVE_STREAM = 0, ALACGPU_WAVE_PACKETS = 1 } alacgpu_wave_layout;
typedef enum alacgpu_wave_type { ALACGPU_WAVE_FLOAT = 0, ALACGPU_WAVE_INT = 1 } alacgpu_wave_type;
int alacgpu_waveform_device(alacgpu_decoder* dec, const uint8_t* d_pcm, size_t pcm_stride, const uint32_t* d_frames,
                            const int32_t* d_status, size_t n_packets, int layout, int type, void* d_wave,
                            size_t channel_stride, size_t packet_stride, uint64_t* d_starts, int sync);
/* Duration of the last waveform pass in milliseconds: HIP events around its kernels (valid after a sync).
 * alacgpu_last_kernel_ms and alacgpu_kernel_times keep counting decodes only. */
int alacgpu_waveform_last_ms(alacgpu_decoder* dec, float* ms);

/*
 * CLIPS: a batch of fixed-length crops at arbitrary frame offsets, gathered from the decoder's PCM slots into one
 * [n_clips][channels][clip_frames] float32 / int32 tensor: one pass of its own behind a decode, like the waveform pass (it
 * does not touch the decode kernels or their outputs). Input is what alacgpu_waveform_device takes: d_pcm / pcm_stride,
 * d_frames, and d_status, which may be NULL. Slot i occupies the frames [i * frame_length, (i + 1) * frame_length) of a GRID
 * over the batch; clip j < n_clips has two 64-bit descriptors on the device: d_begin[j], its first grid frame (any frame, not
 * only a packet boundary), and d_limit[j], the first slot that does not belong to the clip's source (a clip of file A stops in
 * front of file B's packets). With FL = frame_length, L = clip_frames >= 1 and d_clips counted in 4-byte elements:
 *     f[i] = (d_status && d_status[i] != 0) ? 0 : min(d_frames[i], FL)
 *     g    = d_begin[j] + t,  i = g / FL,  r = g % FL                                      for t < L
 *     has  = g does not overflow && i < min(d_limit[j], n_packets) && r < f[i]
 *     d_clips[j * clip_stride + c * channel_stride + t] = has ? sample(i, r, c) : 0        ALACGPU_WAVE_FLOAT / _INT as above
 *     d_valid[j]       (may be NULL) = the number of t < L with `has`
 *     d_clip_status[j] (may be NULL) = d_status[i] of the lowest slot i the clip touches (i < min(d_limit[j], n_packets))
 *                                      with d_status[i] != 0, else 0 (always 0 without d_status)
 * Every column [0, L) of every [clip][channel] row is written, nothing behind column L or between the rows is touched. A
 * failed or short slot inside a clip is a gap of zeros, exactly as ALACGPU_WAVE_PACKETS pads; frames behind the clip's last slot
 * are zeros at the end, and d_valid says how many columns are samples. The descriptors are untrusted: no value of them
 * causes a read outside the slots [0, n_packets) or behind a slot's first f[i] frames — d_begin past the batch or 2^64 - 1,
 * d_limit 0 or above n_packets and d_frames[i] above frame_length all give zeros where they apply.
 * n_clips = 0 succeeds and touches nothing; n_packets = 0 with clips writes zeros (and d_valid = 0).
 * ALACGPU_E_ARG before any HIP call: a NULL handle; with n_clips > 0 a NULL d_pcm, d_frames, d_begin, d_limit or d_clips;
 * an unknown type; clip_frames = 0; d_clips not 4-byte aligned; pcm_stride below the frame bytes (with n_packets > 0);
 * channel_stride < clip_frames; clip_stride < channels * channel_stride; n_packets or n_clips above 2^31 - 1, or strides
 * whose product with them overflows.
 * Every alignment of d_pcm, pcm_stride, d_clips, the strides and d_begin gives the same values, loaded and stored 16 bytes
 * at a time in the body. Asynchronous on the handle's stream unless sync != 0, with the ordering contract
 * of alacgpu_decode_batch_device: called behind a decode with sync = 0 it runs behind that decode, no host synchronisation
 * in between. The pass needs no scratch of the handle. d_valid and d_clip_status come from one lane per clip that walks the
 * slots the clip touches, min(clip_frames / frame_length + 2, n_packets) steps: with frame lengths of a few frames and clips
 * of millions that lane sets the pass's time; pass both as NULL where they are not needed and no such walk is launched.
 */
int alacgpu_clips_device(alacgpu_decoder* dec, const uint8_t* d_pcm, size_t pcm_stride, const uint32_t* d_frames,
                         const int32_t* d_status, size_t n_packets, const uint64_t* d_begin, const uint64_t* d_limit,
                         size_t n_clips, uint32_t clip_frames, int type, void* d_clips, size_t channel_stride,
                         size_t clip_stride, uint32_t* d_valid, int32_t* d_clip_status, int sync);
/* Duration of the last clip gather in milliseconds: HIP events around its kernels (valid after a sync). */
int alacgpu_clips_last_ms(alacgpu_decoder* dec, float* ms);

/*
 * Batch ENCODER (0.6.0; the reference is decode-only). Input: one contiguous interleaved little-endian PCM stream in the
 * decoder's output format (2 / 3 / 3 / 4 bytes per sample at 16 / 20 / 24 / 32 bits; a 20-bit sample is left-aligned in
 * its 3 bytes and its low 4 bits are ignored). total_frames frames become ceil(total_frames / frame_length) packets; only
 * the last one may be short, and only it carries the partial flag and its frame count. Every packet is encoded on its own
 * (nothing carries over between packets): elements in the decoder's channel layout, an END tag, padded to a byte; per
 * element mode 0, denShift 9, pbFactor 4, order 8 with Apple's initial coefficients warmed by one pass over the element's
 * own samples, mixBits 2 / mixRes 2 for a CPE, bytesShifted 0 / 0 / 1 / 2 at 16 / 20 / 24 / 32 bits, the config's pb / mb
 * / kb; an element whose compressed form is not smaller than raw goes out escaped (raw samples), and so does every element
 * when frame_length <= 8 or kb = 0 (configs under which the decoder cannot read an order-8 element). The packets decode to the
 * input PCM through alacgpu_decode_batch* and the reference. One handle is single-caller, like a decoder.
 */
typedef struct alacgpu_encoder alacgpu_encoder;

/* Rejects what alacgpu_create rejects (ALACGPU_E_CONFIG, before any HIP call). One stream per handle. */
int alacgpu_encoder_create(const alacgpu_config* cfg, int device, alacgpu_encoder** out);
void alacgpu_encoder_destroy(alacgpu_encoder* enc);

/* A blob capacity that always suffices for total_frames frames: every element at its escape size plus the largest
 * header, per packet. 0 for a NULL handle. */
uint64_t alacgpu_encode_max_bytes(const alacgpu_encoder* enc, uint64_t total_frames);

/* Device-resident encode. d_pcm: total_frames interleaved frames; d_blob: blob_cap bytes, receives the packets back to
 * back (dense); d_offsets: n + 1 entries, packet i is d_blob[d_offsets[i] .. d_offsets[i + 1]), so the result feeds
 * alacgpu_decode_batch_device(..., d_sizes = NULL, ...) unchanged. A blob_cap below alacgpu_encode_max_bytes() is
 * ALACGPU_E_ARG and nothing is written. Asynchronous on the handle's stream (alacgpu_encoder_stream()) unless sync != 0,
 * with the ordering contract of alacgpu_decode_batch_device: inputs complete or ordered on that stream before the call,
 * outputs complete after alacgpu_encoder_synchronize(). One encode takes at most 2^31 - 1 packets (more is ALACGPU_E_ARG;
 * cut the stream). Device scratch of the handle, grown on demand: about 800 bytes per packet plus 2 x frame_length x depth
 * / 8 bytes per channel of a packet (its chains' bitstreams); a failed allocation is ALACGPU_E_HIP. Every channel of a
 * packet is one serial chain on one lane, so a batch of few long packets runs on few lanes: its time grows with
 * frame_length, not with the device's width. */
int alacgpu_encode_device(alacgpu_encoder* enc, const uint8_t* d_pcm, uint64_t total_frames, uint8_t* d_blob,
                          uint64_t blob_cap, uint64_t* d_offsets, int sync);

/*
 * WAVEFORMS IN: planar float32 / int32 tensors -> the encoder's interleaved PCM, one memory-bound pass of its own on the
 * handle's stream (k_wavepack.hip; the inverse of alacgpu_waveform_device; the encode kernels and their outputs are
 * untouched). d_wave is counted in 4-byte elements, layout and type are alacgpu_wave_layout / alacgpu_wave_type:
 *   ALACGPU_WAVE_STREAM   [channels][channel_stride]: frame t of channel c is d_wave[c * channel_stride + t], t < total_frames
 *   ALACGPU_WAVE_PACKETS  [n][channels] rows, n = ceil(total_frames / frame_length): frame t of clip i is
 *                         d_wave[i * packet_stride + c * channel_stride + t]. Only the last clip may be short; its columns
 *                         behind total_frames - (n - 1) * frame_length are not read.
 * The pass writes total_frames contiguous interleaved frames (alacgpu_encode_device's input format) and nothing outside
 * [d_pcm, d_pcm + total_frames * bytes per frame). Values, exact and deterministic, with q = the bit depth:
 *   ALACGPU_WAVE_FLOAT    v = rint(x * 2^(q - 1)) in float32 (the product is exact, one rounding to nearest even), saturated to
 *                         [-2^(q - 1), 2^(q - 1) - 1]; NaN gives 0. At depth 20 the three bytes hold v << 4, so what
 *                         alacgpu_waveform_device made of a 20-bit stream comes back exactly.
 *   ALACGPU_WAVE_INT      the int32 that alacgpu_waveform_device's INT gives (at depth 20 the 24-bit container value),
 *                         saturated to the container's width 16 / 24 / 24 / 32; at depth 20 the low four bits are cleared.
 * d_clipped (one uint64 on the device, may be NULL) receives the number of samples of this call that were saturated or
 * were NaN (cleared low bits do not count); the entry clears it on the stream first. total_frames = 0 succeeds and writes
 * *d_clipped = 0.
 * alacgpu_encode_waveform_device is the pass into PCM scratch of the handle (total_frames x bytes per frame, grown on
 * demand; a failed allocation is ALACGPU_E_HIP) followed by alacgpu_encode_device on the same stream, no host
 * synchronisation in between: d_blob and d_offsets are byte for byte those of alacgpu_encode_device on that PCM.
 * ALACGPU_E_ARG before any HIP call: a NULL handle, d_wave, d_pcm / d_blob or d_offsets; an unknown layout or type; d_wave
 * not 4-byte aligned; STREAM with channel_stride < total_frames; PACKETS with channel_stride < frame_length or
 * packet_stride < channels * channel_stride; blob_cap below alacgpu_encode_max_bytes(); more than 2^31 - 1 packets.
 * Every alignment of d_wave, the strides and d_pcm gives the same bytes, 16 bytes wide in the body.
 * Asynchronous on the handle's stream unless sync != 0, with the ordering contract of alacgpu_encode_device.
 */
int alacgpu_pcm_from_waveform_device(alacgpu_encoder* enc, const void* d_wave, int layout, int type, size_t channel_stride,
                                     size_t packet_stride, uint64_t total_frames, uint8_t* d_pcm, uint64_t* d_clipped,
                                     int sync);
int alacgpu_encode_waveform_device(alacgpu_encoder* enc, const void* d_wave, int layout, int type, size_t channel_stride,
                                   size_t packet_stride, uint64_t total_frames, uint8_t* d_blob, uint64_t blob_cap,
                                   uint64_t* d_offsets, uint64_t* d_clipped, int sync);
/* Duration of the last pack pass in milliseconds: HIP events around its kernels (valid after a sync).
 * alacgpu_encoder_last_kernel_ms keeps timing the five encode kernels only. */
int alacgpu_encoder_waveform_last_ms(alacgpu_encoder* enc, float* ms);

/* Host buffers, blocking. pcm holds total_frames frames; blob_cap as above; offsets gets n + 1 entries; *blob_bytes_out
 * the bytes written (= offsets[n]). Buffers from alacgpu_host_alloc / hipHostMalloc / hipHostRegister are transferred in
 * place, pageable ones are staged through pinned buffers of the handle. */
int alacgpu_encode(alacgpu_encoder* enc, const uint8_t* pcm, uint64_t total_frames, uint8_t* blob, uint64_t blob_cap,
                   uint64_t* offsets, uint64_t* blob_bytes_out);

/* The 24-byte big-endian ALACSpecificConfig (config.go:64-79, what ParseMagicCookie reads) of what this handle has
 * encoded: the config's fields, max_frame_bytes = its largest packet so far, avg_bit_rate = bits per second over all its
 * packets so far (from the bytes, the frames and sample_rate). Synchronizes the handle's stream. */
int alacgpu_encoder_cookie(alacgpu_encoder* enc, uint8_t out[24]);

/* Duration of the last encode in milliseconds: HIP events around all its kernels (valid after a sync). */
int alacgpu_encoder_last_kernel_ms(alacgpu_encoder* enc, float* ms);

/* The handle's hipStream_t as an opaque pointer, and a wait for everything on it. */
void* alacgpu_encoder_stream(alacgpu_encoder* enc);
int alacgpu_encoder_synchronize(alacgpu_encoder* enc);

/*
 * RESAMPLING: float32 rows at one sample rate -> the same rows at another, one pass on a handle of its own (k_resample.hip,
 * alac_resample.h; no decoder or encoder is involved, and their kernels are untouched). The filter is torchaudio's
 * sinc_interp_hann (its defaults: lowpass_filter_width 6, rolloff 0.99). With g = gcd(orig, new), o = orig / g, n = new / g,
 * W = lowpass_filter_width:
 *     base  = min(o, n) * rolloff,   width = ceil(W * o / base)
 *     t     = clamp(((k - width) / o - i / n) * base, -W, W)                         phase i < n, tap k < 2 * width + o
 *     H[i][k] = |t| == W ? 0 : sinc(pi t) * cos(pi t / (2 W))^2 * base / o           in double, sinc(0) = 1
 *     out_frames(T) = ceil(new * T / orig)
 *     y[m] = sum_k H[i][k] * x[j * o + k - width],  m = j * n + i,  x[.] = 0 outside [0, T)
 * The taps of a phase that are not zero are one run; a plan keeps first[i], the k of phase i's first kept tap, and h[i][q] =
 * float(H[i][first[i] + q]) for q < taps (the widest run). An output is acc = +0.0f; acc = fmaf(h[i][q], x[j * o + first[i] +
 * q - width], acc) for q = 0 .. taps - 1 in that order, +0.0f for an x outside the row: the same bits on every build.
 * alacgpu_resampler_create is ALACGPU_E_ARG, before any HIP call, when no plan can be built: a rate of 0, equal rates,
 * lowpass_filter_width 0, rolloff outside (0, 1], n * (2 * width + 2) table entries above 64 MB, or a ratio so steep that the
 * inputs of 64 outputs exceed the 3 840 floats a workgroup stages (192 000 -> 8 000 fits). The handle owns a stream, an event
 * pair and the table on the device; it is single-caller, like a decoder.
 */
typedef struct alacgpu_resampler alacgpu_resampler;
int alacgpu_resampler_create(int device, uint32_t orig_freq, uint32_t new_freq, uint32_t lowpass_filter_width, double rolloff,
                             alacgpu_resampler** out);
void alacgpu_resampler_destroy(alacgpu_resampler* rs);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernels (valid after a sync). */
void* alacgpu_resampler_stream(alacgpu_resampler* rs);
int alacgpu_resampler_synchronize(alacgpu_resampler* rs);
int alacgpu_resampler_last_ms(alacgpu_resampler* rs, float* ms);
/* ceil(new * in_frames / orig) in 64-bit integers; 0 for a NULL handle or when the product leaves 64 bits. */
uint64_t alacgpu_resample_out_frames(const alacgpu_resampler* rs, uint64_t in_frames);
/*
 * rows rows of in_frames float32 frames, row r at d_in + r * in_row_stride (strides in elements), -> rows of out_frames =
 * alacgpu_resample_out_frames(rs, in_frames) at d_out + r * out_row_stride. Exactly the columns [0, out_frames) of every
 * output row are written, nothing between or behind the rows; nothing outside [0, in_frames) of an input row is read.
 * rows = 0 or in_frames = 0 succeeds and touches nothing. ALACGPU_E_ARG before any HIP call: a NULL handle; with work to do a
 * NULL d_in or d_out, a base that is not 4-byte aligned, in_row_stride < in_frames, out_row_stride < out_frames, or sizes
 * whose products overflow. Every 4-byte-aligned base and every stride gives the same values, loaded and stored 16 bytes at a
 * time in the body. Asynchronous on the handle's stream unless sync != 0: the input must be complete, or
 * ordered on that stream, before the call (the stream is non-blocking: it does not order against torch's by itself).
 */
int alacgpu_resample_device(alacgpu_resampler* rs, const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames,
                            float* d_out, size_t out_row_stride, int sync);
/* The plan the handle's kernel uses: its numbers, and (where the pointers are not NULL and the capacities, counted in
 * entries, suffice: n * taps and n) the host copies of h[n][taps] and first[n]. */
typedef struct alacgpu_resample_info {
    uint32_t o, n, width, taps, tile_out;
} alacgpu_resample_info;
int alacgpu_resampler_plan(const alacgpu_resampler* rs, alacgpu_resample_info* info, float* h_out, size_t h_cap,
                           int32_t* first_out, size_t first_cap);

/*
 * SPECTROGRAMS: float32 rows -> their power spectrograms or (log-)mel spectrograms, one fused pass on a handle of its own
 * (k_mel.hip, alac_mel.h; no decoder, encoder or resampler is involved, and their kernels are untouched): what torch.stft
 * (periodic Hann window, reflect padding), abs()^2, a matmul with torchaudio's melscale_fbanks and a log compute, without the
 * intermediates. N = n_fft, W = win_length, h = hop_length, K = N / 2 + 1:
 *     w[n]    = 0.5 - 0.5 cos(2 pi (n - (N - W) / 2) / W) inside the window's W samples at offset (N - W) / 2, else 0; the one
 *               sample of W = 1 is 1.0, as torch.hann_window(1) is
 *     C[k][n] = w[n] cos(2 pi ((k n) mod N) / N),  S[k][n] = w[n] sin(2 pi ((k n) mod N) / N)     in double, rounded once
 *     frames  center: F = 1 + (T - (N & 1)) / h for T > N / 2 (torch.stft's count: N / 2 samples of padding on each side),
 *             frame f reads x[f h - N / 2 + n], reflected at both ends (index i < 0 is -i, i >= T is 2 (T - 1) - i);
 *             otherwise F = 1 + (T - N) / h for T >= N and frame f reads x[f h + n]
 *     p[k]    = fmaf(im, im, re * re),  re = fmaf(C[k][n], x[n], re), im = fmaf(S[k][n], x[n], im) for n = 0 .. N - 1 from +0.0f
 *     mel[m]  = fmaf chain over q < taps of fbw[m][q] * p[first[m] + q] from +0.0f: the run of filter m's weights that are
 *               not zero, in a window of taps (the widest run) clamped into [0, K)
 *     log     v <= floor ? float(s log(floor)) : s * log(v); s = 10 and log10 for ALACGPU_MEL_LOG_DB
 * Up to the log every build gives the same bits; the device's log differs from libm's in the last places.
 * The filterbank is melscale_fbanks(K, f_min, f_max, n_mels, sample_rate, norm, mel_scale) evaluated in double, its two outer
 * points f_min and f_max themselves. Power (|X|^2) only; no top_db and no per-row maximum: those stay with the caller.
 * alacgpu_mel_create is ALACGPU_E_ARG, before any HIP call, when no plan can be built: n_fft outside [2, 2048], win_length
 * outside [1, n_fft], hop_length 0, sample_rate 0, center or norm above 1, a mel_scale or log outside its values, floor not a
 * positive float32; with a mel scale n_mels outside [1, 4096] or not 0 <= f_min < f_max; with ALACGPU_MEL_SCALE_NONE (the
 * power spectrogram itself is the output) n_mels or norm not 0; or four frames that do not fit 64 KB of LDS. The handle owns
 * a stream, an event pair and the tables on the device; it is single-caller, like a decoder.
 *
 * transform = ALACGPU_MEL_TRANSFORM_FFT (opt-in; k_melfft.hip, alac_melfft.h) computes p[k] by a mixed-radix FFT
 * out of LDS in place of the chains over the basis; frames, mel, log and output are the same. n_fft must be even with M = n_fft /
 * 2 = 2^a 3^b 5^c: any other n_fft is ALACGPU_E_ARG before any HIP call (there is no fall-back to the direct transform), and so is
 * a transform above 1.
 *     v[n]    = w32[n] * x[n], w32 the window above rounded to float32 once;  z[m] = v[2 m] + i v[2 m + 1]
 *     Z       = FFT_M(z): in-place passes of radix 5, 3, 4, 2 in the plan's order, twiddles from float32 tables
 *     X[k]    = (Z[k] + conj Z[M - k]) / 2 + exp(-2 pi i k / N) (Z[k] - conj Z[M - k]) / (2 i), k = 0 .. M, indices mod M
 *     p[k]    = fmaf(im, im, re * re)
 * with every float operation in a fixed order and none contracted (alac_melfft.h writes them out), so up to the log every build
 * gives the same bits here too; they are not the direct transform's bits.
 */
enum { ALACGPU_MEL_SCALE_NONE = 0, ALACGPU_MEL_SCALE_HTK = 1, ALACGPU_MEL_SCALE_SLANEY = 2 };
enum { ALACGPU_MEL_LOG_NONE = 0, ALACGPU_MEL_LOG_LN = 1, ALACGPU_MEL_LOG_LOG10 = 2, ALACGPU_MEL_LOG_DB = 3 };
enum { ALACGPU_MEL_TRANSFORM_DIRECT = 0, ALACGPU_MEL_TRANSFORM_FFT = 1 };
typedef struct alacgpu_mel_config {
    uint32_t sample_rate;
    uint32_t n_fft;
    uint32_t win_length; /* 1 .. n_fft */
    uint32_t hop_length; /* >= 1 */
    double f_min, f_max; /* Hz; read with a mel scale only */
    uint32_t n_mels;     /* 0 with ALACGPU_MEL_SCALE_NONE */
    uint32_t center;     /* 1: frames centred on f * hop_length, reflect padding; 0: frames start there */
    uint32_t norm;       /* 0 none, 1 slaney */
    uint32_t mel_scale;  /* ALACGPU_MEL_SCALE_* */
    uint32_t log;        /* ALACGPU_MEL_LOG_* */
    uint32_t transform;  /* ALACGPU_MEL_TRANSFORM_*; 0, the direct transform, is what a zeroed field asked for before */
    double floor;        /* > 0; read with a log only, but checked always */
} alacgpu_mel_config;
typedef struct alacgpu_mel alacgpu_mel;
int alacgpu_mel_create(int device, const alacgpu_mel_config* config, alacgpu_mel** out);
void alacgpu_mel_destroy(alacgpu_mel* mel);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernels (valid after a sync). */
void* alacgpu_mel_stream(alacgpu_mel* mel);
int alacgpu_mel_synchronize(alacgpu_mel* mel);
int alacgpu_mel_last_ms(alacgpu_mel* mel, float* ms);
/* F for rows of in_frames samples; 0 for a NULL handle, where no frame exists, or above 2^61 samples. */
uint64_t alacgpu_mel_out_frames(const alacgpu_mel* mel, uint64_t in_frames);
/*
 * rows rows of in_frames float32 samples, row r at d_in + r * in_row_stride (strides in elements), -> [rows][bins][F], F =
 * alacgpu_mel_out_frames(mel, in_frames), bins = n_mels or K: element (r, b, f) at d_out + r * out_row_stride + b *
 * out_bin_stride + f. Exactly those elements are written, nothing in the gaps the strides leave; nothing outside [0, in_frames)
 * of an input row is read. rows = 0 or F = 0 succeeds and touches nothing. ALACGPU_E_ARG before any HIP call: a NULL handle;
 * with work to do a NULL d_in or d_out, a base that is not 4-byte aligned, in_row_stride < in_frames, out_bin_stride < F,
 * out_row_stride < (bins - 1) * out_bin_stride + F, or sizes whose products overflow. Every 4-byte-aligned base and every
 * stride gives the same values. Asynchronous on the handle's stream unless sync != 0: the input must be complete, or ordered
 * on that stream, before the call (the stream is non-blocking: it does not order against torch's by itself).
 */
int alacgpu_mel_device(alacgpu_mel* mel, const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out,
                       size_t out_row_stride, size_t out_bin_stride, int sync);
/* The plan the handle's kernel uses: its numbers, and (where the pointers are not NULL and the capacities, counted in
 * entries, suffice) the host copies of the basis [2][n_freqs][n_fft] (C, then S), of the filterbank windows fbw[n_mels][taps]
 * and of first[n_mels]. taps is 0 without a mel stage. */
typedef struct alacgpu_mel_info {
    uint32_t n_fft, win_length, hop_length, n_freqs, n_mels, taps, bins, tile_frames, lds_bytes;
} alacgpu_mel_info;
int alacgpu_mel_plan(const alacgpu_mel* mel, alacgpu_mel_info* info, float* basis_out, size_t basis_cap, float* fb_out,
                     size_t fb_cap, int32_t* first_out, size_t first_cap);
/* The plan of the handle's transform. On a handle with ALACGPU_MEL_TRANSFORM_FFT (whose alacgpu_mel_plan reports a basis of 0
 * entries: none is built; basis_out is left alone): tile_frames and lds_bytes (the FFT's own choice, which alacgpu_mel_plan
 * reports as well), batch_frames (the frames of a tile transformed at a time), pitch (complex elements between two frames in
 * the transform buffer), the passes' radices in order, and (where the pointers are not NULL and the capacities suffice) the
 * window w32[n_fft] and the twiddle table: 8 roots {-0.5, sin(2 pi / 3), cos, sin(2 pi / 5), cos, sin(4 pi / 5), 0, 0}, then per
 * pass s (radix r, L = the product of the radices before it) L (r - 1) pairs {cos, -sin}(2 pi ((q k) mod (L r)) / (L r)) at [k][q
 * - 1], then n_fft / 2 + 1 pairs {cos, -sin}(2 pi k / n_fft). On a direct handle transform is 0, tile_frames and lds_bytes are
 * alacgpu_mel_plan's, and everything else is 0. */
typedef struct alacgpu_mel_fft_info {
    uint32_t transform, tile_frames, lds_bytes, batch_frames, pitch, n_passes;
    uint32_t radix[8];
    uint32_t window_entries, twiddle_entries;
} alacgpu_mel_fft_info;
int alacgpu_mel_fft_plan(const alacgpu_mel* mel, alacgpu_mel_fft_info* info, float* window_out, size_t window_cap,
                         float* twiddle_out, size_t twiddle_cap);

/*
 * KALDI FEATURES: float32 rows -> Kaldi's filterbank (fbank) or MFCC features, one fused pass on a handle of its own
 * (k_fbank.hip, alac_fbank.h over alac_mel.h; the spectrogram pass and every other kernel are untouched): what
 * torchaudio.compliance.kaldi.fbank / .mfcc compute, without the intermediates. W = frame_length, h = frame_shift, N = the
 * next power of two >= W with round_to_power_of_two, else W, at most 2048; K = N / 2 + 1; M = num_mel_bins:
 *     frames  snip_edges: F = 1 + (T - W) / h for T >= W, frame f reads x[f h + n], n < W; otherwise F = (T + h / 2) / h for
 *             T >= W, frame f reads x[f h - (W / 2 - h / 2) + n], index i < 0 being -1 - i and i >= T being 2 T - 1 - i (Kaldi's
 *             reflection: the edge sample repeats). T < W has no frame in either mode.
 *     frame   mean removed (remove_dc_offset), y[n] = v[n] - c v[n - 1] with v[-1] = v[0] (c = preemphasis_coefficient),
 *             times the symmetric window of window_type, zeros up to N; all of it, and `scale`, folded into the basis
 *             C[k][n], S[k][n], n < W, in double, each entry rounded once (alac_fbank.h spells the folding out)
 *     p[k]    = fmaf(im, im, re * re),  re = fmaf(C[k][n], x[n], re), im = fmaf(S[k][n], x[n], im) for n = 0 .. W - 1 from +0.0f
 *     mel[m]  = fmaf chain over q < taps of fbw[m][q] * p[first[m] + q] from +0.0f; the weights are get_mel_banks' in double:
 *             triangles in mel(f) = 1127 ln(1 + f / 700) over the bins k < N / 2, M + 2 points equally spaced from low_freq to
 *             high_freq (<= 0: Nyquist + high_freq)
 *     log     use_log_fbank: ln(max(v, 2^-23))
 *     energy  use_energy: ln(max(scale^2 sum (x[n] - mean)^2, 2^-23)), raised to ln(energy_floor) where that is > 0, as
 *             column 0, or the last column with htk_compat; log_energy = 0 keeps the sum itself (for checks)
 *     MFCC    num_ceps > 0: the log-mel (always logged) times D[c][m] = sqrt(2 / M) cos(pi (m + 0.5) c / M) (row 0: sqrt(1 /
 *             M)), a chain over m upwards, times 1 + 0.5 L sin(pi c / L) where L = cepstral_lifter != 0; with use_energy
 *             column 0 is the energy; with htk_compat column 0 moves to the end, and without use_energy it is then sqrt(2)
 *             C0, as in Kaldi's MfccComputer and torchaudio (row 0 of D is sqrt(2 / M) there)
 * cols = M (+ 1 with use_energy) for fbank, num_ceps for MFCC. Up to the logs every build gives the same bits.
 * alacgpu_fbank_create is ALACGPU_E_ARG, before any HIP call, when no plan can be built: frame_length outside [1, 2048],
 * frame_shift 0, sample_rate 0, a flag above 1, window_type or layout outside its values, dither != 0, vtln_warp != 1,
 * use_power 0, use_energy without raw_energy, num_mel_bins outside [1, 4096], num_ceps > num_mel_bins, a number that is not
 * finite, scale 0, energy_floor < 0, not 0 <= low_freq < Nyquist, 0 < high <= Nyquist, low < high, a filter whose weights
 * are not one run, or four frames that do not fit 64 KB of LDS. The handle owns a stream, an event pair and the tables on the
 * device; it is single-caller, like a decoder.
 *
 * alacgpu_fbank_create_transform with ALACGPU_FBANK_TRANSFORM_FFT (opt-in; k_fbankfft.hip, alac_fbankfft.h)
 * runs the frame's steps one after the other in float32 and a mixed-radix FFT out of LDS in place of the chains over the folded
 * basis; frames, energy, mel, log, MFCC and output are the same functions. The DFT size N must be even, in [2, 2048], with M = N /
 * 2 = 2^a 3^b 5^c: with round_to_power_of_two every frame_length in [2, 2048], without it frame_length itself. Any other size is
 * ALACGPU_E_ARG before any HIP call (there is no fall-back to the direct transform), and so is a transform above 1.
 *     mean    remove_dc_offset: P = 256 / tile_frames classes, s_j = the float32 sum of x[n], n = j, j + P, .. < W upwards from
 *             +0.0f; for d = P / 2 .. 1: s_j += s_{j + d}, j < d; mean = s_0 / (float)W (a division). Otherwise +0.0f, v = x.
 *     v[n]    = x[n] - mean;  y[n] = fmaf(-c32, v[n - 1], v[n]), v[-1] = v[0], c32 = float(preemphasis_coefficient), y = v at 0
 *     z[n]    = ws[n] * y[n], ws[n] = float(scale * window[n]); +0.0f for W <= n < N;  Z[m] = z[2 m] + i z[2 m + 1]
 *     p[k]    from Z by the passes and the split step of ALACGPU_MEL_TRANSFORM_FFT above
 * with every float operation in a fixed order and none contracted, so up to the logs every build gives the same bits; they are
 * not the direct transform's, except the energy column, which is. A constant frame whose sum and mean are exact gives +0.0 in
 * every mel column, as Kaldi does.
 */
enum {
    ALACGPU_FBANK_WINDOW_HANNING = 0,
    ALACGPU_FBANK_WINDOW_HAMMING = 1,
    ALACGPU_FBANK_WINDOW_POVEY = 2,
    ALACGPU_FBANK_WINDOW_RECTANGULAR = 3,
    ALACGPU_FBANK_WINDOW_BLACKMAN = 4
};
enum { ALACGPU_FBANK_LAYOUT_FRAMES = 0, ALACGPU_FBANK_LAYOUT_BINS = 1 };
enum { ALACGPU_FBANK_TRANSFORM_DIRECT = 0, ALACGPU_FBANK_TRANSFORM_FFT = 1 };
typedef struct alacgpu_fbank_config {
    uint32_t sample_rate;
    uint32_t frame_length;          /* W, samples: 1 .. 2048 */
    uint32_t frame_shift;           /* h, samples: >= 1 */
    uint32_t round_to_power_of_two; /* 0 or 1 */
    uint32_t num_mel_bins;          /* 1 .. 4096 */
    uint32_t num_ceps;              /* 0: fbank; 1 .. num_mel_bins: MFCC */
    uint32_t snip_edges;
    uint32_t remove_dc_offset;
    uint32_t window_type;           /* ALACGPU_FBANK_WINDOW_* */
    uint32_t use_log_fbank;         /* fbank only; MFCC always logs */
    uint32_t use_energy;
    uint32_t raw_energy;            /* 1 wherever use_energy is */
    uint32_t htk_compat;
    uint32_t use_power;             /* 1 */
    uint32_t log_energy;            /* 1; 0 keeps the energy column unlogged and unfloored */
    uint32_t layout;                /* ALACGPU_FBANK_LAYOUT_* */
    double preemphasis_coefficient;
    double blackman_coeff;
    double low_freq, high_freq;     /* Hz; high_freq <= 0: Nyquist + high_freq */
    double energy_floor;            /* >= 0; 0: none */
    double scale;                   /* folded into the basis; 32768 feeds [-1, 1] waveforms to recipes made for 16-bit values */
    double cepstral_lifter;         /* 0: none */
    double dither;                  /* 0 */
    double vtln_warp;               /* 1 */
} alacgpu_fbank_config;
typedef struct alacgpu_fbank alacgpu_fbank;
int alacgpu_fbank_create(int device, const alacgpu_fbank_config* config, alacgpu_fbank** out);
/* alacgpu_fbank_create with a transform, ALACGPU_FBANK_TRANSFORM_*: 0 is alacgpu_fbank_create itself. Every other entry serves
 * both kinds of handle. */
int alacgpu_fbank_create_transform(int device, const alacgpu_fbank_config* config, uint32_t transform, alacgpu_fbank** out);
void alacgpu_fbank_destroy(alacgpu_fbank* fb);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernels (valid after a sync). */
void* alacgpu_fbank_stream(alacgpu_fbank* fb);
int alacgpu_fbank_synchronize(alacgpu_fbank* fb);
int alacgpu_fbank_last_ms(alacgpu_fbank* fb, float* ms);
/* F for rows of in_frames samples; 0 for a NULL handle, where no frame exists, or above 2^61 samples. */
uint64_t alacgpu_fbank_out_frames(const alacgpu_fbank* fb, uint64_t in_frames);
/*
 * rows rows of in_frames float32 samples, row r at d_in + r * in_row_stride (strides in elements), F =
 * alacgpu_fbank_out_frames(fb, in_frames). ALACGPU_FBANK_LAYOUT_FRAMES: -> [rows][F][cols], element (r, f, c) at d_out + r *
 * out_row_stride + f * out_inner_stride + c (out_inner_stride >= cols: the frame stride). ALACGPU_FBANK_LAYOUT_BINS: ->
 * [rows][cols][F], element (r, c, f) at d_out + r * out_row_stride + c * out_inner_stride + f (out_inner_stride >= F: the bin
 * stride). Exactly those elements are written, nothing in the gaps the strides leave; nothing outside [0, in_frames) of an
 * input row is read. rows = 0 or F = 0 succeeds and touches nothing. ALACGPU_E_ARG before any HIP call: a NULL handle; with
 * work to do a NULL d_in or d_out, a base that is not 4-byte aligned, in_row_stride < in_frames, an inner stride below a
 * line, a row stride below what a row spans, or sizes whose products overflow. Asynchronous on the handle's stream unless
 * sync != 0: the input must be complete, or ordered on that stream, before the call.
 */
int alacgpu_fbank_device(alacgpu_fbank* fb, const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out,
                         size_t out_row_stride, size_t out_inner_stride, int sync);
/* The plan the handle's kernel uses: its numbers, and (where the pointers are not NULL and the capacities, counted in
 * entries, suffice) the host copies of the folded basis [2][n_freqs][frame_length] (C, then S), of the filterbank windows
 * fbw[num_mel_bins][taps], of first[num_mel_bins], of the DCT [num_ceps][num_mel_bins] and of the lifter [num_ceps]. */
typedef struct alacgpu_fbank_info {
    uint32_t frame_length, frame_shift, n_fft, n_freqs, num_mel_bins, taps, num_ceps, cols, tile_frames, lds_bytes;
} alacgpu_fbank_info;
int alacgpu_fbank_plan(const alacgpu_fbank* fb, alacgpu_fbank_info* info, float* basis_out, size_t basis_cap, float* fb_out,
                       size_t fb_cap, int32_t* first_out, size_t first_cap, float* dct_out, size_t dct_cap, float* lifter_out,
                       size_t lifter_cap);
/* The plan of the handle's transform, as alacgpu_mel_fft_plan. On a handle with ALACGPU_FBANK_TRANSFORM_FFT (whose
 * alacgpu_fbank_plan reports a basis of 0 entries: none is built; basis_out is left alone): tile_frames and lds_bytes (the FFT's
 * own choice, which alacgpu_fbank_plan reports as well), batch_frames, pitch, the passes' radices in order, and (where the
 * pointers are not NULL and the capacities suffice) the window ws[n_fft] = float(scale * window[n]), +0.0f from frame_length on,
 * and the twiddle table laid out as alacgpu_mel_fft_plan's. On a direct handle transform is 0, tile_frames and lds_bytes are
 * alacgpu_fbank_plan's, and everything else is 0. */
typedef struct alacgpu_fbank_fft_info {
    uint32_t transform, tile_frames, lds_bytes, batch_frames, pitch, n_passes;
    uint32_t radix[8];
    uint32_t window_entries, twiddle_entries;
} alacgpu_fbank_fft_info;
int alacgpu_fbank_fft_plan(const alacgpu_fbank* fb, alacgpu_fbank_fft_info* info, float* window_out, size_t window_cap,
                           float* twiddle_out, size_t twiddle_cap);

/*
 * FEATURE NORMALISATION: float32 features [rows][frames][bins] with per-row lengths -> CMVN, max-clamp, affine and masked
 * padding, one pass on a handle of its own (k_featnorm.hip, alac_featnorm.h; the feature kernels and every other
 * are untouched). Element (r, f, b) is at d + r * row_stride + f * frame_stride + b * bin_stride (elements); one of the two
 * inner strides is 1: bin stride 1 is the Kaldi pass's layout frames [rows][F][D], frame stride 1 its layout bins and the
 * spectrogram pass's [rows][bins][F], and views of them (logmel[..., :-1]). n_r = clamp(d_lengths[r], 0, frames), frames where
 * d_lengths is NULL. Per row, in this order:
 *     stat      over the valid frames f < n_r only:
 *               NONE      s = x
 *               MEAN      per bin m = S / (float)n_r, s = x - m
 *               MEAN_VAR  per bin d = x - m, v = Q / (float)n_r (Q the sum of d * d), rstd = 1.0f / sqrtf(v < var_floor ?
 *                         var_floor : v), s = d * rstd: Kaldi's apply-cmvn --norm-vars with a floor, two passes over the
 *                         deviations, never E[x^2] - m^2
 *               MAX       M = the largest x of all bins and valid frames that is no NaN, c = M - range, s = x < c ? c : x
 *     affine    y = s, y = y - shift[b] where a shift was given at create, y = y * scale[b] where a scale was: global CMVN
 *               (x - mean) * istd, or Whisper's (x + 4) / 4 as shift -4, scale 0.25; without them no arithmetic
 *     padding   y = pad_value for f >= n_r; the input there is never used, whatever it holds
 * The sums S and Q are fixed: chunks of tile_frames consecutive frames (alacgpu_norm_plan; a function of bins alone), each a
 * float32 chain in frame order from +0.0f, the chunks' sums added in chunk order from +0.0f; no operation is contracted and no
 * atomic is used. The bits depend on n_r and tile_frames only: not on rows, nor on which axis is contiguous. sqrtf is the
 * compiler's (correctly rounded under hipcc's default, 1 ulp as a bare v_sqrt_f32); every other operation is correctly rounded.
 * alacgpu_norm_create copies shift and scale (bins floats each, either may be NULL) and is ALACGPU_E_ARG, before any HIP call,
 * for a NULL config, bins outside [1, 4096], an unknown stat, var_floor that is not > 0 (in every mode), or stat MAX with a range
 * that is negative or NaN. The handle owns a stream, an event pair, the two tables and a grow-only scratch block on the device
 * (the chunks' partial results; a second pass of a shape allocates nothing); it is single-caller, like a decoder.
 */
enum { ALACGPU_NORM_STAT_NONE = 0, ALACGPU_NORM_STAT_MEAN = 1, ALACGPU_NORM_STAT_MEAN_VAR = 2, ALACGPU_NORM_STAT_MAX = 3 };
typedef struct alacgpu_norm_config {
    uint32_t bins;   /* 1 .. 4096 */
    uint32_t stat;   /* ALACGPU_NORM_STAT_* */
    float var_floor; /* > 0 */
    float range;     /* >= 0; read with ALACGPU_NORM_STAT_MAX only */
    float pad_value;
} alacgpu_norm_config;
typedef struct alacgpu_norm alacgpu_norm;
int alacgpu_norm_create(int device, const alacgpu_norm_config* config, const float* shift, const float* scale, alacgpu_norm** out);
void alacgpu_norm_destroy(alacgpu_norm* nm);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernels (valid after a sync). */
void* alacgpu_norm_stream(alacgpu_norm* nm);
int alacgpu_norm_synchronize(alacgpu_norm* nm);
int alacgpu_norm_last_ms(alacgpu_norm* nm, float* ms);
/* in_frames itself: the pass keeps every frame. 0 for a NULL handle. */
uint64_t alacgpu_norm_out_frames(const alacgpu_norm* nm, uint64_t in_frames);
/*
 * rows x frames x bins elements of d_in -> the same elements of d_out, which has strides of its own and may be d_in with the
 * same strides (in place; any other overlap is undefined). Every element (r, f < frames, b < bins) of the output is written
 * exactly once and nothing else is touched; a row with n_r = 0 is all pad_value. d_lengths: int32 [rows] on the device, or
 * NULL. d_stats: NULL, or [rows][2][bins] floats on the device: mean and rstd for MEAN_VAR, mean and 1.0 for MEAN, M in [r][0][0]
 * for MAX; +0.0 everywhere else and in every row with n_r = 0. rows = 0 or frames = 0 succeeds and touches nothing.
 * ALACGPU_E_ARG before any HIP call: a NULL handle; with work to do a NULL d_in or d_out, a base that is not 4-byte aligned,
 * neither inner stride equal to 1, an inner stride below the other axis' extent (the stride of an axis of one element is free),
 * a row stride below the row's extent, or sizes whose products overflow. Asynchronous on the handle's stream unless sync != 0:
 * the input must be complete, or ordered on that stream, before the call.
 */
int alacgpu_norm_device(alacgpu_norm* nm, const float* d_in, size_t in_row_stride, size_t in_frame_stride, size_t in_bin_stride,
                        size_t rows, size_t frames, const int32_t* d_lengths, float* d_out, size_t out_row_stride,
                        size_t out_frame_stride, size_t out_bin_stride, float* d_stats, int sync);
/* The plan the handle's kernels use: its numbers, the scratch block as it stands (address and bytes: they change only when a
 * pass needs more), and (where the pointers are not NULL and the capacities, counted in entries, suffice) the host copies of
 * shift and scale; shift_entries / scale_entries are bins, or 0 where none was given. */
typedef struct alacgpu_norm_info {
    uint32_t bins, stat, tile_frames, lds_bytes, shift_entries, scale_entries;
    uint64_t scratch_bytes, scratch_address;
} alacgpu_norm_info;
int alacgpu_norm_plan(const alacgpu_norm* nm, alacgpu_norm_info* info, float* shift_out, size_t shift_cap, float* scale_out,
                      size_t scale_cap);

/*
 * FRAME STACKING: float32 features [rows][frames][bins] with per-row lengths -> deltas, context splicing and subsampling with
 * lengths of their own, one pass on a handle of its own (k_stack.hip, alac_stack.h; the normalisation pass and
 * every other are untouched). The input is addressed as the normalisation pass's: element (r, f, b) at d + r * row_stride + f *
 * frame_stride + b * bin_stride (elements), one of the two inner strides 1, the stride of an axis of one element free;
 * n_r = clamp(d_lengths[r], 0, frames), frames where d_lengths is NULL.
 *     weights   Kaldi's DeltaFeatures: w_0 = [1], w_k = w_(k-1) convolved with the ramp j = -window .. window, divided by sum j^2;
 *               half-width M_k = k * window; exact integer numerators over (sum j^2)^k, rounded to float32 once at create
 *     deltas    d_k[t][b] = the chain acc = fmaf(w_k[i], x[clamp(t + i, 0, n_r - 1)][b], acc), i = -M_k .. M_k in that order from
 *               +0.0f, taps of weight zero skipped; d_0 = x, copied. Order 1 is torchaudio's compute_deltas(mode "replicate") with
 *               win_length 2 window + 1; order 2 is Kaldi's add-deltas (one clamp, on x), not compute_deltas applied twice
 *     output    G = ceil(frames / stride) frames of D = (left + right + 1) * (order + 1) * bins columns; m_r = ceil(n_r / stride);
 *               y[r][g][(c * (order + 1) + k) * bins + b] = d_k[clamp(g * stride + c - left, 0, n_r - 1)][b] for g < m_r and
 *               c = 0 .. left + right; pad_value for g >= m_r; d_out_lengths[r] = m_r
 * add-deltas is left = right = 0, stride 1; splice-feats is order 0; subsample-feats is the stride alone; FunASR's apply_lfr(m,
 * n) is left (m - 1) / 2, right m - 1 - left, stride n. The input at frames >= n_r is never read, whatever it holds. fmaf is
 * correctly rounded and nothing else rounds: the bits depend on the row's own data and n_r only.
 * alacgpu_stack_create is ALACGPU_E_ARG, before any HIP call, for a NULL config, bins outside [1, 4096], order above 2, window
 * outside [1, 8] with an order above 0, left or right above 16, stride outside [1, 64], or D above 4096. The handle owns a
 * stream, an event pair and the weights on the device; it is single-caller, like a decoder.
 */
typedef struct alacgpu_stack_config {
    uint32_t bins;   /* 1 .. 4096 */
    uint32_t order;  /* 0 .. 2 */
    uint32_t window; /* 1 .. 8; read with order > 0 only */
    uint32_t left;   /* 0 .. 16 frames of context in front */
    uint32_t right;  /* 0 .. 16 behind */
    uint32_t stride; /* 1 .. 64: every stride-th frame is kept */
    float pad_value;
} alacgpu_stack_config;
typedef struct alacgpu_stack alacgpu_stack;
int alacgpu_stack_create(int device, const alacgpu_stack_config* config, alacgpu_stack** out);
void alacgpu_stack_destroy(alacgpu_stack* st);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernel (valid after a sync). */
void* alacgpu_stack_stream(alacgpu_stack* st);
int alacgpu_stack_synchronize(alacgpu_stack* st);
int alacgpu_stack_last_ms(alacgpu_stack* st, float* ms);
/* G = ceil(in_frames / stride). 0 for a NULL handle. */
uint64_t alacgpu_stack_out_frames(const alacgpu_stack* st, uint64_t in_frames);
/*
 * rows x frames x bins elements of d_in -> rows x G x D elements of d_out, which has strides of its own (frame stride 1: [rows]
 * [D][G]; bin stride 1: [rows][G][D]) whatever the input's layout. Every element (r, g < G, j < D) of the output is written
 * exactly once and nothing else is touched but d_out_lengths (int32 [rows] on the device, or NULL). d_lengths: int32 [rows] on the
 * device, or NULL. rows = 0 or frames = 0 succeeds and touches nothing. ALACGPU_E_ARG before any HIP call: a NULL handle; with
 * work to do a NULL d_in or d_out, a base that is not 4-byte aligned, neither inner stride equal to 1, an inner stride below the
 * other axis' extent, a row stride below the row's extent, an output whose span of addresses meets the input's (there is no in
 * place: the shape differs), frames above 2^31 - 1, or sizes whose products overflow. Asynchronous on the handle's stream unless
 * sync != 0: the input must be complete, or ordered on that stream, before the call.
 */
int alacgpu_stack_device(alacgpu_stack* st, const float* d_in, size_t in_row_stride, size_t in_frame_stride, size_t in_bin_stride,
                         size_t rows, size_t frames, const int32_t* d_lengths, float* d_out, size_t out_row_stride,
                         size_t out_frame_stride, size_t out_bin_stride, int32_t* d_out_lengths, int sync);
/* The plan the handle's kernel uses: a tile is tile_out output frames of a row, stages at most tile_in input frames of tile_bins
 * bins at a time (tile_bins = bins unless the images of one output frame would not fit) in lds_bytes <= 25 600 of LDS, all
 * functions of the configuration alone; window is 0 at order 0; and (where the pointer is not NULL and the capacity, counted in
 * entries, suffices) the weights: w_1 (w1_entries = 2 window + 1, or 0), then w_2 (w2_entries = 4 window + 1, or 0). */
typedef struct alacgpu_stack_info {
    uint32_t bins, order, window, left, right, stride, columns, tile_out, tile_in, tile_bins, lds_bytes, w1_entries, w2_entries;
} alacgpu_stack_info;
int alacgpu_stack_plan(const alacgpu_stack* st, alacgpu_stack_info* info, float* weights_out, size_t weights_cap);

/*
 * SPECAUGMENT: float32 features [rows][frames][bins] with per-row lengths -> a time warp, frequency masks and time masks drawn
 * inside each row's own n_r frames, one pass on a handle of its own (k_specaug.hip, alac_specaug.h; the
 * normalisation pass, the stacking pass and every other are untouched). Input and output are addressed as the normalisation
 * pass's: element (r, f, b) at d + r * row_stride + f * frame_stride + b * bin_stride (elements), one of the two inner strides 1,
 * the stride of an axis of one element free; n_r = clamp(d_lengths[r], 0, frames), frames where d_lengths is NULL.
 *     words     Philox4x32-10 with Random123's constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 *               0xBB67AE85), key (seed low, seed high). Row r's identity is id = d_ids ? (uint64)d_ids[r] : row_base + r; its word j
 *               is output word j % 4 of the block at counter (id low, id high, j / 4, 0). A draw from [0, m) is the high 32 bits
 *               of word * m. A row consumes P = 2 + 2 freq_masks + 2 time_masks words whatever n_r is: an utterance's
 *               augmentation depends on (seed, id, n_r) only, never on the batch around it
 *     warp      words 0 and 1; only where warp (W) > 0 and n_r > 2 W: c = W + draw(n_r - 2 W), w = c - W + 1 + draw(2 W); output
 *               frames [0, w) are the source frames [0, c) resampled linearly, output frames [w, n_r) the source frames [c, n_r),
 *               each segment on its own; otherwise c = w = 0 and every element is copied
 *     resample  output frame t of a segment of a source frames and b output frames: num = (2 t + 1) a - b; num <= 0: i0 = 0, lq = 0;
 *               else i0 = num / (2 b), lq = ((num % (2 b)) << 23) / (2 b) in uint64; i1 = min(i0 + 1, a - 1). Where lq == 0 or
 *               i1 == i0, y = x[i0], copied and never multiplied; else y = fmaf((float)lq * 0x1p-23f, x[i1] - x[i0], x[i0]): linear
 *               interpolation with align_corners false, the position an exact rational, the weight floored to 2^-23
 *     masks     in output coordinates, behind the warp. Frequency mask i (words 2 + 2 i, 3 + 2 i): fw = draw(freq_width + 1),
 *               f0 = draw(bins - fw + 1), bins [f0, f0 + fw). Time mask i (the 2 time_masks words behind them): cap =
 *               min(time_width, (n_r * time_ratio_q16) >> 16), tw = draw(cap + 1), t0 = draw(n_r - tw + 1), frames [t0, t0 + tw):
 *               never outside [0, n_r). An element under any mask is mask_value
 *     padding   y = pad_value for f >= n_r; the input there is never read, whatever it holds. Lengths do not change
 * The integer draws are the same on every build, fmaf is correctly rounded and nothing else rounds but one subtraction.
 * alacgpu_specaug_create is ALACGPU_E_ARG, before any HIP call, for a NULL config, bins outside [1, 4096], freq_masks above 8,
 * freq_width above bins, time_masks above 16, time_width above 65535, time_ratio_q16 above 65536 or warp above 256. The handle
 * owns a stream and an event pair; it is single-caller, like a decoder.
 */
typedef struct alacgpu_specaug_config {
    uint32_t bins;           /* 1 .. 4096 */
    uint32_t freq_masks;     /* 0 .. 8 */
    uint32_t freq_width;     /* 0 .. bins: a frequency mask is at most this wide */
    uint32_t time_masks;     /* 0 .. 16 */
    uint32_t time_width;     /* 0 .. 65535: a time mask is at most this long */
    uint32_t time_ratio_q16; /* 0 .. 65536: and at most this share of n_r, in 1 / 65536; 65536: time_width alone caps it */
    uint32_t warp;           /* 0 .. 256: the warp's centre moves by at most this many frames; 0: no warp */
    float mask_value;
    float pad_value;
} alacgpu_specaug_config;
typedef struct alacgpu_specaug alacgpu_specaug;
int alacgpu_specaug_create(int device, const alacgpu_specaug_config* config, alacgpu_specaug** out);
void alacgpu_specaug_destroy(alacgpu_specaug* sa);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernel (valid after a sync). */
void* alacgpu_specaug_stream(alacgpu_specaug* sa);
int alacgpu_specaug_synchronize(alacgpu_specaug* sa);
int alacgpu_specaug_last_ms(alacgpu_specaug* sa, float* ms);
/*
 * rows x frames x bins elements of d_in -> the same elements of d_out, which has strides of its own and either layout. Every
 * element (r, f < frames, b < bins) of the output is written exactly once and nothing else is touched but d_draws: NULL, or int32
 * [rows][P] on the device, per row the resolved c, w, then (start, width) per mask in word order. d_lengths: int32 [rows] on the
 * device, or NULL; d_ids: int64 [rows] on the device, or NULL. rows = 0 or frames = 0 succeeds and touches nothing.
 * ALACGPU_E_ARG before any HIP call: a NULL handle; with work to do a NULL d_in or d_out, a base that is not aligned to its
 * element (d_ids: 8 bytes), neither inner stride equal to 1, an inner stride below the other axis' extent, a row stride below the
 * row's extent, frames above 2^31 - 1, sizes whose products overflow, or an output whose span of addresses meets the input's,
 * with one exception: d_out == d_in with the same three strides on a handle whose warp is 0 runs in place. Asynchronous on the
 * handle's stream unless sync != 0: the input must be complete, or ordered on that stream, before the call.
 */
int alacgpu_specaug_device(alacgpu_specaug* sa, const float* d_in, size_t in_row_stride, size_t in_frame_stride, size_t in_bin_stride,
                           size_t rows, size_t frames, const int32_t* d_lengths, uint64_t seed, uint64_t row_base, const int64_t* d_ids,
                           float* d_out, size_t out_row_stride, size_t out_frame_stride, size_t out_bin_stride, int32_t* d_draws,
                           int sync);
/* The plan the handle's kernel uses: the parameters, draws = P, and the tile: tile_out output frames of a row (a function of bins
 * alone) in lds_bytes <= 25 600 of LDS. */
typedef struct alacgpu_specaug_info {
    uint32_t bins, freq_masks, freq_width, time_masks, time_width, time_ratio_q16, warp, draws, tile_out, lds_bytes;
    float mask_value, pad_value;
} alacgpu_specaug_info;
int alacgpu_specaug_plan(const alacgpu_specaug* sa, alacgpu_specaug_info* info);

/*
 * WAVEFORM AUGMENTATION: float32 waveforms [rows][samples] with per-row lengths -> a random gain, noise from a bank at a random
 * SNR, dither, clamp and padding, one pass on a handle of its own between the clips and the features (k_waveaug.hip,
 * alac_waveaug.h; SpecAugment and every other pass are untouched). Row r is d_in + r * in_row_stride (elements),
 * n_r = clamp(d_lengths[r], 0, samples), samples where d_lengths is NULL. The bank is noise_rows clips at d_noise + k *
 * noise_row_stride of m_k = clamp(d_noise_lengths[k], 0, noise_samples) samples; a NULL bank or noise_rows = 0 is no noise.
 *     tables    snr_amp[i] = (float)10^(-(snr_lo_q8 + i) / 5120), gain_amp[i] = (float)10^((gain_lo_q8 + i) / 5120): computed in
 *               double at create, rounded once, uploaded; the device never calls pow
 *     words     Philox4x32-10 as SpecAugment's, key (seed low, seed high), id = d_ids ? (uint64)d_ids[r] : row_base + r. The fourth
 *               counter word is a stream number: SpecAugment's is 0, this pass's row draws are stream 2 (word j is output word
 *               j % 4 of the block at (id low, id high, j / 4, 2)) and its dither is stream 3 (sample t: the block at (id low,
 *               id high, t, 3)), so one (seed, ids) serves both passes
 *     draws     five words per row whatever n_r and the bank are: applied = noise_rows > 0 && draw(65536) < noise_prob_q16;
 *               k = draw(noise_rows); o = draw(m_k), and m_k = 0 clears applied; snr_i = draw(snr_hi_q8 - snr_lo_q8 + 1); gain_i =
 *               draw(gain_hi_q8 - gain_lo_q8 + 1); draw(m) is the high 32 bits of word * m. The noise under sample t is
 *               z_t = noise[k][(o + t) mod m_k]: the clip loops. d_draws: applied, k, o, snr_lo_q8 + snr_i, gain_lo_q8 + gain_i
 *     energies  Ex = sum x_t^2, En = sum z_t^2 over t < n_r only, in one order that depends on n_r alone: chunks of `tile`
 *               samples on the row's own index; in a chunk, lane l of 256 chains acc = fmaf(v, v, acc) from +0.0f over the samples
 *               of index = l mod 256 in increasing order; acc[l] += acc[l + s] for s = 128 .. 1; the chunks in order from +0.0f
 *     scalars   a = gain_amp[gain_i]; b = (sqrtf(Ex / En) * snr_amp[snr_i]) * a where applied, Ex > 0, En > 0 and both finite,
 *               else 0. d_stats: Ex, En (0 without noise), a, b
 *     output    t < n_r: v = a * x_t; b != 0: v = fmaf(b, z_t, v); dither != 0: v = fmaf(dither, g_t, v); clamp: v = v < -1 ? -1 :
 *               v > 1 ? 1 : v (a NaN stays one). t >= n_r: pad_value. Nothing at t >= n_r or behind m_k is read; a row with
 *               b == 0 never reads the bank. With a == 1, b == 0, no dither and no clamp a sample is 1.0f * x_t: its own bits,
 *               but a signalling NaN comes out quiet
 *     dither    the block's eight 16-bit halves h0 .. h7 (the low half of word 0 first): s = (h0 + h1 + h2 + h3) - (h4 + h5 + h6
 *               + h7), g = (float)s * 0x1.3988e2p-16f (the float nearest 1 / sqrt((2^32 - 1) * 2 / 3)): an Irwin-Hall(8) stand-in
 *               for a Gaussian of zero mean and unit variance, cut at +-4.9 sigma, bit-exact everywhere
 * alacgpu_waveaug_create is ALACGPU_E_ARG, before any HIP call, for a NULL config, a range outside [-16384, 16384], out of
 * order or more than 16384 (64 dB: 16 385 table entries) wide, noise_prob_q16 above 65536, a dither that is negative or not
 * finite, or clamp above 1. The handle owns a stream, an event pair, the two tables and a grow-only block for the partial sums;
 * it is single-caller, like a decoder.
 */
typedef struct alacgpu_waveaug_config {
    int32_t snr_lo_q8, snr_hi_q8;   /* -16384 .. 16384, lo <= hi <= lo + 16384: the SNR in 1 / 256 dB */
    int32_t gain_lo_q8, gain_hi_q8; /* likewise; 0, 0: no gain */
    uint32_t noise_prob_q16;        /* 0 .. 65536: the share of rows that get noise */
    float dither;                   /* >= 0; 0: none, and no random word is computed per sample */
    uint32_t clamp;                 /* 0 / 1: saturate to [-1, 1] */
    float pad_value;
} alacgpu_waveaug_config;
typedef struct alacgpu_waveaug alacgpu_waveaug;
int alacgpu_waveaug_create(int device, const alacgpu_waveaug_config* config, alacgpu_waveaug** out);
void alacgpu_waveaug_destroy(alacgpu_waveaug* wa);
/* The handle's hipStream_t as an opaque pointer, a wait for everything on it, and the duration of the last pass in
 * milliseconds: HIP events around its kernels (valid after a sync). */
void* alacgpu_waveaug_stream(alacgpu_waveaug* wa);
int alacgpu_waveaug_synchronize(alacgpu_waveaug* wa);
int alacgpu_waveaug_last_ms(alacgpu_waveaug* wa, float* ms);
/*
 * rows x samples elements of d_in -> the same elements of d_out, which has a row stride of its own and may be d_in itself with
 * the same stride (in place). Every element (r, t < samples) of the output is written exactly once and nothing else is touched
 * but d_draws (NULL, or int32 [rows][5] on the device) and d_stats (NULL, or float [rows][4] on the device). d_lengths, d_noise,
 * d_noise_lengths, d_ids (int64 [rows]): on the device, or NULL. rows = 0 or samples = 0 succeeds and touches nothing. Without a
 * bank and without d_stats one kernel runs; otherwise three. ALACGPU_E_ARG before any HIP call: a NULL handle; with work to do a
 * NULL d_in or d_out, a base that is not aligned to its element (d_ids: 8 bytes), a row stride below the row's samples, samples,
 * noise_samples or noise_rows above 2^31 - 1, sizes whose products overflow, an output whose span of addresses meets the
 * input's other than exactly in place, or a bank whose span meets the output's. Asynchronous on the handle's stream unless
 * sync != 0: the input must be complete, or ordered on that stream, before the call.
 */
int alacgpu_waveaug_device(alacgpu_waveaug* wa, const float* d_in, size_t in_row_stride, size_t rows, size_t samples,
                           const int32_t* d_lengths, const float* d_noise, size_t noise_row_stride, size_t noise_rows,
                           size_t noise_samples, const int32_t* d_noise_lengths, uint64_t seed, uint64_t row_base, const int64_t* d_ids,
                           float* d_out, size_t out_row_stride, int32_t* d_draws, float* d_stats, int sync);
/* The plan the handle's kernels use: the parameters, tile (the samples of a chunk), draws = 5, the LDS of a workgroup, the
 * scratch block as it stands (address and bytes: they change only when a pass needs more), and (where the pointers are not NULL
 * and the capacities, counted in entries, suffice) the two tables. */
typedef struct alacgpu_waveaug_info {
    int32_t snr_lo_q8, snr_hi_q8, gain_lo_q8, gain_hi_q8;
    uint32_t noise_prob_q16, clamp, tile, draws, snr_entries, gain_entries, lds_bytes;
    float dither, pad_value;
    uint32_t reserved;
    uint64_t scratch_bytes, scratch_address;
} alacgpu_waveaug_info;
int alacgpu_waveaug_plan(const alacgpu_waveaug* wa, alacgpu_waveaug_info* info, float* snr_out, size_t snr_cap, float* gain_out,
                         size_t gain_cap);

/* Thread-local description of the last ALACGPU_E_HIP / E_ARG / E_CONFIG failure. */
const char* alacgpu_last_error(void);

/* "alacgpu <semver> gfx950" */
const char* alacgpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ALACGPU_H */
