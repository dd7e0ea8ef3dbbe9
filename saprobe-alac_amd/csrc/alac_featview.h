/*
 * alac_featview.h — what a pass over a feature tensor needs and nothing of any one pass: a float32 tensor [rows][frames][bins]
 * given by three element strides, with per-row lengths, as plain host + device code (alac_featnorm.h, alac_stack.h and
 * alac_specaug.h stand on it).
 *
 * Element (r, f, b) is base[r * rs + f * fs + b * bs] (element strides); exactly one of fs / bs is 1 ("frames" layout: the bins
 * of a frame are contiguous; "bins" layout: the frames of a bin are). The stride of an axis of one element is free: the caller's
 * is replaced by the other axis' extent (strides_of). n_r = clamp(lengths[r], 0, frames), or frames where lengths is NULL
 * (length_of). Memory moves in LINES along the contiguous axis, 16 bytes at a time in the chunks of the ABSOLUTE address space
 * that lie inside a line (as alacwf::stage_tile), element by element at a line's two ends (lines_in, lines_out). All index
 * arithmetic is in 64 bits.
 */
#ifndef ALAC_FEATVIEW_H
#define ALAC_FEATVIEW_H

#include "alac_waveform.h"

namespace alacfv {

using alacwf::kThreads;

/* 16 bytes moved by one instruction */
typedef float F4 __attribute__((vector_size(16), may_alias));

/* the valid frames of a row */
ALAC_WF_FN uint64_t length_of(const int32_t* lengths, uint64_t frames, uint64_t row) {
    if (!lengths) return frames;
    const int32_t n = lengths[row];
    if (n <= 0) return 0u;
    return (uint64_t)n < frames ? (uint64_t)n : frames;
}

/* nl lines of len contiguous floats, line l at src + l * stride, into image[l * sl + e * se]: work item `tid` of kThreads takes
 * its 16-byte chunks of the absolute address space. Nothing outside the lines is read. */
ALAC_WF_FN void lines_in(const float* src, uint64_t stride, uint32_t nl, uint32_t len, float* image, uint32_t sl, uint32_t se,
                         uint32_t tid) {
    const uint32_t cpl = (len + 3u) / 4u + 1u; /* chunks that cover a line at any offset within its first */
    const uint32_t total = nl * cpl;
    for (uint32_t c = tid; c < total; c += kThreads) {
        const uint32_t l = c / cpl, k = c - l * cpl;
        const float* s = src + (uint64_t)l * stride;
        const int32_t e0 = (int32_t)(4u * k) - (int32_t)(((uintptr_t)s >> 2) & 3u);
        float* d = image + l * sl;
        if (e0 >= 0 && (uint32_t)e0 + 4u <= len) {
            const F4 v = *(const F4*)(s + e0);
            for (uint32_t j = 0; j < 4u; j++) d[((uint32_t)e0 + j) * se] = v[j];
        } else {
            for (int32_t j = 0; j < 4; j++)
                if (e0 + j >= 0 && (uint32_t)(e0 + j) < len) d[(uint32_t)(e0 + j) * se] = s[e0 + j];
        }
    }
}

/* the reverse: image[l * sl + e * se] to line l at dst + l * stride; exactly the lines' elements are written */
ALAC_WF_FN void lines_out(float* dst, uint64_t stride, uint32_t nl, uint32_t len, const float* image, uint32_t sl, uint32_t se,
                          uint32_t tid) {
    const uint32_t cpl = (len + 3u) / 4u + 1u;
    const uint32_t total = nl * cpl;
    for (uint32_t c = tid; c < total; c += kThreads) {
        const uint32_t l = c / cpl, k = c - l * cpl;
        float* d = dst + (uint64_t)l * stride;
        const int32_t e0 = (int32_t)(4u * k) - (int32_t)(((uintptr_t)d >> 2) & 3u);
        const float* s = image + l * sl;
        if (e0 >= 0 && (uint32_t)e0 + 4u <= len) {
            F4 v;
            for (uint32_t j = 0; j < 4u; j++) v[j] = s[((uint32_t)e0 + j) * se];
            *(F4*)(d + e0) = v;
        } else {
            for (int32_t j = 0; j < 4; j++)
                if (e0 + j >= 0 && (uint32_t)(e0 + j) < len) d[e0 + j] = s[(uint32_t)(e0 + j) * se];
        }
    }
}

/* ---- host only ------------------------------------------------------------------------------------------------------ */
/* one tensor's three strides -> 0 refused, 1 frames layout (bin stride 1, frames at least a line apart), 2 bins layout (frame
 * stride 1, bins at least a line apart); the stride of an axis of one element is free. The row stride is at least the row's
 * extent. */
inline int layout_of(uint64_t rs, uint64_t fs, uint64_t bs, uint64_t rows, uint64_t frames, uint32_t bins) {
    const uint64_t lim = (uint64_t)1 << 61;
    if (rs > lim / rows || fs > lim / frames || bs > lim / bins) return 0;
    int lay = 0;
    if (bs == 1u && (frames == 1u || fs >= bins)) lay = 1;
    else if (fs == 1u && (bins == 1u || bs >= frames)) lay = 2;
    if (!lay) return 0;
    const uint64_t extent = lay == 1 ? (frames == 1u ? 0u : (frames - 1u) * fs) + bins : (bins == 1u ? 0u : (bins - 1u) * bs) + frames;
    return rs >= extent ? lay : 0;
}

/* whether an entry takes the tensor at `base` (4-byte aligned, a layout that layout_of accepts; rows, frames, bins >= 1), and
 * the frame and bin strides its kernels run on: the caller's, but the free stride the other axis' extent. The kernels tell the
 * layout by the bin stride: 1 is the frames layout. */
inline bool strides_of(const void* base, uint64_t rs, uint64_t fs, uint64_t bs, uint64_t rows, uint64_t frames, uint32_t bins,
                       uint64_t* frame_stride, uint64_t* bin_stride) {
    if ((uintptr_t)base & 3u) return false;
    const int lay = layout_of(rs, fs, bs, rows, frames, bins);
    if (!lay) return false;
    *frame_stride = lay == 2 ? 1u : frames == 1u ? bins : fs;
    *bin_stride = lay == 1 ? 1u : bins == 1u ? frames : bs;
    return true;
}

/* the elements between a tensor's first and one past its last */
inline uint64_t extent_of(uint64_t rs, uint64_t fs, uint64_t bs, uint64_t rows, uint64_t frames, uint64_t cols) {
    return (rows - 1u) * rs + (frames - 1u) * fs + (cols - 1u) * bs + 1u;
}

}  // namespace alacfv

#endif /* ALAC_FEATVIEW_H */
