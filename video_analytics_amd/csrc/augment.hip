// Crop and horizontal flip of full-frame inputs on the device: the RandomCrop(224) /
// RandomHorizontalFlip() steps of getTransforms() (Sheet03/utils.py:143,145) for frames of any size, so that 320x240
// clips reach the 224x224 networks without a trip through the host.  The crops are drawn on the host
// (video_analytics_amd/augment.py) and handed over as DEVICE int32 {top, left, flip} triples.
//
// Both gathers are pure gathers: a thread writes runs of 4 consecutive output elements of a channel plane (the writes of a
// wave are one contiguous run) and reads source row top + y, column left + x -- or left + out_w - 1 - x when flipped, the
// same contiguous source segment in reverse order.  A wave whose elements straddle two output rows reads two such
// segments.  No LDS.  Ten-crop evaluation uses the same kernels with V views per source plane.
#include "va_internal.h"
#include <algorithm>
#include <type_traits>

// A crop triple as the kernels use it: offsets clamped to the frame, so that no crop value can address memory outside
// it (the host wrappers reject such crops before they get here).
struct CropWin {
    int top, left, flip;
};

__device__ __forceinline__ CropWin load_crop(const int* __restrict__ crops, int i, int h, int w, int out_h, int out_w)
{
    CropWin c;
    c.top = min(max(crops[3 * i], 0), h - out_h);
    c.left = min(max(crops[3 * i + 1], 0), w - out_w);
    c.flip = crops[3 * i + 2] != 0;
    return c;
}

// S10 then S9, for V views of every clip: flow f32 [n_clips][2L][h][w] (= [n_clips*L][2][h][w]) -> stack f32
// [n_clips][V][2L][out_h][out_w].  Output plane o = (b*V + v)*2L + c reads source plane b*2L + c through crop row o.
// Block row blockIdx.y = (b*2L + c)*V + v: the V views of one source plane are adjacent in dispatch order, so the
// re-reads of a plane come from L2 / the Infinity Cache.  The quantisation and normalisation are k_flow_to_stack's
// expressions in its order; the flip mirrors the quantised image.  With invert_x set, a flipped x-flow plane (c even)
// also becomes q -> 255 - q (the TSN convention); with it clear, as in the reference, the sign of the x flow is kept.
// V = 1, one clip of n_pairs pairs and invert_x = 0 is va_flow_to_stack_crop: o = blockIdx.y = the source plane.
//
// The kernel is write-bound: each thread writes kGatherSteps runs of 4 consecutive outputs (one 16-byte store when the
// plane holds a multiple of 4 floats; one 16-byte load when the crop's left offset is a multiple of 4 as well), so that a
// workgroup writes 16 KB instead of 1 KB (measured on the ten-view volume: one float per thread spent more time launching
// workgroups than moving bytes).
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kGatherSteps = 4;
constexpr int kGatherPerBlock = 256 * 4 * kGatherSteps;

//
// SNIPPETS (S15, va_flow_to_stack_snippets): clip b is snippet b of ONE video of n_pairs flow fields and its window starts
// at pair starts[b] (clamped to [0, n_pairs - L]), so that output plane o reads source plane 2*(starts[b] + c/2) + c%2 =
// 2*starts[b] + c: windows that overlap in the source instead of n copies of the flow.  The block order is the same,
// snippet-major with the V views of a plane adjacent; a plane that the next snippet reads again was last read one
// snippet earlier, i.e. 2L full-frame planes (6 MB at 320x240) and V*2L streamed output planes (40 MB) ago: those re-reads
// come from the Infinity Cache, the V re-reads within a snippet from L2.  Everything after the plane's address is shared.
//
// SRC (S40, va_flowq_to_stack_snippets): float is the flow itself; unsigned char is a STORED flow, the 8-bit flow images
// va_flow_quantize_u8 wrote (S39), i.e. the q of the expressions below computed once and kept.  The u8 form reads q, applies
// the inversion and the normalisation and so gives the float form's bits; its aligned source run is one 4-byte load.
template <bool SNIPPETS, typename SRC>
__global__ void __launch_bounds__(256) k_flow_crop_stack(const SRC* __restrict__ flow, const int* __restrict__ crops,
                                                         const int* __restrict__ starts, int n_pairs,
                                                         float* __restrict__ stack, int w, int h, int out_w, int out_h,
                                                         int chans, int n_views, int invert_x, int vec4, float bound,
                                                         float mean, float stdv)
{
    const int src = blockIdx.y / n_views, v = blockIdx.y - src * n_views;
    const int b = src / chans, c = src - b * chans;
    const int o = (b * n_views + v) * chans + c;
    const int n = out_w * out_h;
    const CropWin cw = load_crop(crops, o, h, w, out_h, out_w);
    const bool inv = invert_x && cw.flip && (c & 1) == 0;
    const int splane = SNIPPETS ? 2 * min(max(starts[b], 0), n_pairs - chans / 2) + c : src;
    const SRC* __restrict__ plane = flow + (size_t)splane * h * w + (size_t)cw.top * w;
    float* __restrict__ dst = stack + (size_t)o * n;
    // vec4 bit 1: 16-byte aligned flow (u8: 4-byte aligned), w and out_w multiples of 4; with a left offset of 4k too, every
    // run of 4 outputs (never split between rows) reads one aligned float4 (u8: one aligned 32-bit word)
    const bool ld4 = (vec4 & 2) && (cw.left & 3) == 0;
#pragma unroll
    for (int s = 0; s < kGatherSteps; ++s) {
        const int i0 = ((blockIdx.x * kGatherSteps + s) * blockDim.x + threadIdx.x) * 4;
        if (i0 >= n) continue;
        int y = i0 / out_w, x = i0 - y * out_w;
        float r[4];
        if constexpr (std::is_same<SRC, float>::value) {
            float val[4];
            if (ld4) {  // the 4 sources are one aligned 16-byte run of row y (reversed when flipped)
                const int sx = cw.flip ? cw.left + out_w - 4 - x : cw.left + x;
                const f32x4 f = *reinterpret_cast<const f32x4*>(plane + (size_t)y * w + sx);
#pragma unroll
                for (int k = 0; k < 4; ++k) val[k] = cw.flip ? f[3 - k] : f[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sx = cw.left + (cw.flip ? out_w - 1 - x : x);
                    val[k] = i0 + k < n ? plane[(size_t)y * w + sx] : 0.0f;  // plane c of clip b: pair c/2, plane c%2
                    if (++x == out_w) x = 0, ++y;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float t = (255.0f * (val[k] + bound)) / (2.0f * bound);
                float q = rintf(fminf(fmaxf(t, 0.0f), 255.0f));
                if (inv) q = 255.0f - q;
                r[k] = (q / 255.0f - mean) / stdv;
            }
        } else {
            unsigned qv[4];
            if (ld4) {  // the 4 sources are one aligned 4-byte run of row y (reversed when flipped)
                const int sx = cw.flip ? cw.left + out_w - 4 - x : cw.left + x;
                const unsigned u = *reinterpret_cast<const unsigned*>(plane + (size_t)y * w + sx);
#pragma unroll
                for (int k = 0; k < 4; ++k) qv[k] = (u >> (8 * (cw.flip ? 3 - k : k))) & 255u;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sx = cw.left + (cw.flip ? out_w - 1 - x : x);
                    qv[k] = i0 + k < n ? (unsigned)plane[(size_t)y * w + sx] : 0u;
                    if (++x == out_w) x = 0, ++y;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float q = (float)qv[k];
                if (inv) q = 255.0f - q;
                r[k] = (q / 255.0f - mean) / stdv;
            }
        }
        if (vec4 & 1) {  // 16-byte aligned stack and planes of a multiple of 4 floats: the run lies in the plane, aligned
            // streamed past the caches: the volume is written once and read by the next kernel, the flow planes are not
            __builtin_nontemporal_store(f32x4{r[0], r[1], r[2], r[3]}, reinterpret_cast<f32x4*>(dst + i0));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < n) dst[i0 + k] = r[k];
        }
    }
}

// S39, the stored flow: flow f32 [n] -> out u8 [n], q = rintf(fminf(fmaxf(t, 0), 255)) with k_flow_crop_stack's t (a NaN
// becomes 0: fmaxf returns its other operand).  Element-wise over the whole array; a thread converts kGatherSteps runs of 4
// consecutive elements: one 16-byte load when ld4 (flow 16-byte aligned), one 4-byte store when st4 (out 4-byte aligned).
// The last run of an array that is no multiple of 4 long goes element by element.
__global__ void __launch_bounds__(256) k_flow_quantize_u8(const float* __restrict__ flow, unsigned char* __restrict__ out,
                                                          size_t n, int ld4, int st4, float bound)
{
#pragma unroll
    for (int s = 0; s < kGatherSteps; ++s) {
        const size_t i0 = (((size_t)blockIdx.x * kGatherSteps + s) * blockDim.x + threadIdx.x) * 4;
        if (i0 >= n) continue;
        const bool whole = i0 + 4 <= n;
        float val[4];
        if (ld4 && whole) {
            const f32x4 f = *reinterpret_cast<const f32x4*>(flow + i0);
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = f[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = i0 + k < n ? flow[i0 + k] : 0.0f;
        }
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = (255.0f * (val[k] + bound)) / (2.0f * bound);
            q[k] = (unsigned)rintf(fminf(fmaxf(t, 0.0f), 255.0f));
        }
        if (st4 && whole) {
            *reinterpret_cast<unsigned*>(out + i0) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < n) out[i0 + k] = (unsigned char)q[k];
        }
    }
}

// S10 on u8 images, V views of each: src [n][c][h][w] (NHWC = false) or [n][h][w][c] (NHWC = true) -> dst
// [n*V][c][out_h][out_w]; output image i reads source image i / V through crop row i, shared by its channels.  Block row
// blockIdx.y = i * c + channel (the views of one source image are adjacent).  Each thread writes kGatherSteps runs of 4
// consecutive bytes (one 4-byte store when vec4 says the runs are aligned), as k_flow_crop_stack does.
template <bool NHWC>
__global__ void __launch_bounds__(256) k_crop_images_u8(const unsigned char* __restrict__ src, const int* __restrict__ crops,
                                                        unsigned char* __restrict__ dst, int c, int w, int h, int out_w,
                                                        int out_h, int n_views, int vec4)
{
    const int img = blockIdx.y / c, chn = blockIdx.y - img * c;
    const int simg = img / n_views;
    const int n = out_w * out_h;
    const CropWin cw = load_crop(crops, img, h, w, out_h, out_w);
    unsigned char* __restrict__ out = dst + (size_t)blockIdx.y * n;
#pragma unroll
    for (int s = 0; s < kGatherSteps; ++s) {
        const int i0 = ((blockIdx.x * kGatherSteps + s) * blockDim.x + threadIdx.x) * 4;
        if (i0 >= n) continue;
        int y = i0 / out_w, x = i0 - y * out_w;
        unsigned r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sy = cw.top + y, sx = cw.left + (cw.flip ? out_w - 1 - x : x);
            const size_t si = NHWC ? (((size_t)simg * h + sy) * w + sx) * c + chn : (((size_t)simg * c + chn) * h + sy) * w + sx;
            r[k] = i0 + k < n ? src[si] : 0u;
            if (++x == out_w) x = 0, ++y;
        }
        if (vec4) {
            *reinterpret_cast<unsigned*>(out + i0) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k < n) out[i0 + k] = (unsigned char)r[k];
        }
    }
}

// ---------------------------------------------------------------- S17: crop-resize gather ------
//
// Scale jittering is the one input transform that resamples: a crop of ch x cw source pixels becomes a
// 224 x 224 input by bilinear interpolation with half-pixel centres and no antialiasing (align_corners = False), confined to
// the crop.  One table row {src, top, left, ch, cw, flip} per output plane (flow) or output image (u8); src is explicit, so
// snippet windows, overlaps and shared crops are all the host's table.  At ch = cw = 224 every weight is exactly 0 and the
// result is S10's gather bit for bit.
//
// A thread produces 4 x 4 outputs: its four columns' taps (x0, x1, ax) once, then row by row the two source rows' taps.  A
// workgroup of 448 threads = 8 row groups x 56 column groups writes 32 output rows; 7 workgroups a plane, no thread out of
// range.  The stores of a row group's 56 threads are one contiguous output row (896 bytes of f32, 224 of u8).  Block row
// blockIdx.y = the table row: the host emits rows snippet-major, so the planes a neighbouring snippet reads again, and the
// channels of one image, are adjacent in dispatch order (L2 / Infinity Cache), as in the gathers above.
constexpr int kResizeSize = 224;
constexpr int kResizeColGroups = kResizeSize / 4;                    // 56
constexpr int kResizeRowGroups = 8;                                  // per workgroup
constexpr int kResizeThreads = kResizeColGroups * kResizeRowGroups;  // 448 = 7 waves
constexpr int kResizeBlocks = kResizeSize / (4 * kResizeRowGroups);  // 7

struct ResizeWin {
    int src, top, left, ch, cw, flip;
};

// a table row clamped so that no value can address memory outside source plane / image [0, n_src) (the host wrappers
// reject such rows before they get here)
__device__ __forceinline__ ResizeWin load_resize(const int* __restrict__ table, int i, int n_src, int h, int w)
{
    const int* t = table + 6 * (size_t)i;
    ResizeWin r;
    r.src = min(max(t[0], 0), n_src - 1);
    r.ch = min(max(t[3], 1), h);
    r.cw = min(max(t[4], 1), w);
    r.top = min(max(t[1], 0), h - r.ch);
    r.left = min(max(t[2], 0), w - r.cw);
    r.flip = t[5] != 0;
    return r;
}

// S17's position of output index o along an axis of `size` source pixels, in its written order (plain float32, no fmaf)
__device__ __forceinline__ void resize_tap(int o, int size, int& i0, int& i1, float& a)
{
    const float s = (float)size / 224.0f;
    float u = ((float)o + 0.5f) * s - 0.5f;
    u = fminf(fmaxf(u, 0.0f), (float)(size - 1));
    i0 = (int)floorf(u);
    a = u - (float)i0;
    i1 = min(i0 + 1, size - 1);
}

// S12's bilinear form
__device__ __forceinline__ float resize_lerp(float A, float B, float C, float D, float ax, float ay)
{
    const float t = A + ax * (B - A);
    const float b = C + ax * (D - C);
    return t + ay * (b - t);
}

// flow f32 [n_src/2][2][h][w] -> stack f32 [n_out][224][224]: S17, then S9 in S9's order; TSN inversion as S10's.
// SRC = unsigned char (S41, va_flowq_to_stack_resize): a stored flow's 8-bit images are resampled as images, TSN's order:
// qr = the value k_resize_images_u8 writes for the plane, then the inversion, then the normalisation.
template <typename SRC>
__global__ void __launch_bounds__(kResizeThreads) k_flow_resize_stack(const SRC* __restrict__ flow, const int* __restrict__ table,
                                                                      float* __restrict__ stack, int n_src, int w, int h,
                                                                      int invert_x, int vec4, float bound, float mean, float stdv)
{
    const int o = blockIdx.y;
    const ResizeWin r = load_resize(table, o, n_src, h, w);
    const int cg = threadIdx.x % kResizeColGroups, rg = blockIdx.x * kResizeRowGroups + threadIdx.x / kResizeColGroups;
    const bool inv = invert_x && r.flip && (r.src & 1) == 0;
    const SRC* __restrict__ plane = flow + (size_t)r.src * h * w + (size_t)r.top * w + r.left;
    float* __restrict__ dst = stack + (size_t)o * (kResizeSize * kResizeSize) + 4 * cg;
    int x0[4], x1[4];
    float ax[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = 4 * cg + k;
        resize_tap(r.flip ? kResizeSize - 1 - x : x, r.cw, x0[k], x1[k], ax[k]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = 4 * rg + j;
        int y0, y1;
        float ay;
        resize_tap(y, r.ch, y0, y1, ay);
        const SRC* __restrict__ ra = plane + (size_t)y0 * w;
        const SRC* __restrict__ rb = plane + (size_t)y1 * w;
        float q4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float val = resize_lerp((float)ra[x0[k]], (float)ra[x1[k]], (float)rb[x0[k]], (float)rb[x1[k]], ax[k], ay);
            const float t = std::is_same<SRC, float>::value ? (255.0f * (val + bound)) / (2.0f * bound) : val;
            float q = rintf(fminf(fmaxf(t, 0.0f), 255.0f));
            if (inv) q = 255.0f - q;
            q4[k] = (q / 255.0f - mean) / stdv;
        }
        if (vec4) {  // 16-byte aligned stack: streamed past the caches, as k_flow_crop_stack's
            __builtin_nontemporal_store(f32x4{q4[0], q4[1], q4[2], q4[3]}, reinterpret_cast<f32x4*>(dst + (size_t)y * kResizeSize));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[(size_t)y * kResizeSize + k] = q4[k];
        }
    }
}

// u8 images [n_src][c][h][w] (NHWC = false) or [n_src][h][w][c] (true) -> dst u8 [n_out][c][224][224]; block row
// blockIdx.y = output image * c + channel; the value is (u8) rintf(clamp(val, 0, 255)) on the u8 values as floats
template <bool NHWC>
__global__ void __launch_bounds__(kResizeThreads) k_resize_images_u8(const unsigned char* __restrict__ src,
                                                                     const int* __restrict__ table, unsigned char* __restrict__ dst,
                                                                     int n_src, int c, int w, int h, int vec4)
{
    const int img = blockIdx.y / c, chn = blockIdx.y - img * c;
    const ResizeWin r = load_resize(table, img, n_src, h, w);
    const int cg = threadIdx.x % kResizeColGroups, rg = blockIdx.x * kResizeRowGroups + threadIdx.x / kResizeColGroups;
    // element (sy, sx) of the channel plane: base[sy * sy_stride + sx * sx_stride]
    const size_t sx_stride = NHWC ? (size_t)c : 1, sy_stride = (size_t)w * sx_stride;
    const unsigned char* __restrict__ base =
        src + (NHWC ? (size_t)r.src * h * w * c + chn : ((size_t)r.src * c + chn) * h * w) + r.top * sy_stride + r.left * sx_stride;
    unsigned char* __restrict__ out = dst + (size_t)blockIdx.y * (kResizeSize * kResizeSize) + 4 * cg;
    int x0[4], x1[4];
    float ax[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = 4 * cg + k;
        resize_tap(r.flip ? kResizeSize - 1 - x : x, r.cw, x0[k], x1[k], ax[k]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = 4 * rg + j;
        int y0, y1;
        float ay;
        resize_tap(y, r.ch, y0, y1, ay);
        const unsigned char* __restrict__ ra = base + y0 * sy_stride;
        const unsigned char* __restrict__ rb = base + y1 * sy_stride;
        unsigned q4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float val = resize_lerp((float)ra[x0[k] * sx_stride], (float)ra[x1[k] * sx_stride], (float)rb[x0[k] * sx_stride],
                                          (float)rb[x1[k] * sx_stride], ax[k], ay);
            q4[k] = (unsigned)rintf(fminf(fmaxf(val, 0.0f), 255.0f));
        }
        if (vec4) {
            *reinterpret_cast<unsigned*>(out + (size_t)y * kResizeSize) = q4[0] | (q4[1] << 8) | (q4[2] << 16) | (q4[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) out[(size_t)y * kResizeSize + k] = (unsigned char)q4[k];
        }
    }
}

// S23, the RGB-difference gather: frames u8 [n_frames][3][h][w] (NHWC = false) or [n_frames][h][w][3] (true) -> stack f32
// [n_out][3*D][224][224].  Block row blockIdx.y = the output ITEM (not a plane): table row {src, top, left, ch, cw, flip} with
// src the first of the item's D + 1 frames.  The thread layout is k_resize_images_u8's (4 x 4 outputs a thread, 448 threads,
// 7 workgroups an item); a thread computes its column taps once per item and its four rows' taps once, then walks channel
// by channel through frames src .. src + D, keeping the previous frame's 16 resampled u8 values in registers, so that every
// source frame is read once.  Plane 3j + c = (float)((int)r_{j+1,c} - (int)r_{j,c}) / den_c with r the value
// k_resize_images_u8 writes: each difference row of a thread is one 16-byte non-temporal store (scalar stores when the stack
// is not 16-byte aligned).  No LDS, no atomics.
template <bool NHWC>
__global__ void __launch_bounds__(kResizeThreads) k_rgbdiff_stack(const unsigned char* __restrict__ src,
                                                                  const int* __restrict__ table, float* __restrict__ stack,
                                                                  int n_frames, int n_diff, int w, int h, int vec4, float den0,
                                                                  float den1, float den2)
{
    constexpr int kPlane = kResizeSize * kResizeSize;
    const int o = blockIdx.y;
    const ResizeWin r = load_resize(table, o, n_frames - n_diff, h, w);  // src + n_diff <= n_frames - 1
    const int cg = threadIdx.x % kResizeColGroups, rg = blockIdx.x * kResizeRowGroups + threadIdx.x / kResizeColGroups;
    // element (sy, sx) of channel chn of frame f: src[f * frame + chn * chn_stride + sy * sy_stride + sx * sx_stride]; the
    // frame, channel and crop corner are the same for the whole workgroup (a scalar base), a thread's own taps 32-bit offsets
    // from it (the entry point refuses frames of 2^31 bytes or more)
    const int sx_stride = NHWC ? 3 : 1, sy_stride = w * sx_stride;
    const size_t frame = (size_t)3 * h * w, chn_stride = NHWC ? 1 : (size_t)h * w;
    // (the table row is one per workgroup: saying so keeps the base in scalar registers and the loads in base + offset form)
    const size_t corner = (size_t)__builtin_amdgcn_readfirstlane(r.src) * frame +
                          (size_t)__builtin_amdgcn_readfirstlane(r.top * sy_stride + r.left * sx_stride);
    const unsigned char* __restrict__ first = src + corner;
    float* __restrict__ out = stack + (size_t)o * 3 * n_diff * kPlane + (size_t)(4 * rg) * kResizeSize + 4 * cg;
    unsigned x0[4], x1[4], ra[4], rb[4];
    float ax[4], ay[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = 4 * cg + k;
        int i0, i1;
        resize_tap(r.flip ? kResizeSize - 1 - x : x, r.cw, i0, i1, ax[k]);
        x0[k] = (unsigned)(i0 * sx_stride);
        x1[k] = (unsigned)(i1 * sx_stride);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int y0, y1;
        resize_tap(4 * rg + j, r.ch, y0, y1, ay[j]);
        ra[j] = (unsigned)(y0 * sy_stride);
        rb[j] = (unsigned)(y1 * sy_stride);
    }
    for (int chn = 0; chn < 3; ++chn) {
        const float den = chn == 0 ? den0 : (chn == 1 ? den1 : den2);
        const unsigned char* __restrict__ plane = first + chn * chn_stride;
        int prev[16];
#pragma unroll 1
        for (int f = 0; f <= n_diff; ++f) {
            int cur[16];
            // The frame's offset and the taps are made opaque to the optimiser here (no instruction is emitted): the loads
            // then take the form scalar base + 32-bit offset, 16 tap registers in all.  Without it the 64 addresses are
            // hoisted out of the loop as 64 per-thread 64-bit pointers advanced frame by frame: 128 registers, and spills.
            size_t foff = f * frame;
            asm volatile("" : "+s"(foff));
            const unsigned char* __restrict__ base = plane + foff;
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(x0[k]), "+v"(x1[k]), "+v"(ra[k]), "+v"(rb[k]));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float val = resize_lerp((float)base[ra[j] + x0[k]], (float)base[ra[j] + x1[k]], (float)base[rb[j] + x0[k]],
                                                  (float)base[rb[j] + x1[k]], ax[k], ay[j]);
                    cur[4 * j + k] = (int)rintf(fminf(fmaxf(val, 0.0f), 255.0f));
                }
            }
            if (f > 0) {
                float* __restrict__ dst = out + (size_t)(3 * (f - 1) + chn) * kPlane;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float d4[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) d4[k] = (float)(cur[4 * j + k] - prev[4 * j + k]) / den;
                    if (vec4) {  // 16-byte aligned stack: streamed past the caches, as k_flow_resize_stack's
                        __builtin_nontemporal_store(f32x4{d4[0], d4[1], d4[2], d4[3]}, reinterpret_cast<f32x4*>(dst + j * kResizeSize));
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) dst[j * kResizeSize + k] = d4[k];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) prev[i] = cur[i];
        }
    }
}

// ---------------------------------------------------------------- S32-S34: colour jitter ------
//
// ColorJitter's four ops and the PCA lighting on u8 [n][3][h][w]: PIL's arithmetic, value for value.
// One table row of 8 floats per image, {op0, op1, op2, op3, f_brightness, f_contrast, f_saturation, hue_shift}: the op codes
// (0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue) in application order.  Contrast blends with the mean gray level of
// the image as it is when contrast's turn comes, so it needs a sum over the whole image: k_color_jitter_sums applies the ops
// that precede contrast in registers and writes one integer partial sum per workgroup, k_color_jitter_apply adds an image's
// partials (integers: any order gives the same sum), forms m and applies the whole row and the lighting.  Both kernels have
// one geometry: kJitterThreads threads, a thread handles runs of 4 consecutive pixels of the plane (one 4-byte load and
// store per channel when the planes are 4-byte aligned); an image of more than 1024 x VA_COLOR_JITTER_PARTIALS pixels gets
// that many workgroups, which stride over it by the grid's width.  Pure element-wise work besides the sum: no LDS but the
// reduction's, no atomics, bit-reproducible.  dst may be src: a thread reads only the pixels it writes.
constexpr int kJitterThreads = 256;
// one run of 4 pixels per thread, 1024 pixels a workgroup, until an image has VA_COLOR_JITTER_PARTIALS workgroups (512 x 512);
// the hue's f64 arithmetic makes a thread's work long, and at 24 images of 224 x 224 four runs a thread left one wave per SIMD
// with nothing to hide its latencies behind (measured: 25.9 us for k_color_jitter_apply)
constexpr int kJitterSteps = 1;
constexpr int kJitterPerBlock = kJitterThreads * 4 * kJitterSteps;
enum { kJitterNone = 0, kJitterBrightness = 1, kJitterContrast = 2, kJitterSaturation = 3, kJitterHue = 4 };

struct JitterRow {
    unsigned ops;             // op k in bits 4k .. 4k+3 (no array: a run-time index would move the row out of registers)
    float fb, fc, fs;         // the blend factors of brightness, contrast, saturation
    int shift;
    int contrast_at;          // the place of contrast among the four ops, 4 when the row has none
};

// a table row clamped so that no value leaves the arithmetic's domain (the host wrappers reject such rows before they get
// here): codes to 0..4 with a repeated code becoming none, factors to [0, 1e30] (NaN: 0), the shift to 0..255; with_contrast
// clear turns contrast into none (no workspace: the caller stated that no row has it)
__device__ __forceinline__ JitterRow load_jitter(const float* __restrict__ table, int i, bool with_contrast)
{
    const float* t = table + 8 * (size_t)i;
    JitterRow r;
    unsigned seen = with_contrast ? 1u : 1u | (1u << kJitterContrast);
    r.ops = 0;
    r.contrast_at = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int c = (int)fminf(fmaxf(t[k], 0.0f), 4.0f);
        if (seen & (1u << c)) c = kJitterNone;
        seen |= 1u << c;
        r.ops |= (unsigned)c << (4 * k);
        if (c == kJitterContrast) r.contrast_at = k;
    }
    r.fb = fminf(fmaxf(t[4], 0.0f), 1.0e30f);
    r.fc = fminf(fmaxf(t[5], 0.0f), 1.0e30f);
    r.fs = fminf(fmaxf(t[6], 0.0f), 1.0e30f);
    r.shift = (int)fminf(fmaxf(t[7], 0.0f), 255.0f);
    return r;
}

// Image.blend: t = d + f*(v - d) in f32, multiply then add; 0 <= f <= 1 keeps t in [0, 255], so one clamped form serves
// both of PIL's branches
__device__ __forceinline__ int jitter_blend(int d, int v, float f)
{
    const float t = (float)d + f * (float)(v - d);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int jitter_gray(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// RGB -> HSV, h += shift (mod 256), HSV -> RGB with PIL's operand widths (S32): the hue expression, fmod(h/6 + 1, 1) and
// the scalings by 255 in double, the ratios in f32; the way back in double with f, fs and fs*f rounded to f32
__device__ __forceinline__ void jitter_hue(int& r, int& g, int& b, int shift)
{
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    if (mx == mn) return;  // h = s = 0: the way back gives r = g = b = v whatever the shifted hue
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx)
        h = (float)((double)bc - (double)gc);
    else if (g == mx)
        h = (float)(2.0 + (double)rc - (double)bc);
    else
        h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;           // in [5/6, 11/6]
    h = (float)(x >= 1.0 ? x - 1.0 : x);              // fmod(x, 1.0), exact
    const int uh = min(max((int)((double)h * 255.0), 0), 255);
    const int us = min(max((int)((double)s * 255.0), 0), 255);
    if (us == 0) {
        r = g = b = mx;
        return;
    }
    const int hh = (uh + shift) & 255;
    const double h6 = (double)hh * 6.0 / 255.0;
    const double fl = floor(h6);
    const float f = (float)(h6 - fl);
    const float fs = (float)((double)us / 255.0);
    const double v = (double)mx;
    const int p = min(max((int)round(v * (1.0 - (double)fs)), 0), 255);
    const int q = min(max((int)round(v * (1.0 - (double)(fs * f))), 0), 255);
    const int t = min(max((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
    switch ((int)fl % 6) {
        case 0: r = mx, g = t, b = p; break;
        case 1: r = q, g = mx, b = p; break;
        case 2: r = p, g = mx, b = t; break;
        case 3: r = p, g = q, b = mx; break;
        case 4: r = t, g = p, b = mx; break;
        default: r = mx, g = p, b = q; break;
    }
}

// ops [first, last) of the row on one pixel; m: contrast's gray value
__device__ __forceinline__ void jitter_ops(const JitterRow& row, int first, int last, int m, int& r, int& g, int& b)
{
    for (int k = first; k < last; ++k) {
        const int op = (int)((row.ops >> (4 * k)) & 15u);  // the same for the whole workgroup
        if (op == kJitterBrightness) {
            r = jitter_blend(0, r, row.fb), g = jitter_blend(0, g, row.fb), b = jitter_blend(0, b, row.fb);
        } else if (op == kJitterContrast) {
            r = jitter_blend(m, r, row.fc), g = jitter_blend(m, g, row.fc), b = jitter_blend(m, b, row.fc);
        } else if (op == kJitterSaturation) {
            const int L = jitter_gray(r, g, b);
            r = jitter_blend(L, r, row.fs), g = jitter_blend(L, g, row.fs), b = jitter_blend(L, b, row.fs);
        } else if (op == kJitterHue) {
            jitter_hue(r, g, b, row.shift);
        }
    }
}

// the run of 4 pixels at plane index i0 of an image's three planes (plane: its pixel count); pixels past the plane read 0
__device__ __forceinline__ void jitter_load(const unsigned char* __restrict__ img, int plane, int i0, int vec4, int (&px)[3][4])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned char* __restrict__ p = img + (size_t)c * plane + i0;
        if (vec4) {
            const unsigned u = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) px[c][k] = (int)((u >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) px[c][k] = i0 + k < plane ? (int)p[k] : 0;
        }
    }
}

// the sum of v over the workgroup, in every thread: shuffles within a wave, then the waves' sums through LDS
__device__ __forceinline__ unsigned long long jitter_block_sum(unsigned long long v)
{
    __shared__ unsigned long long wave_sum[kJitterThreads / 64];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < kJitterThreads / 64; ++k) s += wave_sum[k];
    return s;
}

// launch one: partials u32 [n][gridDim.x]; workgroup (x, img) writes the sum of the gray level, after the ops that precede
// contrast, over its pixels of image img.  Images whose row has no contrast write nothing.
__global__ void __launch_bounds__(kJitterThreads) k_color_jitter_sums(const unsigned char* __restrict__ src,
                                                                      const float* __restrict__ table,
                                                                      unsigned* __restrict__ partials, int plane, int vec4)
{
    const int img = blockIdx.y;
    const JitterRow row = load_jitter(table, img, true);
    if (row.contrast_at == 4) return;
    const unsigned char* __restrict__ base = src + (size_t)img * 3 * plane;
    unsigned sum = 0;  // <= 2^31 / gridDim.x pixels x 255 a workgroup (the entry point bounds the plane): no overflow
    for (int i0 = (blockIdx.x * kJitterThreads + threadIdx.x) * 4; i0 < plane; i0 += gridDim.x * kJitterThreads * 4) {
        int px[3][4];
        jitter_load(base, plane, i0, vec4, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            jitter_ops(row, 0, row.contrast_at, 0, px[0][k], px[1][k], px[2][k]);
            if (i0 + k < plane) sum += (unsigned)jitter_gray(px[0][k], px[1][k], px[2][k]);
        }
    }
    const unsigned long long s = jitter_block_sum(sum);
    if (threadIdx.x == 0) partials[(size_t)img * gridDim.x + blockIdx.x] = (unsigned)s;
}

// launch two: the whole row, then the lighting (lighting f32 [n][3] or null): v <- (u8) rintf(clamp((float)v + off_c, 0, 255))
__global__ void __launch_bounds__(kJitterThreads) k_color_jitter_apply(const unsigned char* __restrict__ src,
                                                                       const float* __restrict__ table,
                                                                       const float* __restrict__ lighting,
                                                                       const unsigned* __restrict__ partials,
                                                                       unsigned char* __restrict__ dst, int plane, int vec4)
{
    const int img = blockIdx.y;
    const JitterRow row = load_jitter(table, img, partials != nullptr);
    int m = 0;
    if (row.contrast_at < 4) {  // the same for the whole workgroup; gridDim.x <= kJitterThreads partials an image
        const unsigned long long S = jitter_block_sum(threadIdx.x < gridDim.x ? partials[(size_t)img * gridDim.x + threadIdx.x] : 0u);
        m = (int)((2 * S + (unsigned long long)plane) / (2 * (unsigned long long)plane));
    }
    float off[3] = {0.0f, 0.0f, 0.0f};
    if (lighting != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) off[c] = lighting[3 * (size_t)img + c];
    }
    const unsigned char* __restrict__ base = src + (size_t)img * 3 * plane;
    unsigned char* __restrict__ out = dst + (size_t)img * 3 * plane;
    for (int i0 = (blockIdx.x * kJitterThreads + threadIdx.x) * 4; i0 < plane; i0 += gridDim.x * kJitterThreads * 4) {
        int px[3][4];
        jitter_load(base, plane, i0, vec4, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) jitter_ops(row, 0, 4, m, px[0][k], px[1][k], px[2][k]);
        if (lighting != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) px[c][k] = (int)rintf(fminf(fmaxf((float)px[c][k] + off[c], 0.0f), 255.0f));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned char* __restrict__ p = out + (size_t)c * plane + i0;
            if (vec4) {
                *reinterpret_cast<unsigned*>(p) = (unsigned)px[c][0] | ((unsigned)px[c][1] << 8) | ((unsigned)px[c][2] << 16) |
                                                  ((unsigned)px[c][3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (i0 + k < plane) p[k] = (unsigned char)px[c][k];
            }
        }
    }
}

// The mean over V views: x f32 [n][V][d] -> out f32 [n][d], out = (((x_0 + x_1) + ...) + x_{V-1}) / V in view order.  One
// thread per (b, j); the loads of a wave are contiguous in j.
__global__ void __launch_bounds__(256) k_view_mean(const float* __restrict__ x, float* __restrict__ out, int n, int n_views,
                                                   int d)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * d) return;
    const int b = (int)(i / d), j = (int)(i - (long long)b * d);
    const float* p = x + (size_t)b * n_views * d + j;
    float s = p[0];
    for (int v = 1; v < n_views; ++v) s += p[(size_t)v * d];
    out[i] = s / (float)n_views;
}

static constexpr int kMaxGridY = 65535;

// The checks every flow gather shares; -> VA_OK or the error va_last_error() then reports.
static int check_flow_gather(const char* who, const void* flow, const void* crops, const void* stack, long long planes,
                             int w, int h, int out_w, int out_h, float bound, float stdv)
{
    VA_CHECK_ARG(flow != nullptr && crops != nullptr && stack != nullptr, "%s: NULL buffer", who);
    VA_CHECK_ARG(w >= 1 && h >= 1, "%s: bad shape", who);
    VA_CHECK_ARG(planes <= kMaxGridY, "%s: %lld output planes exceed %d per call", who, planes, kMaxGridY);
    VA_CHECK_ARG(out_w >= 1 && out_h >= 1 && out_w <= w && out_h <= h, "%s: crop %dx%d does not fit the %dx%d frame", who,
                 out_w, out_h, w, h);
    VA_CHECK_ARG(bound > 0.0f && stdv > 0.0f, "%s: bound and std must be > 0", who);
    return VA_OK;
}

template <typename SRC>
static void launch_flow_gather(const SRC* flow, const int* crops, float* stack, int w, int h, int out_w, int out_h,
                               int chans, int planes, int n_views, int invert_x, float bound, float mean, float stdv,
                               hipStream_t stream, const int* starts = nullptr, int n_pairs = 0)
{
    const dim3 g((unsigned)va_cdiv(out_w * out_h, kGatherPerBlock), (unsigned)planes);
    // one aligned source run of 4 elements: 16 bytes of f32, 4 bytes of u8
    const int vec4 = ((out_w * out_h) % 4 == 0 && reinterpret_cast<uintptr_t>(stack) % 16 == 0 ? 1 : 0) |
                     (w % 4 == 0 && out_w % 4 == 0 && reinterpret_cast<uintptr_t>(flow) % (4 * sizeof(SRC)) == 0 ? 2 : 0);
    if (starts)
        k_flow_crop_stack<true, SRC><<<g, 256, 0, stream>>>(flow, crops, starts, n_pairs, stack, w, h, out_w, out_h, chans,
                                                            n_views, invert_x, vec4, bound, mean, stdv);
    else
        k_flow_crop_stack<false, SRC><<<g, 256, 0, stream>>>(flow, crops, nullptr, 0, stack, w, h, out_w, out_h, chans,
                                                             n_views, invert_x, vec4, bound, mean, stdv);
}

extern "C" int va_flow_to_stack_crop(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean,
                                     float stdv, const void* crops, int out_w, int out_h, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_to_stack_crop: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(n_pairs >= 1, "va_flow_to_stack_crop: bad shape");
    const int rc = check_flow_gather("va_flow_to_stack_crop", flow, crops, stack, 2LL * n_pairs, w, h, out_w, out_h, bound,
                                     stdv);
    if (rc != VA_OK) return rc;
    launch_flow_gather((const float*)flow, (const int*)crops, (float*)stack, w, h, out_w, out_h, 2 * n_pairs, 2 * n_pairs, 1,
                       0, bound, mean, stdv, (hipStream_t)stream);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_flow_to_stack_views(va_ctx* ctx, const void* flow, int n_clips, int flow_count, int n_views, int w, int h,
                                      float bound, float mean, float stdv, const void* crops, int invert_x_on_flip,
                                      int out_w, int out_h, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_to_stack_views: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(n_clips >= 1 && flow_count >= 1 && n_views >= 1, "va_flow_to_stack_views: bad shape");
    VA_CHECK_ARG(invert_x_on_flip == 0 || invert_x_on_flip == 1, "va_flow_to_stack_views: invert_x_on_flip must be 0 or 1");
    const long long planes = (long long)n_clips * n_views * 2 * flow_count;
    const int rc = check_flow_gather("va_flow_to_stack_views", flow, crops, stack, planes, w, h, out_w, out_h, bound, stdv);
    if (rc != VA_OK) return rc;
    launch_flow_gather((const float*)flow, (const int*)crops, (float*)stack, w, h, out_w, out_h, 2 * flow_count,
                       (int)planes, n_views, invert_x_on_flip, bound, mean, stdv, (hipStream_t)stream);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// va_flow_to_stack_snippets and its stored-flow form (S40): the checks and the launch
template <typename SRC>
static int flow_snippets(const char* who, va_ctx* ctx, const void* flow, int n_pairs, const void* starts, int n_snippets,
                         int flow_count, int n_views, int w, int h, float bound, float mean, float stdv, const void* crops,
                         int invert_x_on_flip, int out_w, int out_h, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(n_snippets >= 1 && flow_count >= 1 && n_views >= 1, "%s: bad shape", who);
    VA_CHECK_ARG(n_pairs >= flow_count && n_pairs <= 0x3fffffff, "%s: %d flow pairs do not hold a window of %d", who, n_pairs,
                 flow_count);
    VA_CHECK_ARG(starts != nullptr, "%s: NULL buffer", who);
    VA_CHECK_ARG(invert_x_on_flip == 0 || invert_x_on_flip == 1, "%s: invert_x_on_flip must be 0 or 1", who);
    const long long planes = (long long)n_snippets * n_views * 2 * flow_count;
    const int rc = check_flow_gather(who, flow, crops, stack, planes, w, h, out_w, out_h, bound, stdv);
    if (rc != VA_OK) return rc;
    launch_flow_gather((const SRC*)flow, (const int*)crops, (float*)stack, w, h, out_w, out_h, 2 * flow_count, (int)planes,
                       n_views, invert_x_on_flip, bound, mean, stdv, (hipStream_t)stream, (const int*)starts, n_pairs);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_flow_to_stack_snippets(va_ctx* ctx, const void* flow, int n_pairs, const void* starts, int n_snippets,
                                         int flow_count, int n_views, int w, int h, float bound, float mean, float stdv,
                                         const void* crops, int invert_x_on_flip, int out_w, int out_h, void* stack,
                                         void* stream)
{
    return flow_snippets<float>("va_flow_to_stack_snippets", ctx, flow, n_pairs, starts, n_snippets, flow_count, n_views, w, h,
                                bound, mean, stdv, crops, invert_x_on_flip, out_w, out_h, stack, stream);
}

extern "C" int va_flowq_to_stack_snippets(va_ctx* ctx, const void* flowq, int n_pairs, const void* starts, int n_snippets,
                                          int flow_count, int n_views, int w, int h, float mean, float stdv, const void* crops,
                                          int invert_x_on_flip, int out_w, int out_h, void* stack, void* stream)
{
    // (the images are quantised already: the bound the shared checks and the kernel take is not used)
    return flow_snippets<unsigned char>("va_flowq_to_stack_snippets", ctx, flowq, n_pairs, starts, n_snippets, flow_count,
                                        n_views, w, h, 1.0f, mean, stdv, crops, invert_x_on_flip, out_w, out_h, stack, stream);
}

extern "C" int va_flow_quantize_u8(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, void* out,
                                   void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_quantize_u8: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && out != nullptr, "va_flow_quantize_u8: NULL buffer");
    VA_CHECK_ARG(n_pairs >= 1 && w >= 1 && h >= 1, "va_flow_quantize_u8: bad shape");
    VA_CHECK_ARG(bound > 0.0f, "va_flow_quantize_u8: bound must be > 0");
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(flow) % 4 == 0, "va_flow_quantize_u8: flow must be 4-byte aligned");
    const size_t n = (size_t)2 * n_pairs * w * h;
    const size_t blocks = (n + kGatherPerBlock - 1) / kGatherPerBlock;
    VA_CHECK_ARG(blocks <= 0x7fffffffULL, "va_flow_quantize_u8: %d pairs of %dx%d exceed one launch", n_pairs, w, h);
    k_flow_quantize_u8<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const float*)flow, (unsigned char*)out, n,
                                                                         reinterpret_cast<uintptr_t>(flow) % 16 == 0,
                                                                         reinterpret_cast<uintptr_t>(out) % 4 == 0, bound);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// The checks and the launch every image gather shares (n_views = 1: va_crop_images_u8).
static int crop_images(const char* who, const void* src, int n, int c, int w, int h, int src_nhwc, int n_views,
                       const void* crops, int out_w, int out_h, void* dst, hipStream_t stream)
{
    VA_CHECK_ARG(src != nullptr && crops != nullptr && dst != nullptr, "%s: NULL buffer", who);
    VA_CHECK_ARG(n >= 1 && c >= 1 && w >= 1 && h >= 1 && n_views >= 1, "%s: bad shape", who);
    VA_CHECK_ARG(src_nhwc == 0 || src_nhwc == 1, "%s: src_nhwc must be 0 or 1", who);
    VA_CHECK_ARG((long long)n * n_views * c <= kMaxGridY, "%s: %d x %d x %d planes exceed %d per call", who, n, n_views, c,
                 kMaxGridY);
    VA_CHECK_ARG(out_w >= 1 && out_h >= 1 && out_w <= w && out_h <= h, "%s: crop %dx%d does not fit the %dx%d image", who,
                 out_w, out_h, w, h);
    const dim3 g((unsigned)va_cdiv(out_w * out_h, kGatherPerBlock), (unsigned)(n * n_views * c));
    const int vec4 = (out_w * out_h) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    if (src_nhwc)
        k_crop_images_u8<true><<<g, 256, 0, stream>>>((const unsigned char*)src, (const int*)crops, (unsigned char*)dst, c, w,
                                                      h, out_w, out_h, n_views, vec4);
    else
        k_crop_images_u8<false><<<g, 256, 0, stream>>>((const unsigned char*)src, (const int*)crops, (unsigned char*)dst, c,
                                                       w, h, out_w, out_h, n_views, vec4);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_crop_images_u8(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc, const void* crops,
                                 int out_w, int out_h, void* dst, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_crop_images_u8: ctx is NULL");
    VA_USE_DEVICE(ctx);
    return crop_images("va_crop_images_u8", src, n, c, w, h, src_nhwc, 1, crops, out_w, out_h, dst, (hipStream_t)stream);
}

extern "C" int va_crop_images_u8_views(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc, int n_views,
                                       const void* crops, int out_w, int out_h, void* dst, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_crop_images_u8_views: ctx is NULL");
    VA_USE_DEVICE(ctx);
    return crop_images("va_crop_images_u8_views", src, n, c, w, h, src_nhwc, n_views, crops, out_w, out_h, dst,
                       (hipStream_t)stream);
}

// va_flow_to_stack_resize and its stored-flow form (S41): the checks and the launch
template <typename SRC>
static int flow_resize(const char* who, va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean,
                       float stdv, const void* table, int n_out, int invert_x_on_flip, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && table != nullptr && stack != nullptr, "%s: NULL buffer", who);
    VA_CHECK_ARG(n_pairs >= 1 && n_pairs <= 0x3fffffff && w >= 1 && h >= 1 && n_out >= 1, "%s: bad shape", who);
    VA_CHECK_ARG(n_out <= kMaxGridY, "%s: %d output planes exceed %d per call", who, n_out, kMaxGridY);
    VA_CHECK_ARG(invert_x_on_flip == 0 || invert_x_on_flip == 1, "%s: invert_x_on_flip must be 0 or 1", who);
    VA_CHECK_ARG(bound > 0.0f && stdv > 0.0f, "%s: bound and std must be > 0", who);
    const int vec4 = reinterpret_cast<uintptr_t>(stack) % 16 == 0;
    k_flow_resize_stack<SRC><<<dim3(kResizeBlocks, (unsigned)n_out), kResizeThreads, 0, (hipStream_t)stream>>>(
        (const SRC*)flow, (const int*)table, (float*)stack, 2 * n_pairs, w, h, invert_x_on_flip, vec4, bound, mean, stdv);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_flow_to_stack_resize(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean,
                                       float stdv, const void* table, int n_out, int invert_x_on_flip, void* stack, void* stream)
{
    return flow_resize<float>("va_flow_to_stack_resize", ctx, flow, n_pairs, w, h, bound, mean, stdv, table, n_out,
                              invert_x_on_flip, stack, stream);
}

extern "C" int va_flowq_to_stack_resize(va_ctx* ctx, const void* flowq, int n_pairs, int w, int h, float mean, float stdv,
                                        const void* table, int n_out, int invert_x_on_flip, void* stack, void* stream)
{
    return flow_resize<unsigned char>("va_flowq_to_stack_resize", ctx, flowq, n_pairs, w, h, 1.0f, mean, stdv, table, n_out,
                                      invert_x_on_flip, stack, stream);
}

extern "C" int va_resize_images_u8(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc, const void* table,
                                   int n_out, void* dst, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_resize_images_u8: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(src != nullptr && table != nullptr && dst != nullptr, "va_resize_images_u8: NULL buffer");
    VA_CHECK_ARG(n >= 1 && c >= 1 && w >= 1 && h >= 1 && n_out >= 1, "va_resize_images_u8: bad shape");
    VA_CHECK_ARG(src_nhwc == 0 || src_nhwc == 1, "va_resize_images_u8: src_nhwc must be 0 or 1");
    VA_CHECK_ARG((long long)n_out * c <= kMaxGridY, "va_resize_images_u8: %d x %d planes exceed %d per call", n_out, c, kMaxGridY);
    const dim3 g(kResizeBlocks, (unsigned)(n_out * c));
    const int vec4 = reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    if (src_nhwc)
        k_resize_images_u8<true><<<g, kResizeThreads, 0, (hipStream_t)stream>>>((const unsigned char*)src, (const int*)table,
                                                                                (unsigned char*)dst, n, c, w, h, vec4);
    else
        k_resize_images_u8<false><<<g, kResizeThreads, 0, (hipStream_t)stream>>>((const unsigned char*)src, (const int*)table,
                                                                                 (unsigned char*)dst, n, c, w, h, vec4);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_rgbdiff_to_stack(va_ctx* ctx, const void* frames, int n_frames, int w, int h, int src_nhwc, int n_diff,
                                   const float* den, const void* table, int n_out, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_rgbdiff_to_stack: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(frames != nullptr && den != nullptr && table != nullptr && stack != nullptr, "va_rgbdiff_to_stack: NULL buffer");
    VA_CHECK_ARG(w >= 1 && h >= 1 && n_out >= 1 && 3LL * w * h <= 0x7fffffffLL, "va_rgbdiff_to_stack: bad shape");
    VA_CHECK_ARG(src_nhwc == 0 || src_nhwc == 1, "va_rgbdiff_to_stack: src_nhwc must be 0 or 1");
    VA_CHECK_ARG(n_diff >= 1 && 3 * (long long)n_diff <= 64, "va_rgbdiff_to_stack: n_diff must lie in 1..21 (3*n_diff <= 64 channels), got %d",
                 n_diff);
    VA_CHECK_ARG(n_frames > n_diff && n_frames <= 0x3fffffff, "va_rgbdiff_to_stack: %d frames do not hold a window of %d differences",
                 n_frames, n_diff);
    VA_CHECK_ARG(n_out <= kMaxGridY, "va_rgbdiff_to_stack: %d output items exceed %d per call", n_out, kMaxGridY);
    for (int c = 0; c < 3; ++c)
        VA_CHECK_ARG(den[c] > 0.0f && den[c] <= 3.0e38f, "va_rgbdiff_to_stack: den[%d] must be finite and > 0", c);
    const dim3 g(kResizeBlocks, (unsigned)n_out);
    const int vec4 = reinterpret_cast<uintptr_t>(stack) % 16 == 0;
    if (src_nhwc)
        k_rgbdiff_stack<true><<<g, kResizeThreads, 0, (hipStream_t)stream>>>((const unsigned char*)frames, (const int*)table,
                                                                             (float*)stack, n_frames, n_diff, w, h, vec4, den[0],
                                                                             den[1], den[2]);
    else
        k_rgbdiff_stack<false><<<g, kResizeThreads, 0, (hipStream_t)stream>>>((const unsigned char*)frames, (const int*)table,
                                                                              (float*)stack, n_frames, n_diff, w, h, vec4, den[0],
                                                                              den[1], den[2]);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_color_jitter_u8(va_ctx* ctx, const void* src, int n, int w, int h, const void* table, const void* lighting,
                                  void* dst, void* workspace, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_color_jitter_u8: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(src != nullptr && table != nullptr && dst != nullptr, "va_color_jitter_u8: NULL buffer");
    VA_CHECK_ARG(n >= 1 && w >= 1 && h >= 1 && (long long)w * h <= 0x3fffffffLL, "va_color_jitter_u8: bad shape");
    VA_CHECK_ARG(n <= kMaxGridY, "va_color_jitter_u8: %d images exceed %d per call", n, kMaxGridY);
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(table) % 4 == 0 && reinterpret_cast<uintptr_t>(lighting) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(workspace) % 4 == 0,
                 "va_color_jitter_u8: table, lighting and workspace must be 4-byte aligned");
    const size_t bytes = (size_t)n * 3 * w * h;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    VA_CHECK_ARG(s0 == d0 || s0 + bytes <= d0 || d0 + bytes <= s0, "va_color_jitter_u8: dst must equal src or not overlap it");
    const int plane = w * h;
    const dim3 g((unsigned)std::min(va_cdiv(plane, kJitterPerBlock), VA_COLOR_JITTER_PARTIALS), (unsigned)n);
    const int vec4 = plane % 4 == 0 && s0 % 4 == 0 && d0 % 4 == 0;
    if (workspace != nullptr)
        k_color_jitter_sums<<<g, kJitterThreads, 0, (hipStream_t)stream>>>((const unsigned char*)src, (const float*)table,
                                                                           (unsigned*)workspace, plane, vec4);
    k_color_jitter_apply<<<g, kJitterThreads, 0, (hipStream_t)stream>>>((const unsigned char*)src, (const float*)table,
                                                                        (const float*)lighting, (const unsigned*)workspace,
                                                                        (unsigned char*)dst, plane, vec4);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_view_mean(va_ctx* ctx, const void* x, int n, int n_views, int d, void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_view_mean: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x != nullptr && out != nullptr, "va_view_mean: NULL buffer");
    VA_CHECK_ARG(n >= 1 && n_views >= 1 && d >= 1, "va_view_mean: bad shape");
    const long long threads = (long long)n * d;
    VA_CHECK_ARG(threads <= 0x7fffffffLL, "va_view_mean: %d x %d outputs exceed one launch", n, d);
    k_view_mean<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>((const float*)x, (float*)out, n, n_views,
                                                                                  d);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
