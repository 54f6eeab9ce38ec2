// Crop and horizontal flip of full-frame inputs on the device: the RandomCrop(224) /
// RandomHorizontalFlip() steps of getTransforms() (Sheet03/utils.py:143,145) for frames of any size, so that 320x240
// clips reach the 224x224 networks without a trip through the host.  The crops are drawn on the host
// (video_analytics_amd/augment.py) and handed over as DEVICE int32 {top, left, flip} triples.
//
// Both kernels are pure gathers: thread i of a channel plane writes output element i (the writes of a wave are one
// contiguous run) and reads source row top + y, column left + x -- or left + out_w - 1 - x when flipped, the same
// contiguous source segment in reverse lane order.  A wave whose 64 elements straddle two output rows reads two such
// segments.  No LDS.
#include "va_internal.h"

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

// S10 then S9: flow f32 [n_pairs][2][h][w] -> stack f32 [2 n_pairs][out_h][out_w]; channel ch = 2k + plane reads plane
// `plane` of pair k through crop ch.  The quantisation and normalisation are k_flow_to_stack's expressions in its order;
// the flip mirrors the quantised image and leaves the sign of the x flow alone (the reference flips 8-bit images).
__global__ void __launch_bounds__(256) k_flow_crop_stack(const float* __restrict__ flow, const int* __restrict__ crops,
                                                         float* __restrict__ stack, int w, int h, int out_w, int out_h,
                                                         float bound, float mean, float stdv)
{
    const int ch = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= out_w * out_h) return;
    const CropWin c = load_crop(crops, ch, h, w, out_h, out_w);
    const int y = idx / out_w, x = idx - y * out_w;
    const int sx = c.left + (c.flip ? out_w - 1 - x : x);
    const float v = flow[(size_t)ch * h * w + (size_t)(c.top + y) * w + sx];  // plane ch of [n_pairs][2] is pair ch/2, plane ch%2
    const float t = (255.0f * (v + bound)) / (2.0f * bound);
    const float q = rintf(fminf(fmaxf(t, 0.0f), 255.0f));
    stack[(size_t)ch * out_h * out_w + idx] = (q / 255.0f - mean) / stdv;
}

// S10 on u8 images: src [n][c][h][w] (NHWC = false) or [n][h][w][c] (NHWC = true) -> dst [n][c][out_h][out_w]; one crop
// per image, shared by its channels.  Block row blockIdx.y = image * c + channel.
template <bool NHWC>
__global__ void __launch_bounds__(256) k_crop_images_u8(const unsigned char* __restrict__ src, const int* __restrict__ crops,
                                                        unsigned char* __restrict__ dst, int c, int w, int h, int out_w,
                                                        int out_h)
{
    const int img = blockIdx.y / c, chn = blockIdx.y - img * c;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= out_w * out_h) return;
    const CropWin cw = load_crop(crops, img, h, w, out_h, out_w);
    const int y = idx / out_w, x = idx - y * out_w;
    const int sy = cw.top + y, sx = cw.left + (cw.flip ? out_w - 1 - x : x);
    const size_t s = NHWC ? (((size_t)img * h + sy) * w + sx) * c + chn : (((size_t)img * c + chn) * h + sy) * w + sx;
    dst[(size_t)blockIdx.y * out_h * out_w + idx] = src[s];
}

static constexpr int kMaxGridY = 65535;

extern "C" int va_flow_to_stack_crop(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean,
                                     float stdv, const void* crops, int out_w, int out_h, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_to_stack_crop: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && crops != nullptr && stack != nullptr, "va_flow_to_stack_crop: NULL buffer");
    VA_CHECK_ARG(n_pairs >= 1 && w >= 1 && h >= 1, "va_flow_to_stack_crop: bad shape");
    VA_CHECK_ARG(2 * (long long)n_pairs <= kMaxGridY, "va_flow_to_stack_crop: %d pairs exceed %d channels per call", n_pairs,
                 kMaxGridY);
    VA_CHECK_ARG(out_w >= 1 && out_h >= 1 && out_w <= w && out_h <= h,
                 "va_flow_to_stack_crop: crop %dx%d does not fit the %dx%d frame", out_w, out_h, w, h);
    VA_CHECK_ARG(bound > 0.0f && stdv > 0.0f, "va_flow_to_stack_crop: bound and std must be > 0");
    const dim3 g((unsigned)va_cdiv(out_w * out_h, 256), (unsigned)(2 * n_pairs));
    k_flow_crop_stack<<<g, 256, 0, (hipStream_t)stream>>>((const float*)flow, (const int*)crops, (float*)stack, w, h, out_w,
                                                         out_h, bound, mean, stdv);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_crop_images_u8(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc, const void* crops,
                                 int out_w, int out_h, void* dst, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_crop_images_u8: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(src != nullptr && crops != nullptr && dst != nullptr, "va_crop_images_u8: NULL buffer");
    VA_CHECK_ARG(n >= 1 && c >= 1 && w >= 1 && h >= 1, "va_crop_images_u8: bad shape");
    VA_CHECK_ARG(src_nhwc == 0 || src_nhwc == 1, "va_crop_images_u8: src_nhwc must be 0 or 1");
    VA_CHECK_ARG((long long)n * c <= kMaxGridY, "va_crop_images_u8: %d x %d planes exceed %d per call", n, c, kMaxGridY);
    VA_CHECK_ARG(out_w >= 1 && out_h >= 1 && out_w <= w && out_h <= h,
                 "va_crop_images_u8: crop %dx%d does not fit the %dx%d image", out_w, out_h, w, h);
    const dim3 g((unsigned)va_cdiv(out_w * out_h, 256), (unsigned)(n * c));
    if (src_nhwc)
        k_crop_images_u8<true><<<g, 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (const int*)crops,
                                                                   (unsigned char*)dst, c, w, h, out_w, out_h);
    else
        k_crop_images_u8<false><<<g, 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (const int*)crops,
                                                                    (unsigned char*)dst, c, w, h, out_w, out_h);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
