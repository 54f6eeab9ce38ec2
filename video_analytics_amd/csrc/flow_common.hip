// What the three dense flow methods share (tvl1.hip, brox.hip, farneback.hip): the frames into level 0 (S0), the pyramid
// (S1), the centred gradient (S2), the level geometry, and the shape and buffer checks of a call.  Declarations: the "flow
// methods" section of va_internal.h.  DESIGN.md "TV-L1 specification" fixes every expression; like the methods' own files
// this one must be compiled with -ffp-contract=off.
//
// Layout (all fp32): rows `pitch` = width rounded up to 4 floats, planes rounded up to 64 floats,
//   pyramid  [level][frame][3 = I, Ix, Iy][plane]      built once per FRAME, shared by the two pairs that frame belongs to
#include "va_internal.h"
#include <cmath>

namespace {

constexpr int kMaxRadius = 8;

struct Taps {
    float g[2 * kMaxRadius + 1];
    int R;
};

// S0: gray values into plane 0 of every frame's level-0 block, as they are or (UNIT, S57) divided by 255
template <typename T, bool UNIT>
__global__ void k_frames(const T* __restrict__ frames, float* __restrict__ pyr0, int w, int h, int pitch, size_t plane)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= w * h) return;
    const int y = idx / w, x = idx - y * w;
    const float v = (float)frames[(size_t)f * w * h + idx];
    pyr0[(size_t)f * 3 * plane + (size_t)y * pitch + x] = UNIT ? v / 255.0f : v;
}

// S1: horizontal / vertical Gaussian; src and dst are [frame][stride_f floats] images of pitch `pitch`.
template <bool VERT>
__global__ void k_gauss(const float* __restrict__ src, size_t src_fstride, float* __restrict__ dst, size_t dst_fstride,
                        int w, int h, int pitch, Taps t)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= w * h) return;
    const int y = idx / w, x = idx - y * w;
    const float* s = src + (size_t)f * src_fstride;
    const int R = t.R;
    float acc;
    if (VERT) {
        acc = t.g[0] * s[d_max(y - R, 0) * pitch + x];
        for (int k = -R + 1; k <= R; ++k) acc = fmaf(t.g[k + R], s[d_min(d_max(y + k, 0), h - 1) * pitch + x], acc);
    } else {
        acc = t.g[0] * s[y * pitch + d_max(x - R, 0)];
        for (int k = -R + 1; k <= R; ++k) acc = fmaf(t.g[k + R], s[y * pitch + d_min(d_max(x + k, 0), w - 1)], acc);
    }
    dst[(size_t)f * dst_fstride + (size_t)y * pitch + x] = acc;
}

// S1: bilinear resample of the smoothed level s-1 into level s.
__global__ void k_resample(const float* __restrict__ src, size_t src_fstride, int w, int h, int pitch,
                           float* __restrict__ dst, size_t dst_fstride, int ow, int oh, int opitch)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ow * oh) return;
    const int y = idx / ow, x = idx - y * ow;
    const float fx = (float)w / (float)ow, fy = (float)h / (float)oh;
    dst[(size_t)f * dst_fstride + (size_t)y * opitch + x] =
        bilinear(src + (size_t)f * src_fstride, w, h, pitch, (float)x * fx, (float)y * fy);
}

// S2: centred gradient of every frame's level (planes 1,2 of the frame's [3][plane] block).
__global__ void k_grad(float* __restrict__ pyr, int w, int h, int pitch, size_t plane)
{
    const int f = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= w * h) return;
    const int y = idx / w, x = idx - y * w;
    float* base = pyr + (size_t)f * 3 * plane;
    const float* I = base;
    base[plane + (size_t)y * pitch + x] = 0.5f * (I[y * pitch + d_min(x + 1, w - 1)] - I[y * pitch + d_max(x - 1, 0)]);
    base[2 * plane + (size_t)y * pitch + x] = 0.5f * (I[d_min(y + 1, h - 1) * pitch + x] - I[d_max(y - 1, 0) * pitch + x]);
}

// Row pitch in floats: the width rounded up to 4 (rows start 16-byte aligned: k_iter_tile's 4-pixel runs)
int level_pitch(int w) { return (w + 3) / 4 * 4; }

int zoom_taps(float step, Taps* t)
{
    const float sigma = 0.6f * sqrtf(1.0f / (step * step) - 1.0f);
    int R = (int)(3.0f * sigma) + 1;
    if (R > kMaxRadius) R = kMaxRadius;
    double g[2 * kMaxRadius + 1], sum = 0.0;
    for (int k = -R; k <= R; ++k) {
        g[k + R] = std::exp(-(double)(k * k) / (2.0 * (double)sigma * (double)sigma));
        sum += g[k + R];
    }
    for (int k = 0; k <= 2 * R; ++k) t->g[k] = (float)(g[k] / sum);
    t->R = R;
    return R;
}

bool sides_ok(int w, int h) { return w >= 16 && h >= 16 && w <= 16384 && h <= 16384; }

}  // namespace

int va_flow_pyramid_sizes(int w, int h, float scale_step, int nscales, int* ws, int* hs)
{
    int n = 1;
    ws[0] = w;
    hs[0] = h;
    const int want = nscales > kVaMaxScales ? kVaMaxScales : nscales;
    while (n < want) {
        const int nw = (int)((float)ws[n - 1] * scale_step + 0.5f);
        const int nh = (int)((float)hs[n - 1] * scale_step + 0.5f);
        if ((nw < nh ? nw : nh) < 16) break;
        ws[n] = nw;
        hs[n] = nh;
        ++n;
    }
    return n;
}

void va_stage_layout(int w, int h, int* pitch, size_t* plane)
{
    *pitch = level_pitch(w);
    *plane = va_align_up((size_t)*pitch * h, 64);
}

void va_flow_levels_fill(va_flow_levels* L, int w, int h, int n_seq, int fps, float scale_step, int nscales)
{
    L->ns = va_flow_pyramid_sizes(w, h, scale_step, nscales, L->ws, L->hs);
    L->F = fps;
    L->NF = n_seq * fps;
    L->NP = n_seq * (fps - 1);
    // the buffers every level shares are sized for the LARGEST plane of the pyramid
    L->plane_max = 0;
    for (int s = 0; s < L->ns; ++s) {
        va_stage_layout(L->ws[s], L->hs[s], &L->pitch[s], &L->plane[s]);
        if (L->plane[s] > L->plane_max) L->plane_max = L->plane[s];
    }
}

int va_flow_check_shape(const char* who, int w, int h, int n_seq, int fps, bool frames)
{
    VA_CHECK_ARG(sides_ok(w, h), "%s: frame size %dx%d out of range [16,16384]", who, w, h);
    VA_CHECK_ARG(n_seq >= 1 && fps >= 2, "%s: need n_seq >= 1 and frames_per_seq >= 2 (got %d, %d)", who, n_seq, fps);
    VA_CHECK_ARG((long)n_seq * (frames ? fps : fps - 1) <= 65535, "%s: more than 65535 %s in one call", who, frames ? "frames" : "pairs");
    return VA_OK;
}

int va_flow_check_fields(const char* who, int n, int w, int h)
{
    VA_CHECK_ARG(n >= 1 && n <= 65535 && sides_ok(w, h), "%s: bad shape (n %d, %d x %d)", who, n, w, h);
    return VA_OK;
}

int va_flow_check_buffers(const char* who, const void* frames, const void* flow, const void* workspace, size_t have, size_t need)
{
    VA_CHECK_ARG(frames != nullptr && flow != nullptr && workspace != nullptr, "%s: NULL buffer", who);
    if (need == 0) return VA_OK;
    VA_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    if (have < need) {
        va_set_error("%s: workspace too small (%zu < %zu bytes)", who, have, need);
        return VA_ERR_WORKSPACE;
    }
    return VA_OK;
}

int va_stage_frames(const void* frames, int frames_are_u8, bool unit_range, float* pyr0, int w, int h, int pitch, size_t plane, int NF,
                    hipStream_t st)
{
    const dim3 g(va_cdiv(w * h, 256), NF);
    const unsigned char* u8 = (const unsigned char*)frames;
    const float* f32 = (const float*)frames;
    if (frames_are_u8 && unit_range) k_frames<unsigned char, true><<<g, 256, 0, st>>>(u8, pyr0, w, h, pitch, plane);
    else if (frames_are_u8) k_frames<unsigned char, false><<<g, 256, 0, st>>>(u8, pyr0, w, h, pitch, plane);
    else if (unit_range) k_frames<float, true><<<g, 256, 0, st>>>(f32, pyr0, w, h, pitch, plane);
    else k_frames<float, false><<<g, 256, 0, st>>>(f32, pyr0, w, h, pitch, plane);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// S1: levels 1 .. ns-1 of every frame from level 0 (plane 0 of pyr[0]); tmp1, tmp2: [NF][tmp_stride] scratch
int va_stage_pyramid(float* const* pyr, const int* ws, const int* hs, const int* pitch, const size_t* plane, int ns, int NF,
                     float* tmp1, float* tmp2, size_t tmp_stride, float step, hipStream_t st)
{
    const int TPB = 256;
    Taps taps;
    zoom_taps(step, &taps);
    for (int s = 1; s < ns; ++s) {
        const int pw = ws[s - 1], ph = hs[s - 1], pp = pitch[s - 1];
        const dim3 g(va_cdiv(pw * ph, TPB), NF);
        k_gauss<false><<<g, TPB, 0, st>>>(pyr[s - 1], 3 * plane[s - 1], tmp1, tmp_stride, pw, ph, pp, taps);
        k_gauss<true><<<g, TPB, 0, st>>>(tmp1, tmp_stride, tmp2, tmp_stride, pw, ph, pp, taps);
        const dim3 g2(va_cdiv(ws[s] * hs[s], TPB), NF);
        k_resample<<<g2, TPB, 0, st>>>(tmp2, tmp_stride, pw, ph, pp, pyr[s], 3 * plane[s], ws[s], hs[s], pitch[s]);
        VA_LAUNCH_CHECK();
    }
    return VA_OK;
}

// S2: planes 1, 2 of every frame's [3][plane] block <- the centred gradient of its plane 0
int va_stage_gradient(float* pyr, int w, int h, int pitch, size_t plane, int NF, hipStream_t st)
{
    k_grad<<<dim3(va_cdiv(w * h, 256), NF), 256, 0, st>>>(pyr, w, h, pitch, plane);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
