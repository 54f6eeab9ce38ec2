// Internal definitions shared by the translation units of libva_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <vector>
#include "../../include/va.h"

struct va_prof_span {
    hipEvent_t beg, end;
    int level;  // pyramid level the bracketed inner-iteration launches belong to
};
constexpr int kVaProfLevels = 16;

struct va_ctx {
    int device;
    int n_cu;
    // TV-L1 measurement hooks (va_tvl1_profile_*)
    bool prof_on;
    std::vector<va_prof_span> prof_spans;  // recorded, not yet read
    std::vector<va_prof_span> prof_pool;   // reusable events
    hipEvent_t prof_ref;                   // time origin for the union of spans (several streams)
    double prof_ms, prof_union_ms, prof_launches, prof_pxiters, prof_pxwarps;
    double prof_level_ms[kVaProfLevels], prof_level_pxiters[kVaProfLevels], prof_level_launches[kVaProfLevels];
};

void va_set_error(const char* fmt, ...);

#define VA_CHECK_ARG(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            va_set_error(__VA_ARGS__);   \
            return VA_ERR_INVALID;       \
        }                                \
    } while (0)

#define VA_HIP(call)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            va_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return VA_ERR_HIP;                                                           \
        }                                                                                \
    } while (0)

#define VA_LAUNCH_CHECK() VA_HIP(hipGetLastError())

// Every entry point runs on its context's device whatever the calling thread's current device is (launches,
// events and allocations follow hipSetDevice; the caller's stream and pointers must belong to that device), and hands
// the thread back with the device it came with: a process that holds several devices (torch) keeps its current device.
struct va_device_guard {
    int prev = -1, want = -1;
    hipError_t err = hipSuccess;
    explicit va_device_guard(int device) : want(device)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != want) err = hipSetDevice(want);
    }
    ~va_device_guard()
    {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
    va_device_guard(const va_device_guard&) = delete;
    va_device_guard& operator=(const va_device_guard&) = delete;
};
#define VA_USE_DEVICE(ctx_)                      \
    va_device_guard va_dev_guard_((ctx_)->device); \
    VA_HIP(va_dev_guard_.err)

// va_tvl1_params.tuning[]: the library's own switches (include/va.h keeps them anonymous)
enum {
    VA_TUNE_STREAM_LEVELS = 0,  // -1: the library decides per level; else bit s = pyramid level s iterates with the row pipeline
    VA_TUNE_STREAM_WAVES = 1,   // 0: default shape per level (four waves x 4 or 5 levels where they fit); 1: one-wave pipeline everywhere;
                                // 2: the two-wave form (2 x 8 levels); 7 / 8 / 9: four waves x 4 / 5 / 3 levels wherever they fit
    VA_TUNE_STREAM_CHUNKS = 2,  // 0: rows cut into as many chunks as fill the GPU; n > 0: n chunks (capped at h / 32)
    VA_TUNE_STREAM_SLOTS = 3,   // 0: default target number of strip x chunk x pair jobs per call
    VA_TUNE_ROWS_LEVELS = 4,    // reserved: -1 or 0 (0 with stream_levels = -1: register tiles on every level)
    VA_TUNE_STREAM_PPL = 5,     // 0 / 2: two pixels per lane
    VA_TUNE_STREAM_QUEUE = 6,   // reserved: 0 (2 is accepted: a launch per pass, which is what runs)
    VA_TUNE_ROWS_CFG = 7,       // reserved: 0
};
// va_brox_params.tuning[]: shapes of the inner-step kernel (brox.hip).  No value changes a result.
enum {
    VA_BROX_TUNE_WHOLE = 0,   // -1: a level whose field fits one workgroup runs there whole; 0: every level is tiled
    VA_BROX_TUNE_TILE_W = 1,  // 0: the largest tile the sweep depth allows; else the tile's width in pixels
    VA_BROX_TUNE_TILE_H = 2,  // likewise its height
    VA_BROX_TUNE_K = 3,       // 0: default; else the SOR sweeps of one tiled launch (halo 2K + 2), at most solver_iters
};                            // (slots 4..7: reserved, 0)
// va_farneback_params.tuning[]: tile shapes of the two kernels (farneback.hip).  No value changes a result.
enum {
    VA_FARNEBACK_TUNE_POLY_TILE_W = 0,  // 0: the library's tile; else the tile width of k_farneback_polyexp in pixels
    VA_FARNEBACK_TUNE_POLY_TILE_H = 1,  // likewise its height
    VA_FARNEBACK_TUNE_PASS_TILE_W = 2,  // 0: the library's tile; else the tile width of k_farneback_pass
    VA_FARNEBACK_TUNE_PASS_TILE_H = 3,  // likewise its height
};                                      // (slots 4..7: reserved, 0)
// va_dtraj_params.tuning[]: chunk length and tile shape (dtraj.hip).  No value changes a result.
enum {
    VA_DTRAJ_TUNE_CHUNK = 0,   // 0: the library's chunk; else the frames whose votes and integral planes are held at once
    VA_DTRAJ_TUNE_TILE_W = 1,  // 0: the library's tile; else the tile width of k_dtraj_votes in pixels
    VA_DTRAJ_TUNE_TILE_H = 2,  // likewise its height
};                             // (slots 3..7: reserved, 0)
// va_stip_params.tuning[]: tile shapes of the two smoothing kernels (stip.hip).  No value changes a result.
enum {
    VA_STIP_TUNE_ROW_TILE_W = 0,  // 0: the library's strip; else the outputs of one row a wave of k_stip_rows produces
    VA_STIP_TUNE_COL_TILE_W = 1,  // 0: the library's tile; else the columns of a tile of k_stip_cols, 1..64
    VA_STIP_TUNE_COL_TILE_N = 2,  // 0: as many outputs along the filtered axis as the LDS budget allows; else that number
};                                // (slots 3..7: reserved, 0)

// S12's bilinear sample of plane f (rows `pitch` floats apart) at (px, py): the position is clamped into the frame (a NaN
// lands on 0), the taps are the four neighbours (the last row / column repeats), and the interpolation is plain float32 (no
// fused multiply-add: the library builds with -ffp-contract=off).  S58 samples the second frame's derivatives with it.
__device__ __forceinline__ float va_bilinear_plain(const float* __restrict__ f, int w, int h, int pitch, float px, float py)
{
    const float xc = fminf(fmaxf(px, 0.0f), (float)(w - 1)), yc = fminf(fmaxf(py, 0.0f), (float)(h - 1));
    const int x0 = (int)floorf(xc), y0 = (int)floorf(yc);
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float ax = xc - (float)x0, ay = yc - (float)y0;
    const float* r0 = f + (size_t)y0 * pitch;
    const float* r1 = f + (size_t)y1 * pitch;
    const float a = r0[x0], b = r0[x1], c = r1[x0], d = r1[x1];
    const float top = a + ax * (b - a);
    const float bot = c + ax * (d - c);
    return top + ay * (bot - top);
}

static inline size_t va_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int va_cdiv(int a, int b) { return (a + b - 1) / b; }

// A workspace cut into parts that each start on a 256-byte boundary.  `base` may be NULL: the pointers are then the parts'
// offsets and `off` is the size the workspace needs.
struct va_carver {
    void* base;
    size_t off = 0;
    template <class T>
    T* take(size_t count)
    {
        T* p = (T*)((uintptr_t)base + off);
        off += va_align_up(count * sizeof(T), 256);
        return p;
    }
};

// S72: the integral planes [planes][h+1][w+1] of u32 [planes][h][w], sums mod 2^32 (dtraj.hip; stip.hip sums its votes with it)
int va_integral_planes(const unsigned* votes, unsigned* out, long long planes, int w, int h, hipStream_t st);

// ---- flow methods (tvl1.hip, brox.hip, farneback.hip): the front end they share, S0-S2 and the geometry (flow_common.hip)

constexpr int kVaMaxScales = 16;
constexpr int kVaMaxLds = 160 * 1024;  // what one workgroup of gfx950 can hold

__device__ __forceinline__ int d_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int d_max(int a, int b) { return a > b ? a : b; }

// State / per-warp-constant planes store every aligned run of four pixels as [x0, x0+2, x0+1, x0+3]: a thread of
// k_iter_tile then gets its four pixels as the register pairs E = (x0, x0+2), O = (x0+1, x0+3) straight from one
// 16-byte load, and two of its four x differences per row are a single packed subtract (O - E).
// (`perm` = 0: plain row order, the layout of the levels that k_iter_stream iterates.)
__device__ __forceinline__ int pslot(int x, int perm) { return perm ? ((x & ~3) | ((x & 1) << 1) | ((x >> 1) & 1)) : x; }

// S3 (perm: the image uses the interleaved state layout above)
__device__ __forceinline__ float bilinear(const float* __restrict__ img, int w, int h, int pitch, float x, float y, int perm = 0)
{
    x = fminf(fmaxf(x, 0.0f), (float)(w - 1));
    y = fminf(fmaxf(y, 0.0f), (float)(h - 1));
    const int x0 = (int)x, y0 = (int)y;
    const int x1 = d_min(x0 + 1, w - 1), y1 = d_min(y0 + 1, h - 1);
    const float ax = x - (float)x0, ay = y - (float)y0;
    const int s0 = pslot(x0, perm), s1 = pslot(x1, perm);
    const float a = img[y0 * pitch + s0], b = img[y0 * pitch + s1];
    const float c = img[y1 * pitch + s0], d = img[y1 * pitch + s1];
    const float top = fmaf(ax, b - a, a);
    const float bot = fmaf(ax, d - c, c);
    return fmaf(ay, bot - top, top);
}

// A kernel launched with more than 64 KB of dynamic LDS has to ask for it first
template <typename K>
int va_allow_lds(K* kernel, size_t lds)
{
    if (lds > 64 * 1024) VA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kVaMaxLds));
    return VA_OK;
}

// The levels of a call's pyramid (S1's sizes; rows `pitch` = width rounded up to 4 floats, planes rounded up to 64 floats)
// and its counts: F frames per sequence, NF frames, NP pairs.  Every method's plan starts with it.
struct va_flow_levels {
    int ns, ws[kVaMaxScales], hs[kVaMaxScales], pitch[kVaMaxScales];
    size_t plane[kVaMaxScales], plane_max;
    int F, NF, NP;
};
int va_flow_pyramid_sizes(int w, int h, float scale_step, int nscales, int* ws, int* hs);
void va_flow_levels_fill(va_flow_levels* L, int w, int h, int n_seq, int fps, float scale_step, int nscales);

// The shapes a call accepts (frames: the 65535 bound a grid's y extent sets holds the frames, not only the pairs), those of a
// stage's entry point (n fields of w x h), and the buffers of a call: none NULL and, once the plan is known (need > 0), the
// workspace 256-byte aligned and at least `need` bytes (VA_ERR_WORKSPACE otherwise).  `who` heads the message.
int va_flow_check_shape(const char* who, int w, int h, int n_seq, int fps, bool frames);
int va_flow_check_fields(const char* who, int n, int w, int h);
int va_flow_check_buffers(const char* who, const void* frames, const void* flow, const void* workspace, size_t have, size_t need);

// S0 (unit_range: gray values divided by 255), S1, S2 on the caller's buffers, frames [frame][3][plane]
void va_stage_layout(int w, int h, int* pitch, size_t* plane);
int va_stage_frames(const void* frames, int frames_are_u8, bool unit_range, float* pyr0, int w, int h, int pitch, size_t plane, int NF,
                    hipStream_t st);
int va_stage_pyramid(float* const* pyr, const int* ws, const int* hs, const int* pitch, const size_t* plane, int ns, int NF,
                     float* tmp1, float* tmp2, size_t tmp_stride, float step, hipStream_t st);
int va_stage_gradient(float* pyr, int w, int h, int pitch, size_t plane, int NF, hipStream_t st);
// S8 and the output copy for a state [pair][6][plane] in plain row order (tvl1.hip, beside the kernels of TV-L1's state layout)
int va_stage_upsample(const float* cstate, int cw, int ch, int cpitch, size_t cplane, float* tmp, float* fstate, int fw, int fh,
                      int fpitch, size_t fplane, float inv_step, int NP, hipStream_t st);
int va_stage_flow_out(const float* state, int w, int h, int pitch, size_t plane, float* flow, int NP, hipStream_t st);

// ---- baseline JPEG (jpeg.hip decodes, jpeg_encode.hip encodes): the block grid both speak about

constexpr long long kJpegMaxSamples = 0x7fffffffLL;  // MCU-padded samples of one image, all components (jpeg.MAX_SAMPLES)

// The block grid of one image.  A gray file is one component of 1x1 blocks per MCU; a colour file has hs x vs luma blocks and
// one block of each chroma component per MCU.  Blocks are kept per component in raster order: luma first, then Cb, then Cr.
struct jpeg_geom {
    int w, h, ncomp, hs, vs;
    int mw, mh;      // MCUs across and down
    int bwY, bhY;    // luma blocks across and down (MCU-padded)
    int bwC, bhC;    // chroma blocks across and down
    int nbY, nbC;    // blocks per luma / chroma component
    int blocks;      // blocks per image
    int plane_bytes; // the MCU-padded component planes of one image: Y, then Cb, then Cr
};

static inline bool jpeg_shape_ok(int n, int w, int h, int ncomp, int hs, int vs)
{
    if (n < 1 || w < 3 || h < 3 || w > 65535 || h > 65535) return false;
    if (ncomp == 1 ? !(hs == 1 && vs == 1) : !(ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))))
        return false;
    // the MCU-padded samples of one image (64 per block, all components) stay below 2^31: every count of jpeg_geom is an int
    const long long mw = (w + 8 * hs - 1) / (8 * hs), mh = (h + 8 * vs - 1) / (8 * vs);
    const long long blocks = mw * mh * (hs * vs + (ncomp == 3 ? 2 : 0));
    return blocks * 64 <= kJpegMaxSamples;
}

static inline jpeg_geom jpeg_make_geom(int w, int h, int ncomp, int hs, int vs)
{
    jpeg_geom g{};
    g.w = w, g.h = h, g.ncomp = ncomp, g.hs = hs, g.vs = vs;
    g.mw = va_cdiv(w, 8 * hs), g.mh = va_cdiv(h, 8 * vs);
    g.bwY = g.mw * hs, g.bhY = g.mh * vs;
    g.bwC = ncomp == 3 ? g.mw : 0, g.bhC = ncomp == 3 ? g.mh : 0;
    g.nbY = g.bwY * g.bhY, g.nbC = g.bwC * g.bhC;
    g.blocks = g.nbY + 2 * g.nbC;
    g.plane_bytes = g.blocks * 64;
    return g;
}

// workgroups of a launch of `threads` lanes; 0 when one launch cannot hold them
static inline long long jpeg_grid(long long lanes, int threads)
{
    const long long b = (lanes + threads - 1) / threads;
    return b <= 0x7fffffffLL ? b : 0;
}
