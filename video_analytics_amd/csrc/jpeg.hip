// Baseline JPEG decoding on the device: the frames of a Motion-JPEG AVI, the frame files and the flow
// images of both datasets, value for value what libjpeg's default decompressor (PIL) gives.  The host parses the headers and
// splits the entropy-coded bytes at the restart markers (video_analytics_amd/jpeg.py); three launches follow: Huffman decode
// with one lane per segment, dequantisation + the "islow" integer IDCT with one lane per 8x8 block, and for colour files the
// "fancy" chroma upsampling + the fixed-point YCbCr -> RGB.  Integer work only.
//
// The domain of "value for value" (DESIGN.md S47): every block whose dequantised coefficients are the quantised DCT of some
// 8x8 block of 8-bit samples -- what an encoder writes.  The 64 basis sign images at quality 100, 95 and 50 sit at its edge
// and are held to PIL (tests/test_jpeg_streams_*.py).  Outside it libjpeg's own builds disagree with each other (its SIMD
// IDCT against its C one; measured on the host, see S47), so there is nothing to equal: the device follows the C "islow"
// arithmetic with sums that wrap at 32 bits and a clamp to 0..255, which tests/test_jpeg_gpu.py holds to the host model.
#include "va_internal.h"

#include <cstdint>

namespace {

constexpr int kJpegLook = 9;              // bits of the look-ahead table: longer codes walk maxcode / valoff
constexpr int kJpegHuffBytes = 1424;      // one Huffman table: look u16[512], maxcode i32[18], valoff i32[18], vals u8[256]
constexpr int kJpegQuantBytes = 3 * 128;  // quant u16[3][64], natural order, one table per component
constexpr int kJpegSetBytes = kJpegQuantBytes + 6 * kJpegHuffBytes;  // quant, then (DC, AC) of component 0, 1, 2
constexpr int kJpegImgInts = 4;           // image table row: {table set, first segment, segments, 0}
constexpr int kJpegSegInts = 8;           // segment table row: {image, byte offset, bytes, first MCU, MCUs, 0, 0, 0}
constexpr int kJpegEntropyThreads = 64;
constexpr int kJpegThreads = 256;

enum { kJpegBadCode = 1, kJpegBadRun = 2, kJpegOutOfBits = 4, kJpegBadSegment = 8 };

// natural index of the k-th coefficient in zigzag order
__constant__ unsigned char kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

size_t jpeg_coef_bytes(int n, const jpeg_geom& g) { return va_align_up((size_t)n * g.blocks * 128, 256); }

// ---------------------------------------------------------------------------------------------- a. entropy decode

// MSB-first bit reader over the aligned words of one segment: the top n bits of acc are valid, `pending` is word `next`, loaded
// one refill ahead of its use so that a lane that decodes alone in its wave does not wait for every load.  Words behind the
// segment read as zero, so nothing outside it is ever loaded; used() then exceeds the segment's bits and the lane reports it.
struct jpeg_bits {
    const unsigned* __restrict__ src;
    int nwords, next, n;
    unsigned pending;
    unsigned long long acc;

    __device__ __forceinline__ void start(const unsigned* words, int count)
    {
        src = words, nwords = count, next = 0, n = 0, acc = 0;
        pending = count > 0 ? words[0] : 0u;
    }
    __device__ __forceinline__ void refill()  // afterwards at least 33 bits are valid: one code (<= 16) and its value (<= 16)
    {
        if (n <= 32) {
            const unsigned v = __builtin_bswap32(pending);
            ++next;
            pending = next < nwords ? src[next] : 0u;
            acc |= (unsigned long long)v << (32 - n);
            n += 32;
        }
    }
    __device__ __forceinline__ unsigned peek16() const { return (unsigned)(acc >> 48); }
    __device__ __forceinline__ void skip(int k) { acc <<= k, n -= k; }
    __device__ __forceinline__ int value(int s)  // s <= 16 bits through EXTEND
    {
        const int v = (int)((acc >> 32) >> (32 - s));
        skip(s);
        return s == 0 || v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
    }
    __device__ __forceinline__ long long used() const { return 32LL * next - n; }
};

// One Huffman symbol from the table at `tab`; -1 for a code the table does not hold.
__device__ __forceinline__ int jpeg_symbol(const unsigned char* tab, jpeg_bits& b)
{
    const unsigned short* look = reinterpret_cast<const unsigned short*>(tab);
    const int* maxcode = reinterpret_cast<const int*>(tab + 1024);
    const int* valoff = maxcode + 18;
    const unsigned char* vals = tab + 1024 + 144;
    const unsigned c16 = b.peek16();
    const unsigned e = look[c16 >> (16 - kJpegLook)];
    if (e != 0) {
        b.skip((int)(e >> 8) & 15);
        return (int)(e & 255);
    }
    // maxcode grows with the length (the host fills lengths without codes in), so the first length that holds the code is
    // the number of lengths that do not: seven independent loads, not a chain of them
    int len = kJpegLook + 1;
#pragma unroll
    for (int l = kJpegLook + 1; l <= 16; ++l) len += (int)(c16 >> (16 - l)) > maxcode[l] ? 1 : 0;
    if (len > 16) return -1;
    b.skip(len);
    return (int)vals[(valoff[len] + (int)(c16 >> (16 - len))) & 255];
}

// One lane per segment.  packed: the image table, the segment table, the table sets and the segment bytes (the offsets are the
// kernel's arguments); coef i16 [n][blocks][64], zero-filled, receives the nonzero coefficients in natural order.  A lane reads
// its own segment's words and writes the blocks of its own MCUs only; whatever goes wrong sets a bit of status[image].
template <bool SHARED>
__global__ void __launch_bounds__(kJpegEntropyThreads) k_jpeg_entropy(const unsigned char* __restrict__ packed, int off_seg, int off_tab,
                                                                      int off_data, long long data_bytes, int n, int nseg, int nsets,
                                                                      jpeg_geom g, short* __restrict__ coef, int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_tab[SHARED ? kJpegSetBytes : 16];
    __shared__ unsigned char s_zigzag[64];
    if (SHARED) {  // the whole call shares one table set
        const unsigned* src = reinterpret_cast<const unsigned*>(packed + off_tab);
        unsigned* dst = reinterpret_cast<unsigned*>(s_tab);
        for (int i = threadIdx.x; i < kJpegSetBytes / 4; i += kJpegEntropyThreads) dst[i] = src[i];
    }
    for (int i = threadIdx.x; i < 64; i += kJpegEntropyThreads) s_zigzag[i] = kJpegZigzag[i];
    __syncthreads();
    const int seg = blockIdx.x * kJpegEntropyThreads + threadIdx.x;
    if (seg >= nseg) return;
    const int* __restrict__ row = reinterpret_cast<const int*>(packed + off_seg) + (size_t)seg * kJpegSegInts;
    const int img = row[0], off = row[1], nbytes = row[2], first = row[3], count = row[4];
    if (img < 0 || img >= n) return;  // no image to report to
    const int set = reinterpret_cast<const int*>(packed)[(size_t)img * kJpegImgInts];
    const int nwords = (int)(((long long)nbytes + 3) / 4);
    if (set < 0 || set >= nsets || off < 0 || (off & 3) != 0 || nbytes < 0 || (long long)off + 4LL * nwords > data_bytes || first < 0 ||
        count < 0 || (long long)first + count > (long long)g.mw * g.mh) {
        atomicOr(&status[img], kJpegBadSegment);
        return;
    }
    const unsigned char* tabs = SHARED ? s_tab + kJpegQuantBytes : packed + off_tab + (size_t)set * kJpegSetBytes + kJpegQuantBytes;
    jpeg_bits b;
    b.start(reinterpret_cast<const unsigned*>(packed + off_data + off), nwords);
    const int hv = g.hs * g.vs, nb = g.ncomp == 3 ? hv + 2 : 1;
    short* __restrict__ blocks = coef + (size_t)img * g.blocks * 64;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int err = 0;
    for (int m = first; m < first + count && err == 0; ++m) {
        const int my = m / g.mw, mx = m - my * g.mw;
        for (int k = 0; k < nb && err == 0; ++k) {
            int ci, bx, by;
            if (k < hv) {
                const int v = k / g.hs;
                ci = 0, by = my * g.vs + v, bx = mx * g.hs + (k - v * g.hs);
            } else {
                ci = k - hv + 1, by = my, bx = mx;
            }
            const int at = ci == 0 ? by * g.bwY + bx : g.nbY + (ci - 1) * g.nbC + by * g.bwC + bx;
            short* __restrict__ dst = blocks + (size_t)at * 64;
            const unsigned char* dc = tabs + (size_t)(2 * ci) * kJpegHuffBytes;
            const unsigned char* ac = dc + kJpegHuffBytes;
            b.refill();
            const int t = jpeg_symbol(dc, b);
            if (t < 0) {
                err = kJpegBadCode;
                break;
            }
            const int diff = b.value(t & 15);
            int p = ci == 0 ? pred0 : ci == 1 ? pred1 : pred2;
            p += diff;
            pred0 = ci == 0 ? p : pred0, pred1 = ci == 1 ? p : pred1, pred2 = ci == 2 ? p : pred2;
            if (p != 0) dst[0] = (short)p;
            int i = 1;
            while (i < 64) {
                b.refill();
                const int rs = jpeg_symbol(ac, b);
                if (rs < 0) {
                    err = kJpegBadCode;
                    break;
                }
                const int r = rs >> 4, s = rs & 15;
                if (s == 0) {
                    if (r != 15) break;  // EOB
                    i += 16;             // ZRL
                    continue;
                }
                i += r;
                if (i > 63) {
                    err = kJpegBadRun;
                    break;
                }
                dst[s_zigzag[i]] = (short)b.value(s);
                ++i;
            }
            if (err == 0 && b.used() > 8LL * nbytes) err = kJpegOutOfBits;
        }
    }
    if (err != 0) atomicOr(&status[img], err);
}

// ---------------------------------------------------------------------------------------------- b. dequantise + IDCT

// One 8-point pass of jidctint's "islow" IDCT; 32-bit arithmetic that wraps (unsigned), the descale an arithmetic shift.
__device__ __forceinline__ void jpeg_idct8(const int (&a)[8], int (&o)[8], int sh)
{
    typedef unsigned u;
    const u c0 = (u)a[0], c2 = (u)a[2], c4 = (u)a[4], c6 = (u)a[6];
    u z1 = (c2 + c6) * 4433u;
    const u t2 = z1 - c6 * 15137u, t3 = z1 + c2 * 6270u;
    const u t0 = (c0 + c4) << 13, t1 = (c0 - c4) << 13;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u o0 = (u)a[7], o1 = (u)a[5], o2 = (u)a[3], o3 = (u)a[1];
    z1 = o0 + o3;
    u z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const u z5 = (z3 + z4) * 9633u;
    o0 *= 2446u, o1 *= 16819u, o2 *= 25172u, o3 *= 12299u;
    z1 *= (u)-7373, z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5, z4 = z4 * (u)-3196 + z5;
    o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
    const u r = 1u << (sh - 1);
    o[0] = (int)(t10 + o3 + r) >> sh, o[7] = (int)(t10 - o3 + r) >> sh;
    o[1] = (int)(t11 + o2 + r) >> sh, o[6] = (int)(t11 - o2 + r) >> sh;
    o[2] = (int)(t12 + o1 + r) >> sh, o[5] = (int)(t12 - o1 + r) >> sh;
    o[3] = (int)(t13 + o0 + r) >> sh, o[4] = (int)(t13 - o0 + r) >> sh;
}

// One lane per block: coef i16 [n][blocks][64] times the component's quantisation table through both passes into u8.  Colour
// files: the MCU-padded component planes, planes u8 [n][plane_bytes].  Gray files: the cropped image itself, out u8 [n][h][w].
// img_table may be null (every image uses table set 0).
__global__ void __launch_bounds__(kJpegThreads) k_jpeg_idct(const short* __restrict__ coef, const int* __restrict__ img_table,
                                                            const unsigned char* __restrict__ sets, int nsets, int n, jpeg_geom g,
                                                            unsigned char* __restrict__ dst)
{
    const long long gid = (long long)blockIdx.x * kJpegThreads + threadIdx.x;
    if (gid >= (long long)n * g.blocks) return;
    const int img = (int)(gid / g.blocks), blk = (int)(gid - (long long)img * g.blocks);
    int ci = 0, li = blk;
    if (blk >= g.nbY) ci = 1 + (blk - g.nbY) / g.nbC, li = blk - g.nbY - (ci - 1) * g.nbC;
    const int bw = ci == 0 ? g.bwY : g.bwC;
    const int by = li / bw, bx = li - by * bw;
    int set = img_table != nullptr ? img_table[(size_t)img * kJpegImgInts] : 0;
    set = min(max(set, 0), nsets - 1);
    const uint4* __restrict__ cp = reinterpret_cast<const uint4*>(coef + (size_t)gid * 64);
    const uint4* __restrict__ qp = reinterpret_cast<const uint4*>(sets + (size_t)set * kJpegSetBytes + (size_t)ci * 128);
    int c[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 cv = cp[r], qv = qp[r];
        const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[8 * r + 2 * j] = (int)(short)(cw[j] & 0xffffu) * (int)(qw[j] & 0xffffu);
            c[8 * r + 2 * j + 1] = (int)(short)(cw[j] >> 16) * (int)(qw[j] >> 16);
        }
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int a[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = c[8 * k + x];
        jpeg_idct8(a, o, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) c[8 * k + x] = o[k];
    }
    int stride, limw, limh;
    unsigned char* __restrict__ base;
    if (g.ncomp == 1) {
        stride = g.w, limw = g.w, limh = g.h;
        base = dst + (size_t)img * g.w * g.h;
    } else {
        stride = bw * 8, limw = bw * 8, limh = (ci == 0 ? g.bhY : g.bhC) * 8;
        base = dst + (size_t)img * g.plane_bytes + (ci == 0 ? 0 : (size_t)g.nbY * 64 + (size_t)(ci - 1) * g.nbC * 64);
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int a[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = c[8 * y + k];
        jpeg_idct8(a, o, 18);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = min(max(o[k] + 128, 0), 255);
        const int yy = by * 8 + y, x0 = bx * 8;
        if (yy >= limh) continue;
        unsigned char* __restrict__ p = base + (size_t)yy * stride + x0;
        const unsigned lo = (unsigned)o[0] | ((unsigned)o[1] << 8) | ((unsigned)o[2] << 16) | ((unsigned)o[3] << 24);
        const unsigned hi = (unsigned)o[4] | ((unsigned)o[5] << 8) | ((unsigned)o[6] << 16) | ((unsigned)o[7] << 24);
        const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
        if (x0 + 8 <= limw && (ad & 7) == 0) {
            *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
        } else if (x0 + 8 <= limw && (ad & 3) == 0) {
            reinterpret_cast<unsigned*>(p)[0] = lo;
            reinterpret_cast<unsigned*>(p)[1] = hi;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (x0 + k < limw) p[k] = (unsigned char)o[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------- c. upsample + colour

__device__ __forceinline__ int jpeg_clip8(int v) { return min(max(v, 0), 255); }

// libjpeg's "fancy" upsampling of one chroma plane at output pixel (x, y).  s: the plane, `stride` bytes per row, of which
// cw x ch samples are real; neighbours are clamped to the real samples, which is what libjpeg's edge cases amount to.
__device__ __forceinline__ int jpeg_chroma(const unsigned char* __restrict__ s, int stride, int cw, int ch, int hs, int vs, int x, int y)
{
    if (hs == 1) return (int)s[(size_t)y * stride + x];
    const int i = x >> 1, j = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (vs == 1) {  // h2v1
        const unsigned char* __restrict__ r = s + (size_t)y * stride;
        return (3 * (int)r[i] + (int)r[j] + 1 + (x & 1)) >> 2;
    }
    const int yc = y >> 1, yn = (y & 1) ? min(yc + 1, ch - 1) : max(yc - 1, 0);  // h2v2
    const unsigned char* __restrict__ r0 = s + (size_t)yc * stride;
    const unsigned char* __restrict__ r1 = s + (size_t)yn * stride;
    const int vi = 3 * (int)r0[i] + (int)r1[i], vj = 3 * (int)r0[j] + (int)r1[j];
    return (3 * vi + vj + 8 - (x & 1)) >> 4;
}

// planes u8 [n][plane_bytes] (Y, Cb, Cr, MCU-padded) -> out u8 [n][3][h][w].  A thread makes four adjacent pixels of one row
// in all three channels; the groups are laid out so that the R row leaves as whole dwords wherever it is aligned.
__global__ void __launch_bounds__(kJpegThreads) k_jpeg_color(const unsigned char* __restrict__ planes, int n, jpeg_geom g, int groups,
                                                             unsigned char* __restrict__ out)
{
    const long long idx = (long long)blockIdx.x * kJpegThreads + threadIdx.x;
    const long long rows = (long long)n * g.h;
    if (idx >= rows * groups) return;
    const long long r = idx / groups;
    const int gr = (int)(idx - r * groups);
    const int img = (int)(r / g.h), y = (int)(r - (long long)img * g.h);
    const unsigned char* __restrict__ Y = planes + (size_t)img * g.plane_bytes;
    const unsigned char* __restrict__ Cb = Y + (size_t)g.nbY * 64;
    const unsigned char* __restrict__ Cr = Cb + (size_t)g.nbC * 64;
    const int sy = g.bwY * 8, sc = g.bwC * 8;
    const int cw = (g.w + g.hs - 1) / g.hs, ch = (g.h + g.vs - 1) / g.vs;
    const size_t plane = (size_t)g.w * g.h;
    unsigned char* __restrict__ R = out + (size_t)img * 3 * plane + (size_t)y * g.w;
    const int x0 = 4 * gr - (int)(reinterpret_cast<uintptr_t>(R) & 3);
    int px[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(max(x0 + k, 0), g.w - 1);  // pixels outside the row repeat its nearest one and are not stored
        const int yv = (int)Y[(size_t)y * sy + x];
        const int cb = jpeg_chroma(Cb, sc, cw, ch, g.hs, g.vs, x, y) - 128;
        const int cr = jpeg_chroma(Cr, sc, cw, ch, g.hs, g.vs, x, y) - 128;
        px[0][k] = jpeg_clip8(yv + ((91881 * cr + 32768) >> 16));
        px[1][k] = jpeg_clip8(yv + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        px[2][k] = jpeg_clip8(yv + ((116130 * cb + 32768) >> 16));
    }
    const int first = max(0, -x0), last = min(4, g.w - x0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned char* __restrict__ p = R + (size_t)c * plane + x0;
        if (first == 0 && last == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            *reinterpret_cast<unsigned*>(p) =
                (unsigned)px[c][0] | ((unsigned)px[c][1] << 8) | ((unsigned)px[c][2] << 16) | ((unsigned)px[c][3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k >= first && k < last) p[k] = (unsigned char)px[c][k];
        }
    }
}

int jpeg_launch_idct(const short* coef, const int* img_table, const unsigned char* sets, int nsets, int n, const jpeg_geom& g,
                     unsigned char* dst, hipStream_t st)
{
    const long long blocks = jpeg_grid((long long)n * g.blocks, kJpegThreads);
    VA_CHECK_ARG(blocks > 0, "va_jpeg: %d images of %dx%d exceed one launch", n, g.w, g.h);
    k_jpeg_idct<<<(unsigned)blocks, kJpegThreads, 0, st>>>(coef, img_table, sets, nsets, n, g, dst);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int jpeg_launch_color(const unsigned char* planes, int n, const jpeg_geom& g, unsigned char* out, hipStream_t st)
{
    const int groups = (g.w + 6) / 4;
    const long long blocks = jpeg_grid((long long)n * g.h * groups, kJpegThreads);
    VA_CHECK_ARG(blocks > 0, "va_jpeg: %d images of %dx%d exceed one launch", n, g.w, g.h);
    k_jpeg_color<<<(unsigned)blocks, kJpegThreads, 0, st>>>(planes, n, g, groups, out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

}  // namespace

extern "C" size_t va_jpeg_decode_workspace_bytes(int n, int w, int h, int ncomp, int hs, int vs)
{
    if (!jpeg_shape_ok(n, w, h, ncomp, hs, vs)) return 0;
    const jpeg_geom g = jpeg_make_geom(w, h, ncomp, hs, vs);
    return jpeg_coef_bytes(n, g) + (ncomp == 3 ? (size_t)n * g.plane_bytes : 0);
}

extern "C" int va_jpeg_decode(va_ctx* ctx, const void* packed, size_t packed_bytes, int n, int w, int h, int ncomp, int hs, int vs,
                              int n_segments, int n_sets, void* out, void* status, void* workspace, size_t workspace_bytes,
                              void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_jpeg_decode: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(jpeg_shape_ok(n, w, h, ncomp, hs, vs),
                 "va_jpeg_decode: bad shape (%d images of %dx%d, %d components, luma sampling %dx%d)", n, w, h, ncomp, hs, vs);
    VA_CHECK_ARG(n_segments >= 1 && n_sets >= 1 && n_sets <= n, "va_jpeg_decode: %d segments and %d table sets for %d images",
                 n_segments, n_sets, n);
    VA_CHECK_ARG(packed != nullptr && out != nullptr && status != nullptr, "va_jpeg_decode: NULL buffer");
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(packed) % 16 == 0 && reinterpret_cast<uintptr_t>(status) % 4 == 0,
                 "va_jpeg_decode: packed must be 16-byte and status 4-byte aligned");
    const size_t off_seg = va_align_up((size_t)n * kJpegImgInts * 4, 16);
    const size_t off_tab = off_seg + (size_t)n_segments * kJpegSegInts * 4;
    const size_t off_data = off_tab + (size_t)n_sets * kJpegSetBytes;
    VA_CHECK_ARG(packed_bytes >= off_data && packed_bytes <= 0x7fffffffULL,
                 "va_jpeg_decode: the packed buffer holds %zu bytes, the tables alone need %zu (and 2^31 is the limit)", packed_bytes,
                 off_data);
    const jpeg_geom g = jpeg_make_geom(w, h, ncomp, hs, vs);
    const size_t coef_bytes = jpeg_coef_bytes(n, g), need = va_jpeg_decode_workspace_bytes(n, w, h, ncomp, hs, vs);
    if (workspace == nullptr || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        va_set_error("va_jpeg_decode: the workspace holds %zu bytes, %zu are needed (16-byte aligned)",
                     workspace == nullptr ? (size_t)0 : workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    const long long e_blocks = jpeg_grid(n_segments, kJpegEntropyThreads);
    VA_CHECK_ARG(e_blocks > 0, "va_jpeg_decode: %d segments exceed one launch", n_segments);

    const hipStream_t st = (hipStream_t)stream;
    const unsigned char* pk = (const unsigned char*)packed;
    short* coef = (short*)workspace;
    unsigned char* planes = (unsigned char*)workspace + coef_bytes;
    VA_HIP(hipMemsetAsync(coef, 0, coef_bytes, st));
    VA_HIP(hipMemsetAsync(status, 0, (size_t)n * 4, st));
    const long long data_bytes = (long long)(packed_bytes - off_data);
    if (n_sets == 1)
        k_jpeg_entropy<true><<<(unsigned)e_blocks, kJpegEntropyThreads, 0, st>>>(pk, (int)off_seg, (int)off_tab, (int)off_data, data_bytes,
                                                                                 n, n_segments, n_sets, g, coef, (int*)status);
    else
        k_jpeg_entropy<false><<<(unsigned)e_blocks, kJpegEntropyThreads, 0, st>>>(pk, (int)off_seg, (int)off_tab, (int)off_data, data_bytes,
                                                                                  n, n_segments, n_sets, g, coef, (int*)status);
    VA_LAUNCH_CHECK();
    const int rc = jpeg_launch_idct(coef, (const int*)pk, pk + off_tab, n_sets, n, g, ncomp == 3 ? planes : (unsigned char*)out, st);
    if (rc != VA_OK) return rc;
    return ncomp == 3 ? jpeg_launch_color(planes, n, g, (unsigned char*)out, st) : VA_OK;
}

extern "C" int va_jpeg_idct(va_ctx* ctx, const void* coef, const void* quant, int n, int w, int h, int ncomp, int hs, int vs, void* dst,
                            void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_jpeg_idct: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(jpeg_shape_ok(n, w, h, ncomp, hs, vs), "va_jpeg_idct: bad shape");
    VA_CHECK_ARG(coef != nullptr && quant != nullptr && dst != nullptr, "va_jpeg_idct: NULL buffer");
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(coef) % 16 == 0 && reinterpret_cast<uintptr_t>(quant) % 16 == 0,
                 "va_jpeg_idct: coef and quant must be 16-byte aligned");
    const jpeg_geom g = jpeg_make_geom(w, h, ncomp, hs, vs);
    return jpeg_launch_idct((const short*)coef, nullptr, (const unsigned char*)quant, 1, n, g, (unsigned char*)dst, (hipStream_t)stream);
}

extern "C" int va_jpeg_upsample(va_ctx* ctx, const void* planes, int n, int w, int h, int hs, int vs, void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_jpeg_upsample: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(jpeg_shape_ok(n, w, h, 3, hs, vs), "va_jpeg_upsample: bad shape");
    VA_CHECK_ARG(planes != nullptr && out != nullptr, "va_jpeg_upsample: NULL buffer");
    const jpeg_geom g = jpeg_make_geom(w, h, 3, hs, vs);
    return jpeg_launch_color((const unsigned char*)planes, n, g, (unsigned char*)out, (hipStream_t)stream);
}
