// Baseline JPEG encoding on the device: frame files and flow images, byte for byte the scan libjpeg's
// default compressor (PIL's Image.save) writes.  The host writes the headers around it (video_analytics_amd/jpeg.py).  Integer
// work only, in two stages:
//   a. k_jpeg_fdct, one lane per 8x8 block of the MCU-padded grid: colour conversion, edge padding, downsampling, the "islow"
//      forward DCT and the quantisation, into the decoder's coefficient array (i16 [n][blocks][64], natural order).
//   b. entropy coding, one workgroup per image and no workgroup ever waiting for another:
//      k_jpeg_entropy_encode  every lane takes one block in scan order, counts its bits, a workgroup scan gives it its bit
//                             position (every restart interval starts on a whole byte), and it writes its codes there into a
//                             zero-filled, un-stuffed buffer: whole words with plain stores, shared ones with atomic OR;
//      k_jpeg_stuff<false>    counts the FF bytes and the markers of the image: its final length;
//      k_jpeg_stuff<true>     places every byte behind the images before it: FF -> FF 00, RSTm in front of every interval but
//                             the first.
// The bytes depend on no launch shape and no timing: positions come from sums, and OR-ing disjoint bits has no order.
#include "va_internal.h"

#include <cstdint>

namespace {

constexpr int kEncThreads = 256;
constexpr int kEncQuantBytes = 3 * 128;           // quant u16[3][64], natural order, one table per component
constexpr int kEncHuffInts = 2 * (16 + 256);      // (DC u32[16], AC u32[256]) of luma, then of chroma: length << 16 | code
constexpr int kEncBlockBits = 20 + 63 * 26;       // the most one block codes to (jpeg.BLOCK_BITS)
constexpr int kEncRow = 33;                       // dwords of one block in LDS: 32 and one of padding against bank conflicts

enum { kEncRange = 1, kEncFit = 2 };

__constant__ unsigned char kEncZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------- a. samples -> coefficients

// One 8-point pass of jfdctint's "islow" forward DCT.  FIRST: the row pass, its output scaled up by PASS1_BITS = 2.
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(const int (&d)[8], int (&o)[8])
{
    constexpr int sh = FIRST ? 11 : 15, r = 1 << (sh - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    o[0] = FIRST ? (t10 + t11) << 2 : (t10 + t11 + 2) >> 2;
    o[4] = FIRST ? (t10 - t11) << 2 : (t10 - t11 + 2) >> 2;
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + r) >> sh;
    o[6] = (z1 - t12 * 15137 + r) >> sh;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    o[7] = (a4 + z1 + z3 + r) >> sh;
    o[5] = (a5 + z2 + z4 + r) >> sh;
    o[3] = (a6 + z2 + z3 + r) >> sh;
    o[1] = (a7 + z1 + z4 + r) >> sh;
}

// jccolor.c's 16-bit fixed point; which: 0 Y, 1 Cb, 2 Cr
__device__ __forceinline__ int jpeg_ycc(int which, int r, int g, int b)
{
    if (which == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (which == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// One lane per block of the MCU-padded grid.  images u8 [n][h][w] (NCOMP = 1) or [n][3][h][w]; coef i16 [n][blocks][64].
// Edges: columns repeat the last full-resolution column, rows the last full-resolution row up to a multiple of VS and from
// there the last downsampled row, so every read is a clamped one.  A dummy block (outside its component's real blocks) takes
// the block before it in the MCU's own order, which may be a dummy too, down to a real one, and keeps its DC alone.
template <int NCOMP, int HS, int VS>
__global__ void __launch_bounds__(kEncThreads) k_jpeg_fdct(const unsigned char* __restrict__ images, const unsigned char* __restrict__ tables,
                                                           int n, jpeg_geom g, short* __restrict__ coef)
{
    const long long gid = (long long)blockIdx.x * kEncThreads + threadIdx.x;
    if (gid >= (long long)n * g.blocks) return;
    const int img = (int)(gid / g.blocks), blk = (int)(gid - (long long)img * g.blocks);
    int ci = 0, li = blk;
    if (NCOMP == 3 && blk >= g.nbY) ci = 1 + (blk - g.nbY) / g.nbC, li = blk - g.nbY - (ci - 1) * g.nbC;
    const int bw = ci == 0 ? g.bwY : g.bwC;
    int by = li / bw, bx = li - by * bw;
    bool dummy = false;
    if (NCOMP == 3 && ci == 0 && HS * VS > 1) {
        const int wb = (g.w + 7) / 8, hb = (g.h + 7) / 8;
        const int mx = bx / HS, my = by / VS;
        int k = (by - my * VS) * HS + (bx - mx * HS);
        while (bx >= wb || by >= hb) {  // block 0 of every MCU is a real one
            dummy = true;
            --k;
            bx = mx * HS + k % HS, by = my * VS + k / HS;
        }
    }
    const size_t plane = (size_t)g.w * g.h;
    const unsigned char* __restrict__ src = images + (size_t)img * NCOMP * plane;
    const bool sub = NCOMP == 3 && ci > 0 && HS == 2;  // a downsampled component
    const int ch = (g.h + VS - 1) / VS;                // its real rows
    int c[64];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int d[8], o[8];
        const int yy = by * 8 + y;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int xx = bx * 8 + x;
            int v;
            if (NCOMP == 1) {
                v = (int)src[(size_t)min(yy, g.h - 1) * g.w + min(xx, g.w - 1)];
            } else if (!sub) {
                const size_t at = (size_t)min(yy, g.h - 1) * g.w + min(xx, g.w - 1);
                v = jpeg_ycc(ci, (int)src[at], (int)src[at + plane], (int)src[at + 2 * plane]);
            } else {
                const int yc = min(yy, ch - 1);
                v = VS == 2 ? 1 + (x & 1) : (x & 1);  // the bias alternates along the output row, from 1 (h2v2) or 0 (h2v1)
#pragma unroll
                for (int dy = 0; dy < VS; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const size_t at = (size_t)min(yc * VS + dy, g.h - 1) * g.w + min(xx * 2 + dx, g.w - 1);
                        v += jpeg_ycc(ci, (int)src[at], (int)src[at + plane], (int)src[at + 2 * plane]);
                    }
                v >>= VS;  // four samples (h2v2): >> 2; two (h2v1): >> 1
            }
            d[x] = v - 128;
        }
        jpeg_fdct8<true>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) c[8 * y + k] = o[k];
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int a[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = c[8 * k + x];
        jpeg_fdct8<false>(a, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) c[8 * k + x] = o[k];
    }
    const uint4* __restrict__ qp = reinterpret_cast<const uint4*>(tables + (size_t)ci * 128);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(coef + (size_t)gid * 64);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 qv = qp[r];
        const unsigned qw[4] = {qv.x, qv.y, qv.z, qv.w};
        unsigned out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned pair = 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const unsigned q = max((qw[j] >> (16 * e)) & 0xffffu, 1u);
                const int v = c[8 * r + 2 * j + e];
                const unsigned mag = ((unsigned)abs(v) + 4u * q) / (8u * q);  // half away from zero
                int s = v < 0 ? -(int)mag : (int)mag;
                if (dummy && (r | j | e) != 0) s = 0;
                pair |= ((unsigned)s & 0xffffu) << (16 * e);
            }
            out[j] = pair;
        }
        dst[r] = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// ---------------------------------------------------------------------------------------------- b. coefficients -> scan bytes

// The scan order of one image: MCU by MCU; inside one the luma blocks in raster order, then Cb, then Cr.
struct enc_order {
    int nb, hv, ri, mcus;  // blocks per MCU, luma blocks per MCU, MCUs per restart interval, MCUs
};

__device__ __forceinline__ int enc_block_at(const jpeg_geom& g, const enc_order& od, int m, int k)
{
    if (g.ncomp == 1) return m;
    if (k >= od.hv) return g.nbY + (k - od.hv) * g.nbC + m;
    const int my = m / g.mw, mx = m - my * g.mw, v = k / g.hs;
    return (my * g.vs + v) * g.bwY + mx * g.hs + (k - v * g.hs);
}

// MSB-first bit writer at a bit position of a zero-filled buffer of 32-bit words that its neighbours write too: a word this
// lane fills alone leaves with a plain store, the two it may share with an atomic OR.
struct enc_bits {
    unsigned* words;
    long long wi;
    unsigned long long acc;  // the top n bits are this lane's, in front of them the (zero) bits of the lane before
    int n;
    bool shared;

    __device__ __forceinline__ void start(unsigned* buf, long long bitpos)
    {
        words = buf, wi = bitpos >> 5, n = (int)(bitpos & 31), acc = 0, shared = n != 0;
    }
    __device__ __forceinline__ void put(unsigned v, int len)  // len <= 27
    {
        if (len == 0) return;
        acc |= (unsigned long long)v << (64 - n - len);
        n += len;
        if (n >= 32) {
            const unsigned word = __builtin_bswap32((unsigned)(acc >> 32));
            if (shared)
                atomicOr(&words[wi], word);
            else
                words[wi] = word;
            shared = false, ++wi, acc <<= 32, n -= 32;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (n > 0) atomicOr(&words[wi], __builtin_bswap32((unsigned)(acc >> 32)));
    }
};

__device__ __forceinline__ int enc_category(int v) { return 32 - __clz(abs(v)); }

// The codes of one block -> its bit count; WRITE: through `bw` as well.  blk: the block's 64 coefficients in LDS, two per
// dword.  A coefficient outside the baseline categories, or a symbol the table does not hold, sets kEncRange and is left out,
// in both passes alike.
template <bool WRITE>
__device__ __forceinline__ int enc_code_block(const unsigned* __restrict__ blk, int pred, const unsigned* __restrict__ dc,
                                              const unsigned* __restrict__ ac, const unsigned char* __restrict__ zig, enc_bits& bw,
                                              int& err)
{
    int bits = 0;
    auto emit = [&](unsigned e, int v, int s) {
        if (e == 0) {
            err |= kEncRange;
            return;
        }
        const int len = (int)(e >> 16) + s;
        bits += len;
        if (WRITE) bw.put(((e & 0xffffu) << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), len);
    };
    int diff = (int)(short)(blk[0] & 0xffffu) - pred;
    int s = enc_category(diff);
    if (s > 11) err |= kEncRange, diff = 0, s = 0;
    emit(dc[s], diff, s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int at = zig[k];
        int v = (int)(short)((blk[at >> 1] >> (16 * (at & 1))) & 0xffffu);
        s = enc_category(v);
        if (s > 10) err |= kEncRange, v = 0;
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            emit(ac[0xf0], 0, 0);
            run -= 16;
        }
        emit(ac[(run << 4) | s], v, s);
        run = 0;
    }
    if (run > 0) emit(ac[0], 0, 0);
    return bits;
}

// A lane's block as a function of the bit position before it: x -> x + a, or, with h set (a restart interval begins inside),
// x -> align8(x + a) + c.  Such functions compose to one of the same form, so positions come from one scan.
struct enc_fn {
    int h, a, c;
};
__device__ __forceinline__ int enc_align8(int v) { return (v + 7) & ~7; }
__device__ __forceinline__ enc_fn enc_compose(const enc_fn& f, const enc_fn& g)  // f first
{
    if (!g.h) return f.h ? enc_fn{1, f.a, f.c + g.a} : enc_fn{0, f.a + g.a, 0};
    return f.h ? enc_fn{1, f.a, enc_align8(f.c + g.a) + g.c} : enc_fn{1, f.a + g.a, g.c};
}

// One workgroup per image, 256 blocks of the scan order at a time with the bit position carried from one round to the next.
// coef i16 [n][blocks][64]; ubuf u8 [n][ustride], zero-filled, receives the un-stuffed bytes, every interval from a whole
// byte and filled up with 1-bits; marks u8 [n][ustride], zero-filled: 1 at the first byte of every interval but the first;
// ulen i64 [n]: the bytes of ubuf in use.  status: kEncRange / kEncFit.
__global__ void __launch_bounds__(kEncThreads) k_jpeg_entropy_encode(const short* __restrict__ coef, const unsigned char* __restrict__ tables,
                                                                     int n, jpeg_geom g, int restart, unsigned char* __restrict__ ubuf,
                                                                     unsigned char* __restrict__ marks, long long ustride,
                                                                     long long* __restrict__ ulen, int* __restrict__ status)
{
    __shared__ unsigned s_tab[kEncHuffInts];
    __shared__ unsigned char s_zig[64];
    __shared__ unsigned s_blk[kEncThreads * kEncRow];
    __shared__ int s_h[kEncThreads], s_a[kEncThreads], s_c[kEncThreads];
    __shared__ long long s_end[kEncThreads];
    const int t = threadIdx.x, img = blockIdx.x;
    {
        const unsigned* src = reinterpret_cast<const unsigned*>(tables + kEncQuantBytes);
        for (int i = t; i < kEncHuffInts; i += kEncThreads) s_tab[i] = src[i];
        if (t < 64) s_zig[t] = kEncZigzag[t];
    }
    __syncthreads();
    enc_order od;
    od.hv = g.ncomp == 3 ? g.hs * g.vs : 1, od.nb = g.ncomp == 3 ? od.hv + 2 : 1;
    od.mcus = g.mw * g.mh, od.ri = restart > 0 ? restart : od.mcus;
    const short* __restrict__ blocks = coef + (size_t)img * g.blocks * 64;
    unsigned* __restrict__ words = reinterpret_cast<unsigned*>(ubuf + (size_t)img * ustride);
    unsigned char* __restrict__ mk = marks + (size_t)img * ustride;
    const long long cap_bits = ustride * 8;
    long long x = 0;  // the bit position behind everything before this round (the same in every lane)
    int err = 0;
    unsigned* __restrict__ mine = s_blk + t * kEncRow;
    for (int base = 0; base < g.blocks; base += kEncThreads) {
        const int s = base + t;
        const bool live = s < g.blocks;
        int bits = 0, pred = 0, ci = 0;
        bool head = false, last = false;
        if (live) {
            const int m = s / od.nb, k = s - m * od.nb;
            const bool first_mcu = m % od.ri == 0;
            ci = k < od.hv ? 0 : k - od.hv + 1;
            head = k == 0 && first_mcu;
            last = k == od.nb - 1 && ((m + 1) % od.ri == 0 || m + 1 == od.mcus);
            const int at = enc_block_at(g, od, m, k);
            const uint4* __restrict__ cp = reinterpret_cast<const uint4*>(blocks + (size_t)at * 64);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint4 v = cp[r];
                mine[4 * r] = v.x, mine[4 * r + 1] = v.y, mine[4 * r + 2] = v.z, mine[4 * r + 3] = v.w;
            }
            // the predictor: the block of this component coded before this one, 0 at the start of an interval
            if (ci == 0 && k > 0)
                pred = blocks[(size_t)enc_block_at(g, od, m, k - 1) * 64];
            else if (!first_mcu)
                pred = blocks[(size_t)enc_block_at(g, od, m - 1, ci == 0 ? od.hv - 1 : k) * 64];
            enc_bits none;
            bits = enc_code_block<false>(mine, pred, s_tab + (ci ? 272 : 0), s_tab + (ci ? 272 : 0) + 16, s_zig, none, err);
        }
        // inclusive scan of the lanes' functions
        enc_fn f = head ? enc_fn{1, 0, bits} : enc_fn{0, bits, 0};
        s_h[t] = f.h, s_a[t] = f.a, s_c[t] = f.c;
        __syncthreads();
        for (int d = 1; d < kEncThreads; d <<= 1) {
            enc_fn p{0, 0, 0};
            if (t >= d) p = enc_fn{s_h[t - d], s_a[t - d], s_c[t - d]};
            __syncthreads();
            if (t >= d) {
                f = enc_compose(p, f);
                s_h[t] = f.h, s_a[t] = f.a, s_c[t] = f.c;
            }
            __syncthreads();
        }
        s_end[t] = f.h ? ((x + f.a + 7) & ~7LL) + f.c : x + f.a;
        __syncthreads();
        const long long before = t > 0 ? s_end[t - 1] : x;
        const long long start = head ? (before + 7) & ~7LL : before;
        x = s_end[kEncThreads - 1];
        if (live) {
            const int fill = last ? (int)(-(start + bits) & 7) : 0;
            if (start + bits + fill > cap_bits) {
                err |= kEncFit;  // the bound of the shape holds every image: only a buffer smaller than asked for comes here
            } else {
                enc_bits bw;
                bw.start(words, start);
                int again = 0;
                enc_code_block<true>(mine, pred, s_tab + (ci ? 272 : 0), s_tab + (ci ? 272 : 0) + 16, s_zig, bw, again);
                bw.put((1u << fill) - 1u, fill);
                bw.finish();
                if (head && s > 0) mk[start >> 3] = 1;
            }
        }
        __syncthreads();
    }
    if (err != 0) atomicOr(&status[img], err);
    if (t == 0) ulen[img] = min((x + 7) >> 3, ustride);
}

// One workgroup per image over its un-stuffed bytes, four per lane and round.  Byte i goes to i + (FF bytes before it) +
// 2 (intervals that begin at or before it).  WRITE = false: lengths[img] alone.  WRITE = true: the bytes, behind the images
// before this one (the sum of their lengths); an image that does not fit out_bytes gets kEncFit and writes nothing.
template <bool WRITE>
__global__ void __launch_bounds__(kEncThreads) k_jpeg_stuff(const unsigned char* __restrict__ ubuf, const unsigned char* __restrict__ marks,
                                                            long long ustride, const long long* __restrict__ ulen, int n,
                                                            int* __restrict__ lengths, unsigned char* __restrict__ out,
                                                            long long out_bytes, int* __restrict__ status)
{
    __shared__ long long s_sum[kEncThreads];
    __shared__ int s_e[kEncThreads], s_k[kEncThreads];
    const int t = threadIdx.x, img = blockIdx.x;
    const long long U = ulen[img];
    long long off = 0;
    if (WRITE) {
        long long part = 0;
        for (int i = t; i < img; i += kEncThreads) part += lengths[i];
        s_sum[t] = part;
        __syncthreads();
        for (int d = kEncThreads / 2; d > 0; d >>= 1) {
            if (t < d) s_sum[t] += s_sum[t + d];
            __syncthreads();
        }
        off = s_sum[0];
        if (off + lengths[img] > out_bytes) {  // the same in every lane
            if (t == 0) atomicOr(&status[img], kEncFit);
            return;
        }
    }
    const unsigned* __restrict__ words = reinterpret_cast<const unsigned*>(ubuf + (size_t)img * ustride);
    const unsigned* __restrict__ mwords = reinterpret_cast<const unsigned*>(marks + (size_t)img * ustride);
    unsigned char* __restrict__ dst = out + off;
    long long E = 0, K = 0;  // FF bytes + 2 per marker, and markers, before this round
    for (long long base = 0; base < U; base += 4 * kEncThreads) {
        const long long i0 = base + 4 * t;
        unsigned u = 0, mw = 0;
        if (i0 < U) u = words[i0 >> 2], mw = mwords[i0 >> 2];  // ustride is a multiple of 4; bytes behind U are zero
        int e = 0, k = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < U;
            const int m = in ? (int)((mw >> (8 * j)) & 1u) : 0;
            e += 2 * m + (in && ((u >> (8 * j)) & 0xffu) == 0xffu ? 1 : 0);
            k += m;
        }
        int ie = e, ik = k;  // inclusive sums
        s_e[t] = ie, s_k[t] = ik;
        __syncthreads();
        for (int d = 1; d < kEncThreads; d <<= 1) {
            int pe = 0, pk = 0;
            if (t >= d) pe = s_e[t - d], pk = s_k[t - d];
            __syncthreads();
            ie += pe, ik += pk;
            s_e[t] = ie, s_k[t] = ik;
            __syncthreads();
        }
        if (WRITE) {
            long long ee = E + ie - e, kk = K + ik - k;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= U) break;
                const unsigned b = (u >> (8 * j)) & 0xffu;
                if ((mw >> (8 * j)) & 1u) {
                    dst[i0 + j + ee] = 0xff;
                    dst[i0 + j + ee + 1] = (unsigned char)(0xd0 + (int)(kk & 7));
                    ee += 2, ++kk;
                }
                dst[i0 + j + ee] = (unsigned char)b;
                if (b == 0xffu) {
                    ++ee;
                    dst[i0 + j + ee] = 0;
                }
            }
        }
        E += s_e[kEncThreads - 1], K += s_k[kEncThreads - 1];
        __syncthreads();
    }
    if (!WRITE && t == 0) {
        const long long total = U + E;
        lengths[img] = (int)min(total, 0x7fffffffLL);
        if (total > 0x7fffffffLL) atomicOr(&status[img], kEncFit);
    }
}

// the un-stuffed bytes one image may take: the bound of every block, one byte of fill per interval, a multiple of 16
long long enc_ustride(const jpeg_geom& g, int restart)
{
    const long long mcus = (long long)g.mw * g.mh;
    const long long intervals = restart > 0 ? (mcus + restart - 1) / restart : 1;
    return (((long long)g.blocks * kEncBlockBits + 7) / 8 + intervals + 15) / 16 * 16;
}

bool enc_shape_ok(int n, int w, int h, int ncomp, int hs, int vs, int restart)
{
    if (!jpeg_shape_ok(n, w, h, ncomp, hs, vs) || restart < 0 || restart > 65535) return false;
    const jpeg_geom g = jpeg_make_geom(w, h, ncomp, hs, vs);
    return 2 * enc_ustride(g, restart) + 2LL * g.mw * g.mh <= 0x7fffffffLL;  // the length of one image is an int
}

size_t enc_coef_bytes(int n, const jpeg_geom& g) { return va_align_up((size_t)n * g.blocks * 128, 256); }

int enc_launch_fdct(const unsigned char* images, const unsigned char* tables, int n, const jpeg_geom& g, short* coef, hipStream_t st)
{
    const long long blocks = jpeg_grid((long long)n * g.blocks, kEncThreads);
    VA_CHECK_ARG(blocks > 0, "va_jpeg_fdct: %d images of %dx%d exceed one launch", n, g.w, g.h);
    const unsigned gr = (unsigned)blocks;
    if (g.ncomp == 1)
        k_jpeg_fdct<1, 1, 1><<<gr, kEncThreads, 0, st>>>(images, tables, n, g, coef);
    else if (g.hs == 1)
        k_jpeg_fdct<3, 1, 1><<<gr, kEncThreads, 0, st>>>(images, tables, n, g, coef);
    else if (g.vs == 1)
        k_jpeg_fdct<3, 2, 1><<<gr, kEncThreads, 0, st>>>(images, tables, n, g, coef);
    else
        k_jpeg_fdct<3, 2, 2><<<gr, kEncThreads, 0, st>>>(images, tables, n, g, coef);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// stage b on `work`: ubuf, marks, ulen
int enc_launch_entropy(const short* coef, const unsigned char* tables, int n, const jpeg_geom& g, int restart, unsigned char* out,
                       size_t out_bytes, int* lengths, int* status, unsigned char* work, hipStream_t st)
{
    const long long ustride = enc_ustride(g, restart);
    unsigned char* ubuf = work;
    unsigned char* marks = work + (size_t)n * ustride;
    long long* ulen = reinterpret_cast<long long*>(work + 2 * (size_t)n * ustride);
    VA_HIP(hipMemsetAsync(work, 0, 2 * (size_t)n * ustride, st));
    VA_HIP(hipMemsetAsync(status, 0, (size_t)n * 4, st));
    k_jpeg_entropy_encode<<<(unsigned)n, kEncThreads, 0, st>>>(coef, tables, n, g, restart, ubuf, marks, ustride, ulen, status);
    VA_LAUNCH_CHECK();
    k_jpeg_stuff<false><<<(unsigned)n, kEncThreads, 0, st>>>(ubuf, marks, ustride, ulen, n, lengths, out, (long long)out_bytes, status);
    VA_LAUNCH_CHECK();
    k_jpeg_stuff<true><<<(unsigned)n, kEncThreads, 0, st>>>(ubuf, marks, ustride, ulen, n, lengths, out, (long long)out_bytes, status);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

size_t enc_entropy_bytes(int n, const jpeg_geom& g, int restart) { return 2 * (size_t)n * enc_ustride(g, restart) + (size_t)n * 8; }

}  // namespace

extern "C" size_t va_jpeg_encode_workspace_bytes(int n, int w, int h, int ncomp, int hs, int vs, int restart)
{
    if (!enc_shape_ok(n, w, h, ncomp, hs, vs, restart)) return 0;
    const jpeg_geom g = jpeg_make_geom(w, h, ncomp, hs, vs);
    return va_align_up(enc_entropy_bytes(n, g, restart), 256) + enc_coef_bytes(n, g);
}

#define VA_ENC_COMMON(who)                                                                                                          \
    VA_CHECK_ARG(ctx != nullptr, who ": ctx is NULL");                                                                              \
    VA_USE_DEVICE(ctx);                                                                                                             \
    VA_CHECK_ARG(enc_shape_ok(n, w, h, ncomp, hs, vs, restart),                                                                     \
                 who ": bad shape (%d images of %dx%d, %d components, luma sampling %dx%d, restart interval %d)", n, w, h, ncomp, hs, \
                 vs, restart);                                                                                                      \
    const jpeg_geom g = jpeg_make_geom(w, h, ncomp, hs, vs)

extern "C" int va_jpeg_fdct(va_ctx* ctx, const void* images, const void* tables, int n, int w, int h, int ncomp, int hs, int vs, void* coef,
                            void* stream)
{
    const int restart = 0;
    VA_ENC_COMMON("va_jpeg_fdct");
    VA_CHECK_ARG(images != nullptr && tables != nullptr && coef != nullptr, "va_jpeg_fdct: NULL buffer");
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(tables) % 16 == 0 && reinterpret_cast<uintptr_t>(coef) % 16 == 0,
                 "va_jpeg_fdct: tables and coef must be 16-byte aligned");
    return enc_launch_fdct((const unsigned char*)images, (const unsigned char*)tables, n, g, (short*)coef, (hipStream_t)stream);
}

extern "C" int va_jpeg_entropy_encode(va_ctx* ctx, const void* coef, const void* tables, int n, int w, int h, int ncomp, int hs, int vs,
                                      int restart, void* out, size_t out_bytes, void* lengths, void* status, void* workspace,
                                      size_t workspace_bytes, void* stream)
{
    VA_ENC_COMMON("va_jpeg_entropy_encode");
    VA_CHECK_ARG(coef != nullptr && tables != nullptr && out != nullptr && lengths != nullptr && status != nullptr,
                 "va_jpeg_entropy_encode: NULL buffer");
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(tables) % 16 == 0 && reinterpret_cast<uintptr_t>(coef) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(lengths) % 4 == 0 && reinterpret_cast<uintptr_t>(status) % 4 == 0,
                 "va_jpeg_entropy_encode: tables and coef must be 16-byte, lengths and status 4-byte aligned");
    const size_t need = enc_entropy_bytes(n, g, restart);
    if (workspace == nullptr || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        va_set_error("va_jpeg_entropy_encode: the workspace holds %zu bytes, %zu are needed (16-byte aligned)",
                     workspace == nullptr ? (size_t)0 : workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    return enc_launch_entropy((const short*)coef, (const unsigned char*)tables, n, g, restart, (unsigned char*)out, out_bytes, (int*)lengths,
                              (int*)status, (unsigned char*)workspace, (hipStream_t)stream);
}

extern "C" int va_jpeg_encode(va_ctx* ctx, const void* images, int n, int w, int h, int ncomp, int hs, int vs, int restart,
                              const void* tables, void* out, size_t out_bytes, void* lengths, void* status, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    VA_ENC_COMMON("va_jpeg_encode");
    VA_CHECK_ARG(images != nullptr && tables != nullptr && out != nullptr && lengths != nullptr && status != nullptr,
                 "va_jpeg_encode: NULL buffer");
    VA_CHECK_ARG(reinterpret_cast<uintptr_t>(tables) % 16 == 0 && reinterpret_cast<uintptr_t>(lengths) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(status) % 4 == 0,
                 "va_jpeg_encode: tables must be 16-byte, lengths and status 4-byte aligned");
    const size_t need = va_jpeg_encode_workspace_bytes(n, w, h, ncomp, hs, vs, restart);
    if (workspace == nullptr || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        va_set_error("va_jpeg_encode: the workspace holds %zu bytes, %zu are needed (16-byte aligned)",
                     workspace == nullptr ? (size_t)0 : workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    unsigned char* work = (unsigned char*)workspace;
    short* coefs = (short*)(work + va_align_up(enc_entropy_bytes(n, g, restart), 256));
    const int rc = enc_launch_fdct((const unsigned char*)images, (const unsigned char*)tables, n, g, coefs, (hipStream_t)stream);
    if (rc != VA_OK) return rc;
    return enc_launch_entropy(coefs, (const unsigned char*)tables, n, g, restart, (unsigned char*)out, out_bytes, (int*)lengths, (int*)status,
                              work, (hipStream_t)stream);
}
