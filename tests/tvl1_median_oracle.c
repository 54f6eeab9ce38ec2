/*
 * tests/tvl1_median_oracle.c  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The CPU oracle of oracle/tvl1_oracle.c with the median filter of DESIGN.md S55: the flow u1, u2 is replaced by its
 * k x k median (k = 3 or 5) at the head of every inner iteration `it` with it % median_every == 0.  The stock file is
 * included, not copied: its statics (bilinear, divergence_at, pyr_build, pyr_free) and its arithmetic contract are
 * reused; only the level and the driver are restated, operation for operation, with the filter in place.  Build with
 * the flags of oracle/Makefile (-ffp-contract=off).
 *
 *   S55  median in {0, 3, 5}; median_every >= 0, 0 meaning `iters`.  After S5 has computed the warp's constants from the
 *        unfiltered u, at the head of inner iteration it (it = 0 included) with it % median_every == 0: u1 and u2 are
 *        each replaced by their k x k median; window centred on the pixel, coordinates clamped to the level's frame,
 *        every sample read from the values before the filter; the result is the ((k*k+1)/2)-th smallest sample (exact
 *        selection).  p is untouched.  With epsilon > 0 the filter is the first statement of the loop body: a pair that
 *        has stopped is not filtered again in that warp, and the first error sum after a filter measures the step from
 *        the filtered field.
 */
#include "../oracle/tvl1_oracle.c"

/* k x k median of one plane, src -> dst (src != dst).  Selection by insertion sort of the k*k samples. */
static void median_plane(const float* src, float* dst, int w, int h, int k)
{
    const int r = k / 2, n = k * k;
    int x, y, dx, dy, i, j;
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) {
            float v[25];
            i = 0;
            for (dy = -r; dy <= r; dy++)
                for (dx = -r; dx <= r; dx++)
                    v[i++] = src[(size_t)imin(imax(y + dy, 0), h - 1) * w + imin(imax(x + dx, 0), w - 1)];
            for (i = 1; i < n; i++) {
                const float t = v[i];
                for (j = i; j > 0 && v[j - 1] > t; j--) v[j] = v[j - 1];
                v[j] = t;
            }
            dst[(size_t)y * w + x] = v[n / 2];
        }
}

/* The filter on a dense field [n][2][h][w].  Returns 0, or -1 on bad arguments. */
int ora_flow_median(const float* flow, int n_fields, int w, int h, int k, float* out)
{
    int f;
    if (!flow || !out || flow == out || n_fields < 1 || w < 1 || h < 1 || (k != 3 && k != 5)) return -1;
    for (f = 0; f < 2 * n_fields; f++) median_plane(flow + (size_t)f * w * h, out + (size_t)f * w * h, w, h, k);
    return 0;
}

/* S4-S7 with S55: ora_tvl1_level restated; median = 0 is ora_tvl1_level. */
long ora_tvl1_median_level(const float* I0, const float* I1, const float* I1x, const float* I1y, int w, int h,
                           const ora_tvl1_params* P, int median, int median_every, float* u1, float* u2)
{
    size_t n = (size_t)w * h;
    float* buf = (float*)calloc(n * 10, sizeof(float));
    float *p11 = buf, *p12 = buf + n, *p21 = buf + 2 * n, *p22 = buf + 3 * n;
    float *wx = buf + 4 * n, *wy = buf + 5 * n, *rc = buf + 6 * n, *ig = buf + 7 * n;
    float *n1 = buf + 8 * n, *n2 = buf + 9 * n;
    const float l_t = P->lambda * P->theta;
    const float taut = P->tau / P->theta;
    const float theta = P->theta;
    const int fixed = !(P->epsilon > 0.0f);
    const uint64_t qthr = fixed ? 0 : (uint64_t)((double)P->epsilon * (double)P->epsilon * (double)n * 4294967296.0);
    const int every = median_every > 0 ? median_every : P->iters;
    long total = 0;
    int wp, it, x, y;

    for (wp = 0; wp < P->warps; wp++) {
        /* S5 (from the unfiltered u) */
        for (y = 0; y < h; y++)
            for (x = 0; x < w; x++) {
                float fxp, fyp, Iw, Iwx, Iwy, grad;
                const size_t i = (size_t)y * w + x;
                fxp = (float)x + u1[i]; fyp = (float)y + u2[i];
                Iw = bilinear(I1, w, h, fxp, fyp);
                Iwx = bilinear(I1x, w, h, fxp, fyp);
                Iwy = bilinear(I1y, w, h, fxp, fyp);
                grad = fmaf(Iwy, Iwy, Iwx * Iwx);
                wx[i] = Iwx; wy[i] = Iwy;
                ig[i] = grad < 1e-10f ? 0.0f : 1.0f / grad;
                rc[i] = fmaf(-Iwy, u2[i], fmaf(-Iwx, u1[i], Iw - I0[i]));
            }
        for (it = 0; it < P->iters; it++) {
            uint64_t qsum = 0;
            /* S55 */
            if (median && it % every == 0) {
                median_plane(u1, n1, w, h, median);
                median_plane(u2, n2, w, h, median);
                memcpy(u1, n1, n * sizeof(float));
                memcpy(u2, n2, n * sizeof(float));
            }
            /* S6, S7 */
            for (y = 0; y < h; y++)
                for (x = 0; x < w; x++) {
                    float rho, fi, v1, v2, a, b;
                    const size_t i = (size_t)y * w + x;
                    rho = fmaf(wy[i], u2[i], fmaf(wx[i], u1[i], rc[i]));
                    fi = fminf(fmaxf(-rho * ig[i], -l_t), l_t);
                    v1 = fmaf(fi, wx[i], u1[i]);
                    v2 = fmaf(fi, wy[i], u2[i]);
                    a = fmaf(theta, divergence_at(p11, p12, w, h, x, y), v1);
                    b = fmaf(theta, divergence_at(p21, p22, w, h, x, y), v2);
                    if (!fixed) {
                        float d1 = a - u1[i], d2 = b - u2[i];
                        float e = fmaf(d2, d2, d1 * d1);
                        qsum += (uint64_t)(fminf(e, 1024.0f) * 4294967296.0f);
                    }
                    n1[i] = a; n2[i] = b;
                }
            memcpy(u1, n1, n * sizeof(float));
            memcpy(u2, n2, n * sizeof(float));
            for (y = 0; y < h; y++)
                for (x = 0; x < w; x++) {
                    float u1x, u1y, u2x, u2y, d1, d2, rinv, r1, r2;
                    const size_t i = (size_t)y * w + x;
                    u1x = x < w - 1 ? u1[i + 1] - u1[i] : 0.0f;
                    u1y = y < h - 1 ? u1[i + w] - u1[i] : 0.0f;
                    u2x = x < w - 1 ? u2[i + 1] - u2[i] : 0.0f;
                    u2y = y < h - 1 ? u2[i + w] - u2[i] : 0.0f;
                    d1 = fmaf(taut, sqrtf(fmaf(u1y, u1y, fmaf(u1x, u1x, ORA_NORM_REG))), 1.0f);
                    d2 = fmaf(taut, sqrtf(fmaf(u2y, u2y, fmaf(u2x, u2x, ORA_NORM_REG))), 1.0f);
                    rinv = 1.0f / (d1 * d2);
                    r1 = d2 * rinv;
                    r2 = d1 * rinv;
                    p11[i] = fmaf(taut, u1x, p11[i]) * r1;
                    p12[i] = fmaf(taut, u1y, p12[i]) * r1;
                    p21[i] = fmaf(taut, u2x, p21[i]) * r2;
                    p22[i] = fmaf(taut, u2y, p22[i]) * r2;
                }
            total++;
            if (!fixed && qsum < qthr) break;
        }
    }
    free(buf);
    return total;
}

/* ora_tvl1_flow restated over ora_tvl1_median_level (same arguments, plus the two options). */
int ora_tvl1_median_flow(const float* frames, int n_seq, int frames_per_seq, int w, int h, const ora_tvl1_params* P,
                         int median, int median_every, float* flow, long* iters_run, int nthreads)
{
    int ws[ORA_MAX_SCALES], hs[ORA_MAX_SCALES];
    int ns, npairs, pi;
    if (!frames || !flow || !P || n_seq < 1 || frames_per_seq < 2 || w < 1 || h < 1) return -1;
    if (P->nscales < 1 || P->warps < 1 || P->iters < 1 || !(P->scale_step > 0.0f && P->scale_step < 1.0f) ||
        !(P->theta > 0.0f) || !(P->tau > 0.0f) || !(P->lambda > 0.0f)) return -1;
    if ((median != 0 && median != 3 && median != 5) || median_every < 0) return -1;
    ns = ora_tvl1_pyramid_sizes(w, h, P->nscales, P->scale_step, ws, hs);
    npairs = n_seq * (frames_per_seq - 1);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#else
    (void)nthreads;
#endif
#pragma omp parallel for schedule(dynamic, 1) if (npairs > 1)
    for (pi = 0; pi < npairs; pi++) {
        int sq = pi / (frames_per_seq - 1), k = pi % (frames_per_seq - 1), s;
        const float* f0 = frames + ((size_t)sq * frames_per_seq + k) * (size_t)w * h;
        const float* f1 = f0 + (size_t)w * h;
        ora_pyr A, B;
        float *u1, *u2;
        long total = 0;
        pyr_build(&A, f0, ns, ws, hs, P->scale_step);
        pyr_build(&B, f1, ns, ws, hs, P->scale_step);
        u1 = (float*)calloc((size_t)ws[ns - 1] * hs[ns - 1], sizeof(float));
        u2 = (float*)calloc((size_t)ws[ns - 1] * hs[ns - 1], sizeof(float));
        for (s = ns - 1; s >= 0; s--) {
            total += ora_tvl1_median_level(A.I[s], B.I[s], B.Ix[s], B.Iy[s], ws[s], hs[s], P, median, median_every, u1, u2);
            if (s > 0) {
                size_t nf = (size_t)ws[s - 1] * hs[s - 1];
                float* f1u = (float*)malloc(nf * sizeof(float));
                float* f2u = (float*)malloc(nf * sizeof(float));
                ora_tvl1_upsample_flow(u1, ws[s], hs[s], f1u, ws[s - 1], hs[s - 1], P->scale_step);
                ora_tvl1_upsample_flow(u2, ws[s], hs[s], f2u, ws[s - 1], hs[s - 1], P->scale_step);
                free(u1); free(u2); u1 = f1u; u2 = f2u;
            }
        }
        memcpy(flow + (size_t)pi * 2 * w * h, u1, (size_t)w * h * sizeof(float));
        memcpy(flow + ((size_t)pi * 2 + 1) * w * h, u2, (size_t)w * h * sizeof(float));
        if (iters_run) iters_run[pi] = total;
        free(u1); free(u2);
        pyr_free(&A, ns); pyr_free(&B, ns);
    }
    return 0;
}
