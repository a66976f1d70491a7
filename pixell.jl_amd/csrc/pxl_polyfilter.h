// pxl_polyfilter.h -- the per-scan polynomial filter of a (D, T) timestream: for every detector and every
// segment [seg_start[s], seg_start[s+1]) a Legendre polynomial of degree <= ORD is fitted to the samples with wfit > 0 and
// subtracted from ALL samples of the segment.  The items, the live-sample rule, the moments, the tree rule, the solve and the
// second pass are pxl_fit.h's, stated there; this header holds the basis and who sums what.  Included by pxl_kernels.hip after pxl_fit.h.
//
// THE BASIS.  A segment of L samples has, for its sample j = 0 .. L - 1,
//     x_j = double((2 j + 1) - L) / double(L)                          the integer exact, the division one rounding
//     P_0 = 1,  P_1 = x,  P_(n+1) = ((double(2n+1) * x) * P_n  -  double(n) * P_(n-1)) / double(n+1)     (legendre below)
// so the second pass starts from f = c_0 * 1.0, which is c_0 for every double.
//
// OWNERSHIP.  One group of G lanes (G a power of two, 1 to 64, or 256, chosen by the host from n_t, n_seg and the order alone:
// polyfilter_group in pxl_kernels.hip) owns one (detector, item).  Lane l adds the terms of the live samples j = l, l + G, l + 2G, ...
// in that order into its own 44 (for ORD = 7) sums.  The tree runs off = G/2, ..., 1 (capped at 32) within a wavefront; for
// G = 256 the four wavefronts' sums go through LDS and every lane forms (s0 + s1) + (s2 + s3).  A group of G < 64 lanes shares its
// wavefront with 64 / G - 1 other items, so the only loops whose trip counts differ within a wavefront are the two passes.  In
// place, the wavefront runs in step between a segment's first-pass reads and its writes; for G = 256 the barrier of the LDS join
// stands between.

template <int ORD>
__device__ __forceinline__ void legendre(double x, double (&P)[ORD + 1]) {
    P[0] = 1.0;
    if constexpr (ORD >= 1) P[1] = x;
#pragma unroll
    for (int n = 1; n < ORD; ++n) P[n + 1] = (((double)(2 * n + 1) * x) * P[n] - (double)n * P[n - 1]) / (double)(n + 1);
}
__device__ __forceinline__ double poly_x(int64_t j, int64_t L) { return (double)((2 * j + 1) - L) / (double)L; }

template <int ORD>
__global__ __launch_bounds__(256) void k_polyfilter(unsigned block0, int64_t n_t, int64_t n_seg, int64_t n_items, const int64_t* __restrict__ seg_start,
                                                    double rmin, int G, const double* d, const double* __restrict__ wfit, double* out,
                                                    double* __restrict__ coeffs, int64_t* __restrict__ n_used) {
    constexpr int NP = ORD + 1, NG = Fit<NP>::NG;
    __shared__ double wave_sum[4][NG + NP];
    const int lane = threadIdx.x & (G - 1);
    const int64_t item = (int64_t)(block0 + blockIdx.x) * (256 / G) + threadIdx.x / G;    // block0: launch_chunks in pxl_kernels.hip
    const bool has = item < n_items;
    const int64_t det = has ? item / (n_seg + 2) : 0;
    const int64_t sp = has ? item - det * (n_seg + 2) : 0;
    FitSpan span = {0, 0, false};
    if (has) span = fit_span(sp, seg_start, n_seg, n_t);
    const int64_t L = span.hi - span.lo;
    const int64_t k0 = det * n_t + span.lo;                                 // the segment's first sample in d, wfit and out

    double g[NG], b[NP];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) b[i] = 0.0;
    if (span.fit) {
        for (int64_t j0 = lane; j0 < L; j0 += 2 * (int64_t)G) {             // two samples' loads issued together; the order of the sums is j0, j0 + G
            double wv[2], dv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int64_t j = j0 + (int64_t)u * G;
                const bool in = j < L;
                wv[u] = in ? (wfit ? wfit[k0 + j] : 1.0) : 0.0;
                dv[u] = in ? d[k0 + j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!(wv[u] > 0.0)) continue;
                double P[NP];
                legendre<ORD>(poly_x(j0 + (int64_t)u * G, L), P);
#pragma unroll
                for (int i = 0; i < NP; ++i) {                              // pxl_fit.h, THE MOMENTS
                    const double wp = wv[u] * P[i];
#pragma unroll
                    for (int k = 0; k <= i; ++k) g[fit_idx(i, k)] = g[fit_idx(i, k)] + wp * P[k];
                    b[i] = b[i] + wp * dv[u];
                }
            }
        }
    }
    for (int off = (G < 64 ? G : 64) >> 1; off > 0; off >>= 1) {            // pxl_fit.h, THE TREE: the levels inside a wavefront
#pragma unroll
        for (int i = 0; i < NG; ++i) g[i] = g[i] + __shfl_xor(g[i], off, 64);
#pragma unroll
        for (int i = 0; i < NP; ++i) b[i] = b[i] + __shfl_xor(b[i], off, 64);
    }
    if (G == 256) {
        const int wv = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < NG; ++i) wave_sum[wv][i] = g[i];
#pragma unroll
            for (int i = 0; i < NP; ++i) wave_sum[wv][NG + i] = b[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NG; ++i) g[i] = (wave_sum[0][i] + wave_sum[1][i]) + (wave_sum[2][i] + wave_sum[3][i]);
#pragma unroll
        for (int i = 0; i < NP; ++i) b[i] = (wave_sum[0][NG + i] + wave_sum[1][NG + i]) + (wave_sum[2][NG + i] + wave_sum[3][NG + i]);
    }
    double c[NP];
    const int nu = fit_solve<NP>(g, b, rmin, c);
    if (span.fit && lane == 0) {
        const int64_t f = det * n_seg + (sp - 1);
        if (n_used) n_used[f] = nu;
        if (coeffs) {
#pragma unroll
            for (int i = 0; i < NP; ++i) coeffs[f * NP + i] = c[i];
        }
    }
    if (nu == 0) {
        if (out != d)
            for (int64_t j = lane; j < L; j += G) out[k0 + j] = d[k0 + j];
        return;
    }
    for (int64_t j = lane; j < L; j += G) {
        double P[NP];
        legendre<ORD>(poly_x(j, L), P);
        out[k0 + j] = d[k0 + j] - fit_model(c, P);
    }
}
