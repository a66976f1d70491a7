// pxl_polyfilter.h -- the per-scan polynomial filter of a (D, T) timestream: for every detector and every
// segment [seg_start[s], seg_start[s+1]) a Legendre polynomial of degree <= ORD is fitted to the samples with wfit > 0 and
// subtracted from ALL samples of the segment; included by pxl_kernels.hip after pxl_baseline.h (one translation unit,
// -ffp-contract=off: every product and every sum below is rounded once, nothing is fused).
//
// THE DEFINITION, operation by operation.  Both ends of a segment are clamped to [0, n_t]; an end that is not above its start
// makes the segment empty.  A segment of L samples has, for its sample j = 0 .. L - 1,
//     x_j = double((2 j + 1) - L) / double(L)                          the integer exact, the division one rounding
//     P_0 = 1,  P_1 = x,  P_(n+1) = ((double(2n+1) * x) * P_n  -  double(n) * P_(n-1)) / double(n+1)     (legendre below)
// A sample is LIVE when wfit > 0 (a NaN weight is not; a null wfit is 1.0 everywhere).  Over the live samples
//     G_ik = sum (w * P_i) * P_k   for i >= k,        b_i = sum (w * P_i) * d
// each term two roundings; a sample that is not live adds no term, and its d enters no arithmetic at all.
//
// OWNERSHIP, no atomics.  One group of G lanes (G a power of two, 1 to 64, or 256, chosen by the host from n_t, n_seg and the
// order alone: polyfilter_group in pxl_kernels.hip) owns one (detector, segment).  Lane l adds the terms of the live samples
// j = l, l + G, l + 2G, ... in that order into its own 44 (for ORD = 7) sums, each starting from +0.0.  The lane sums are joined by
// a fixed tree: within a wavefront level by level, v_l = v_l + v_(l ^ off) for off = G/2, ..., 1 (capped at 32) -- IEEE addition
// commutes, so every lane of the group ends with the bits lane 0 has, which are those of the tree l += l + off; for G = 256
// the four wavefronts' sums go through LDS and every lane forms (s0 + s1) + (s2 + s3).  The bits depend on the arguments alone.
// A group of G < 64 lanes shares its wavefront with 64 / G - 1 other segments.
//
// THE SOLVE (poly_solve below, every lane of the group redundantly, in registers): LDL^T of G without pivoting, in the
// Legendre order.  Row i, for k = 0 .. i-1 in order:  U_ik = G_ik - U_i0 * L_k0 - ... - U_i,k-1 * L_k,k-1 (left to right),
// L_ik = U_ik / D_k;  D_i = G_ii - U_i0 * L_i0 - ... - U_i,i-1 * L_i,i-1 (left to right).  Pivot i is ACCEPTED when
// D_i > rcond_min * G_ii (a NaN fails); the fit is truncated at the first rejected pivot, n_used = the number of accepted
// leading pivots.  Then y_i = b_i - L_i0 * y_0 - ... - L_i,i-1 * y_i-1 for i < n_used, and from i = n_used - 1 down
// c_i = y_i / D_i - L_i+1,i * c_i+1 - ... - L_nu-1,i * c_nu-1 (left to right); c_i = +0.0 for i >= n_used.
//
// THE SECOND PASS, over every sample of the segment, live or not:  f = c_0, then f = f + c_n * P_n for n = 1 .. ORD in order, and
// out_j = d_j - f.  With n_used = 0 out_j = d_j, the bits copied (and not written at all when out is d).
//
// The samples before the first segment and from the end of the last on are two more items per detector that skip the first
// pass: their sums stay +0.0, pivot 0 is rejected (0 > 0 fails), and the second pass copies them.  So every lane runs the same
// code, the shuffles and the barriers are never divergent, and the only loops whose trip counts differ within a wavefront are
// the two passes.  out may be exactly d: a sample is read and written by the same lane, and every first-pass read of a
// segment precedes its first write (the wavefront runs in step; for G = 256 the barriers of the LDS join stand between).

template <int ORD>
struct PolyFit {
    static constexpr int NP = ORD + 1;                  // coefficients
    static constexpr int NG = NP * (NP + 1) / 2;        // moments G_ik, i >= k, at i * (i + 1) / 2 + k
};
__device__ __forceinline__ constexpr int poly_idx(int i, int k) { return i * (i + 1) / 2 + k; }

template <int ORD>
__device__ __forceinline__ void legendre(double x, double (&P)[ORD + 1]) {
    P[0] = 1.0;
    if constexpr (ORD >= 1) P[1] = x;
#pragma unroll
    for (int n = 1; n < ORD; ++n) P[n + 1] = (((double)(2 * n + 1) * x) * P[n] - (double)n * P[n - 1]) / (double)(n + 1);
}
__device__ __forceinline__ double poly_x(int64_t j, int64_t L) { return (double)((2 * j + 1) - L) / (double)L; }

// LDL^T in place in g (L below the diagonal, D on it, for the rows that were reached), then the two substitutions.  Returns n_used.
template <int ORD>
__device__ __forceinline__ int poly_solve(double (&g)[PolyFit<ORD>::NG], const double (&b)[ORD + 1], double rmin, double (&c)[ORD + 1]) {
    constexpr int NP = ORD + 1;
    int nu = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (nu == i) {
            double u[NP];
            const double gii = g[poly_idx(i, i)];
            double dd = gii;
#pragma unroll
            for (int k = 0; k < i; ++k) {
                double s = g[poly_idx(i, k)];
#pragma unroll
                for (int m = 0; m < k; ++m) s = s - u[m] * g[poly_idx(k, m)];
                u[k] = s;
                const double l = s / g[poly_idx(k, k)];
                g[poly_idx(i, k)] = l;
                dd = dd - s * l;
            }
            g[poly_idx(i, i)] = dd;
            if (dd > rmin * gii) nu = i + 1;
        }
    }
    double y[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        double s = b[i];
#pragma unroll
        for (int m = 0; m < i; ++m) s = s - g[poly_idx(i, m)] * y[m];
        y[i] = s;                                                           // rows from n_used on are never read
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        double s = 0.0;
        if (i < nu) {
            s = y[i] / g[poly_idx(i, i)];
#pragma unroll
            for (int m = i + 1; m < NP; ++m)
                if (m < nu) s = s - g[poly_idx(m, i)] * c[m];
        }
        c[i] = s;
    }
    return nu;
}

template <int ORD>
__global__ __launch_bounds__(256) void k_polyfilter(int64_t n_t, int64_t n_seg, int64_t n_items, const int64_t* __restrict__ seg_start,
                                                    double rmin, int G, const double* d, const double* __restrict__ wfit, double* out,
                                                    double* __restrict__ coeffs, int64_t* __restrict__ n_used) {
    constexpr int NP = PolyFit<ORD>::NP, NG = PolyFit<ORD>::NG;
    __shared__ double wave_sum[4][NG + NP];
    const int lane = threadIdx.x & (G - 1);
    const int64_t item = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool has = item < n_items;
    // an item: (detector, 0) the samples before the first segment, (detector, s + 1) segment s, (detector, n_seg + 1) the rest
    const int64_t det = has ? item / (n_seg + 2) : 0;
    const int64_t sp = has ? item - det * (n_seg + 2) : 0;
    const bool fit = has && sp >= 1 && sp <= n_seg;
    int64_t lo = 0, hi = 0;
    if (has) {
        lo = sp == 0 ? 0 : seg_start[sp - 1];
        hi = sp == n_seg + 1 ? n_t : seg_start[sp];
        lo = lo < 0 ? 0 : lo > n_t ? n_t : lo;
        hi = hi < lo ? lo : hi > n_t ? n_t : hi;
    }
    const int64_t L = hi - lo;
    const int64_t k0 = det * n_t + lo;                                      // the segment's first sample in d, wfit and out

    double g[NG], b[NP];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) b[i] = 0.0;
    if (fit) {
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
                for (int i = 0; i < NP; ++i) {
                    const double wp = wv[u] * P[i];
#pragma unroll
                    for (int k = 0; k <= i; ++k) g[poly_idx(i, k)] = g[poly_idx(i, k)] + wp * P[k];
                    b[i] = b[i] + wp * dv[u];
                }
            }
        }
    }
    // the fixed tree over the group's lanes (partners that stay inside a wavefront)
    for (int off = (G < 64 ? G : 64) >> 1; off > 0; off >>= 1) {
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
    const int nu = poly_solve<ORD>(g, b, rmin, c);
    if (fit && lane == 0) {
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
        double f = c[0];
#pragma unroll
        for (int n = 1; n < NP; ++n) f = f + c[n] * P[n];
        out[k0 + j] = d[k0 + j] - f;
    }
}
