// pxl_modefilter.h -- the detector-mode filter of a (D, T) timestream.  For every detector group
// [grp_start[g], grp_start[g+1]) and every time sample t, K amplitudes are fitted to the group's detectors with wfit > 0 on the
// caller's (D, K) couplings F (`modes`), and F c is subtracted from ALL detectors of the group.  The items (along the detector
// axis), the live-sample rule, the moments, the tree rule, the solve (in the caller's mode order) and the second pass are
// pxl_fit.h's, stated there, with the basis B = row r of F; this header holds who sums what.  Included by pxl_kernels.hip after pxl_fit.h.
//
// OWNERSHIP.  A block of 256 lanes owns one (item, tile of C consecutive time samples), C = 64 or 16 chosen by the host from n_t
// and n_grp alone (modefilter_tile in pxl_kernels.hip): 64 where n_grp * ceil(n_t / 64) >= 512, the wide tile alone making two
// blocks for each of the 256 compute units, else 16.  Lane l holds column l % C of the tile and row phase p = l / C of
// R = 256 / C: lanes run along t, so every load and store of a row is contiguous.  Phase p adds the terms of the live detectors
// lo + p, lo + p + R, ... in that order into its own K (K + 1) / 2 + K sums.  The phases of a column are joined by the tree,
// off = R/2, ..., 1 in phases.  Phases R/2 and R/4 apart sit in other wavefronts (lanes 128 and 64 apart) and meet through LDS,
// at most 11 sums at a time; for C = 16 the last two levels (lanes 32 and 16 apart) are shuffles.  Every lane of a column solves,
// and the second pass runs by the same phases.  A tile that runs past n_t masks its lanes the way a copied item does.  In place,
// the barrier of the join stands between a block's first-pass reads and its writes.  amps (n_grp, K, n_t) and n_used (n_grp, n_t)
// are written by phase 0.

template <int K>
__global__ __launch_bounds__(256) void k_modefilter(unsigned block0, int64_t n_det, int64_t n_t, int64_t n_grp, int64_t n_tiles, const int64_t* __restrict__ grp_start,
                                                    const double* __restrict__ modes, double rmin, int C, const double* d,
                                                    const double* __restrict__ wfit, double* out, double* __restrict__ amps,
                                                    int64_t* __restrict__ n_used) {
    constexpr int NG = Fit<K>::NG, NV = Fit<K>::NV;
    constexpr int CH = NV < 11 ? NV : 11;                                   // sums that cross the wavefronts together
    constexpr int UNR = K <= 4 ? 4 : 2;                                     // rows whose loads are issued together
    __shared__ double part[4][CH][64];
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int R = 256 / C;
    const int p = threadIdx.x / C;
    const int64_t bid = (int64_t)(block0 + blockIdx.x);                     // block0: launch_chunks in pxl_kernels.hip
    const int64_t sp = bid / n_tiles;
    const int64_t t = (bid - sp * n_tiles) * C + (threadIdx.x & (C - 1));
    const bool col = t < n_t;
    const FitSpan span = fit_span(sp, grp_start, n_grp, n_det);
    const int64_t lo = span.lo, hi = span.hi;

    double v[NV];                                                           // the moments, then b_i at NG + i
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0;
    if (span.fit && col) {
        for (int64_t r0 = lo + p; r0 < hi; r0 += (int64_t)UNR * R) {        // the order of the sums is r0, r0 + R, ...
            double wv[UNR], dv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int64_t r = r0 + (int64_t)u * R;
                const bool in = r < hi;
                wv[u] = in ? (wfit ? wfit[r * n_t + t] : 1.0) : 0.0;
                dv[u] = in ? d[r * n_t + t] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (!(wv[u] > 0.0)) continue;
                const double* F = modes + (r0 + (int64_t)u * R) * K;
#pragma unroll
                for (int i = 0; i < K; ++i) {                               // pxl_fit.h, THE MOMENTS
                    const double wf = wv[u] * F[i];
#pragma unroll
                    for (int k = 0; k <= i; ++k) v[fit_idx(i, k)] = v[fit_idx(i, k)] + wf * F[k];
                    v[NG + i] = v[NG + i] + wf * dv[u];
                }
            }
        }
    }
    // the two tree levels whose partners are other wavefronts: (v_w + v_(w ^ 2)) + (v_(w ^ 1) + v_(w ^ 3)), CH sums at a time
#pragma unroll
    for (int c0 = 0; c0 < NV; c0 += CH) {
        if (c0) __syncthreads();
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if (c0 + i < NV) part[wave][i][ln] = v[c0 + i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if (c0 + i < NV) v[c0 + i] = (v[c0 + i] + part[wave ^ 2][i][ln]) + (part[wave ^ 1][i][ln] + part[wave ^ 3][i][ln]);
    }
    for (int off = 32; off >= C; off >>= 1) {                               // C = 16: the levels that stay inside a wavefront
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = v[i] + __shfl_xor(v[i], off, 64);
    }
    double g[NG], b[K], c[K];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = v[i];
#pragma unroll
    for (int i = 0; i < K; ++i) b[i] = v[NG + i];
    const int nu = fit_solve<K>(g, b, rmin, c);
    if (span.fit && col && p == 0) {
        if (n_used) n_used[(sp - 1) * n_t + t] = nu;
        if (amps) {
#pragma unroll
            for (int i = 0; i < K; ++i) amps[((sp - 1) * K + i) * n_t + t] = c[i];
        }
    }
    if (!col || (nu == 0 && out == d)) return;
    for (int64_t r0 = lo + p; r0 < hi; r0 += (int64_t)UNR * R) {
        double dv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t r = r0 + (int64_t)u * R;
            dv[u] = r < hi ? d[r * n_t + t] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t r = r0 + (int64_t)u * R;
            if (r >= hi) continue;
            if (nu == 0) {
                out[r * n_t + t] = dv[u];
                continue;
            }
            out[r * n_t + t] = dv[u] - fit_model(c, modes + r * K);
        }
    }
}
