// pxl_modefilter.h -- the detector-mode filter of a (D, T) timestream: the transposed problem of pxl_polyfilter.h.
// For every detector group [grp_start[g], grp_start[g+1]) and every time sample t, K amplitudes are fitted to the group's detectors
// with wfit > 0 on the caller's (D, K) couplings F (`modes`), and F c is subtracted from ALL detectors of the group.  Included by
// pxl_kernels.hip after pxl_polyfilter.h, whose PolyFit, poly_idx and poly_solve it uses unchanged (one translation unit,
// -ffp-contract=off: every product and every sum below is rounded once, nothing is fused).
//
// THE DEFINITION, operation by operation.  Both ends of a group are clamped to [0, n_det]; an end that is not above its start
// makes the group empty.  Detector r at time t is LIVE when wfit[r,t] > 0 (a NaN weight is not; a null wfit is 1.0 everywhere).
// Over the live detectors of the group, with w = wfit[r,t],
//     G_ik = sum (w * F_ri) * F_rk   for i >= k,        b_i = sum (w * F_ri) * d[r,t]
// each term two roundings; a detector that is not live adds no term, and its d enters no arithmetic at all.
//
// OWNERSHIP, no atomics.  A block of 256 lanes owns one (group, tile of C consecutive time samples), C = 64 or 16 chosen by the host
// from n_t and n_grp alone (modefilter_tile in pxl_kernels.hip): 64 where n_grp * ceil(n_t / 64) >= 512, the wide tile alone making
// two blocks for each of the 256 compute units, else 16.  Lane l holds column l % C of the tile and row phase p = l / C of
// R = 256 / C: lanes run along t, so every load and store of a row is contiguous.  Phase p adds the terms of the live detectors
// lo + p, lo + p + R, ... in that order into its own K (K + 1) / 2 + K sums, each starting from +0.0.  The phases of a column are
// joined by polyfilter's tree rule, v_p = v_p + v_(p ^ off) for off = R/2, ..., 1 -- IEEE addition commutes, so every phase ends
// with the bits phase 0 has.  Phases R/2 and R/4 apart sit in other wavefronts (lanes 128 and 64 apart) and meet through LDS,
// at most 11 sums at a time; for C = 16 the last two levels (lanes 32 and 16 apart) are shuffles.  The bits depend on the
// arguments alone.
//
// THE SOLVE is poly_solve<K - 1> of pxl_polyfilter.h, word for word: LDL^T without pivoting in the caller's mode order, pivot i
// accepted when D_i > rcond_min * G_ii, truncated at the first rejected pivot; n_used = the accepted leading modes, c_i = +0.0
// from n_used on.  Every lane of a column solves redundantly, in registers.
//
// THE SECOND PASS, over every detector of the group, live or not, by the same phases:  f = c_0 * F_r0, then f = f + c_k * F_rk for
// k = 1 .. K - 1 in order, and out[r,t] = d[r,t] - f.  With n_used = 0 out = d, the bits copied (and not written when out is d).
//
// The detectors before the first group and from the end of the last on are two more items per tile that skip the first pass:
// their sums stay +0.0, pivot 0 is rejected (0 > 0 fails), and the second pass copies them.  A tile that runs past n_t masks its
// lanes the same way.  So every lane runs the same code and no barrier or shuffle is divergent.  out may be exactly d: an
// element is read and written by the same lane, and the barrier of the join stands between a block's first-pass reads and its
// writes.  amps (n_grp, K, n_t) and n_used (n_grp, n_t) are written by phase 0.

template <int K>
__global__ __launch_bounds__(256) void k_modefilter(int64_t n_det, int64_t n_t, int64_t n_grp, int64_t n_tiles, const int64_t* __restrict__ grp_start,
                                                    const double* __restrict__ modes, double rmin, int C, const double* d,
                                                    const double* __restrict__ wfit, double* out, double* __restrict__ amps,
                                                    int64_t* __restrict__ n_used) {
    constexpr int NP = PolyFit<K - 1>::NP, NG = PolyFit<K - 1>::NG, NV = NG + NP;
    constexpr int CH = NV < 11 ? NV : 11;                                   // sums that cross the wavefronts together
    constexpr int UNR = K <= 4 ? 4 : 2;                                     // rows whose loads are issued together
    __shared__ double part[4][CH][64];
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int R = 256 / C;
    const int p = threadIdx.x / C;
    // an item: (0, tile) the detectors before the first group, (g + 1, tile) group g, (n_grp + 1, tile) the rest
    const int64_t sp = (int64_t)blockIdx.x / n_tiles;
    const int64_t t = ((int64_t)blockIdx.x - sp * n_tiles) * C + (threadIdx.x & (C - 1));
    const bool col = t < n_t;
    const bool fit = sp >= 1 && sp <= n_grp;
    int64_t lo = sp == 0 ? 0 : grp_start[sp - 1];
    int64_t hi = sp == n_grp + 1 ? n_det : grp_start[sp];
    lo = lo < 0 ? 0 : lo > n_det ? n_det : lo;
    hi = hi < lo ? lo : hi > n_det ? n_det : hi;

    double v[NV];                                                           // G_ik at poly_idx(i, k), then b_i
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0;
    if (fit && col) {
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
                for (int i = 0; i < K; ++i) {
                    const double wf = wv[u] * F[i];
#pragma unroll
                    for (int k = 0; k <= i; ++k) v[poly_idx(i, k)] = v[poly_idx(i, k)] + wf * F[k];
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
    // C = 16: the levels that stay inside a wavefront
    for (int off = 32; off >= C; off >>= 1) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = v[i] + __shfl_xor(v[i], off, 64);
    }
    double g[NG], b[NP], c[NP];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = v[i];
#pragma unroll
    for (int i = 0; i < NP; ++i) b[i] = v[NG + i];
    const int nu = poly_solve<K - 1>(g, b, rmin, c);
    if (fit && col && p == 0) {
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
            const double* F = modes + r * K;
            double f = c[0] * F[0];
#pragma unroll
            for (int k = 1; k < K; ++k) f = f + c[k] * F[k];
            out[r * n_t + t] = dv[u] - f;
        }
    }
}
