// pxl_binfilter.h -- the binned-template filter of a (D, T) timestream: for every detector and every bin of a plan
// shared by all detectors -- the samples t = order[j], j in [bin_start[b], bin_start[b+1]) -- the weighted mean of the samples with
// wfit > 0 is subtracted from ALL samples of the bin: scan-synchronous signal (ground pickup binned in azimuth, a half-wave plate's
// in its angle).  It is Fit<1> with the basis B_0 = 1: the items, the live-sample rule, the moments, the tree rule, the solve and
// the second pass are pxl_fit.h's, stated there, with n_axis = n_t POSITIONS of `order`; this header holds who sums what, and the
// gather.  Included by pxl_kernels.hip after pxl_fit.h.
//
// THE GATHER.  An item is not contiguous in memory: position j of it is the sample order[lo + j] of its detector's row.  A position
// whose sample lies outside [0, n_t) is skipped in both passes, neither read nor written, so the kernel stays inside its buffers
// for any contents of order and bin_start; where order repeats a sample, that sample's value is unspecified.  A valid plan is a
// stable sort of the samples by bin, so an item's samples run forward in time, and where the scan stays in a bin for several
// samples neighbouring lanes read neighbouring addresses.
//
// OWNERSHIP is k_polyfilter<0>'s.  One group of G lanes (G a power of two, 1 to 64, or 256, chosen by the host as
// polyfilter_group(n_t, n_bin, 0)) owns one (detector, item).  Lane l adds the terms of the live positions j = l, l + G, l + 2G, ...
// in that order into its two sums, four positions' loads issued together (an index, then a weight and a sample behind it: the
// gather is two dependent loads deep; two or eight in flight measured the same to the 5 % between two runs).  The tree runs
// off = G/2, ..., 1 (capped at 32) within a wavefront; for G = 256 the four wavefronts' sums go through LDS and every lane forms
// (s0 + s1) + (s2 + s3).  In place, the wavefront runs in step between an item's first-pass reads and its writes; for G = 256 the
// barrier of the LDS join stands between.
//
// THE ORDER OF THE ITEMS IS DETECTOR-MAJOR, k_polyfilter's: item = det * (n_bin + 2) + sp, so the blocks that are resident
// together work on the bins of a few detector rows.  A sweep leaves a bin after a few samples, so most 64-byte sectors of a row
// hold samples of two or three bins: the blocks that want the same sector then run at the same time and the later ones find it on
// chip.  The hardware deals consecutive blocks round-robin over the 8 XCDs, whose L2s do not share; the kernel therefore gives
// XCD x the x-th eighth of the items in order, so that the bins of one row meet in one L2 (1.10 -> 0.99 ms out of place and
// 1.09 -> 0.90 in place at 5 samples per bin and sweep, nothing at 10 and 40).  That is a choice of speed alone: every item is
// still taken by exactly one block, whichever XCD runs it.  In bin-major order (item = sp * n_det + det) neighbouring blocks
// share their bin's slice of `order` instead, but the other bins' samples of every sector they fetch are wanted only much later
// in the launch, when the sector has left the caches: measured slower, 1.67 against 1.09 ms at 5 samples per bin and sweep,
// 1.01 against 0.79 at 10, the same at 40.  `order` is not staged: it is 8 bytes per sample against the 24 of
// the row, read once per pass by one lane, and shared by all detectors it stays in the caches.

__global__ __launch_bounds__(256) void k_binfilter(unsigned block0, int64_t n_det, int64_t n_t, int64_t n_bin, int64_t n_items,
                                                   const int64_t* __restrict__ bin_start, const int64_t* __restrict__ order, int G,
                                                   const double* d, const double* __restrict__ wfit, double* out,
                                                   double* __restrict__ means, int64_t* __restrict__ n_used) {
    constexpr int NP = 1, NG = Fit<NP>::NG, U = 4;
    __shared__ double wave_sum[4][NG + NP];
    const int lane = threadIdx.x & (G - 1);
    const unsigned xcd = blockIdx.x % 8, per = gridDim.x / 8, rest = gridDim.x % 8;                 // blocks are dealt round-robin over the 8 XCDs:
    const unsigned block = xcd * per + (xcd < rest ? xcd : rest) + blockIdx.x / 8;                  // XCD x takes the x-th eighth of the items, in order
    const int64_t item = (int64_t)(block0 + block) * (256 / G) + threadIdx.x / G;                    // block0: launch_chunks (pxl_kernels.hip); the deal is per chunk
    const bool has = item < n_items;
    const int64_t det = has ? item / (n_bin + 2) : 0;
    const int64_t sp = has ? item - det * (n_bin + 2) : 0;
    FitSpan span = {0, 0, false};
    if (has) span = fit_span(sp, bin_start, n_bin, n_t);
    const int64_t L = span.hi - span.lo;
    const int64_t* __restrict__ idx = order + span.lo;                      // the item's positions of order
    const int64_t k0 = det * n_t;                                           // the detector's first sample in d, wfit and out

    double g[NG], b[NP];
    g[0] = 0.0;
    b[0] = 0.0;
    if (span.fit) {
        for (int64_t j0 = lane; j0 < L; j0 += U * (int64_t)G) {             // U positions' loads issued together; the order of the sums is j0, j0 + G, ...
            int64_t t[U];
            double wv[U], dv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t j = j0 + (int64_t)u * G;
                t[u] = j < L ? idx[j] : -1;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = (uint64_t)t[u] < (uint64_t)n_t;
                wv[u] = in ? (wfit ? wfit[k0 + t[u]] : 1.0) : 0.0;
                dv[u] = in ? d[k0 + t[u]] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!(wv[u] > 0.0)) continue;
                const double wp = wv[u] * 1.0;                              // pxl_fit.h, THE MOMENTS, with B_0 = 1
                g[0] = g[0] + wp * 1.0;
                b[0] = b[0] + wp * dv[u];
            }
        }
    }
    for (int off = (G < 64 ? G : 64) >> 1; off > 0; off >>= 1) {            // pxl_fit.h, THE TREE: the levels inside a wavefront
        g[0] = g[0] + __shfl_xor(g[0], off, 64);
        b[0] = b[0] + __shfl_xor(b[0], off, 64);
    }
    if (G == 256) {
        const int wv = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            wave_sum[wv][0] = g[0];
            wave_sum[wv][NG] = b[0];
        }
        __syncthreads();
        g[0] = (wave_sum[0][0] + wave_sum[1][0]) + (wave_sum[2][0] + wave_sum[3][0]);
        b[0] = (wave_sum[0][NG] + wave_sum[1][NG]) + (wave_sum[2][NG] + wave_sum[3][NG]);
    }
    double c[NP];
    const int nu = fit_solve<NP>(g, b, 0.0, c);                             // accepted when G_00 > 0 * G_00: a positive, finite sum of weights
    if (span.fit && lane == 0) {
        const int64_t f = det * n_bin + (sp - 1);
        if (n_used) n_used[f] = nu;
        if (means) means[f] = c[0];
    }
    if (nu == 0) {
        if (out != d)
            for (int64_t j = lane; j < L; j += G) {
                const int64_t tj = idx[j];
                if ((uint64_t)tj < (uint64_t)n_t) out[k0 + tj] = d[k0 + tj];
            }
        return;
    }
    const double one[NP] = {1.0};
    const double f = fit_model(c, one);                                     // c_0 * 1.0
    for (int64_t j = lane; j < L; j += G) {
        const int64_t tj = idx[j];
        if ((uint64_t)tj < (uint64_t)n_t) out[k0 + tj] = d[k0 + tj] - f;
    }
}
