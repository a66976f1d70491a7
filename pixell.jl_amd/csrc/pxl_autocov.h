// pxl_autocov.h -- the gappy autocovariance of a (D, T) timestream: per detector and lag k = 0 .. lambda the sum of
// z_t * z_(t+k) over the pairs of live samples of one segment, and the number of those pairs.  The noise estimate that
// ops.noise_psd_from_autocov turns into the spectrum of the Toeplitz weight (pxl_toeplitz.h).  Included by pxl_kernels.hip (one
// translation unit, -ffp-contract=off: every product and every sum below is rounded once, nothing is fused).
//
// THE DEFINITION.  Segments and LIVE are pxl_toeplitz.h's: segment s is [seg_start[s], seg_start[s+1]) with both ends clamped to
// [0, n_t] (fit_span), a sample is live when it lies in a segment and wlive > 0 (a NaN weight is not; a null wlive is live
// everywhere).  z_j = x_j where j is live and +0.0 elsewhere; an x that is not live enters no arithmetic.
//     sums[det][k]  = sum of z_t * z_(t+k) over the t with t and t + k live in the SAME segment,
//     pairs[det][k] = the number of those t, exact;  +0.0 and 0 where there is none.
//
// THE ORDER OF THE SUM, from lambda, n_t and the contents of seg_start alone.  With need = ceil((lambda + 1) / 5),
//     LPG = the smallest power of two >= need, at most 256;   W = 5 LPG;   P = 256 / LPG   (P W = C = PXL_ACOV_C = 1280).
// The sum of one (detector, lag) is split into P PARTIALS.  A segment [lo, hi) is walked in tiles of C samples from lo on; the
// sample lo + u belongs to partial p = (u mod C) / W.  Each partial starts from +0.0 and takes its terms one by one,
//     v_p = v_p + z_t * z_(t+k),
// through the segments in the order of s and through a segment in the order of t, z_(t+k) = +0.0 from hi on.  A term with a +0.0
// factor is +-0.0 for finite data and leaves v_p's bits as they are, so only the pairs of the definition count: the kernel stops a
// lane's walk through a tile at the first multiple of 5 steps past hi - k, and skips what lies wholly beyond.  Then the tree, for
// off = P / 2, P / 4, .. 1 in that order:  v_p = v_p + v_(p + off) for p < off;  sums = v_0.  With lambda >= 640 P is 1: one
// running sum over the whole row, no tree.  Nothing depends on n_det, on the detector or on the grid; no atomics, no scratch.
//
// A non-finite LIVE sample makes lag 0 of its detector non-finite (its square is a term) and may make any other lag of that
// detector non-finite (Inf * +0.0 is a NaN, where its partner is a cut or lies past the segment's end); a block works on one
// detector and writes only its row, so no other detector is touched.
//
// OWNERSHIP.  A block of 256 lanes owns one (detector, group of W consecutive lags from k0); lane l = p LPG + q carries the five
// CONSECUTIVE lags k0 + 5 q + r of partial p in five independent accumulators, which hide the latency of the adds.  Per tile the
// block stages z at [t0, t0 + C) (the left factors) and at [t0 + k0, t0 + k0 + C + W) (the right ones; for k0 = 0 the same array) in
// LDS, cuts and the segment's end applied there, so the product loop has no branch.  A step reads one left factor, shared by the
// LPG lanes of a group, and one new right factor: the five-wide window of right factors slides by one sample per step, two LDS
// reads for five products, neighbouring lanes five doubles apart (an odd stride: no bank conflict for ds_read_b64).
// The liveness of the staged samples is kept as bits, one ballot per wavefront; pairs[k] of a tile is the sum over its 20 words of
// popcount(left word & the right bits shifted by k - k0).  The block's 1280 slots l + 256 m are P parts of W lags: slot part W + j
// counts lag k0 + j over the words part, part + P, ..; at the end the parts of a lag are added through LDS.  Integer sums need no order.
//
// Segments that overlap are each walked: their pairs are counted twice (unspecified by the contract, inside the buffers).

constexpr int PXL_ACOV_C = 1280;

// the lanes of a group, as a power of two, from lambda alone
static inline int autocov_lpg_log2(int64_t lambda) {
    const int64_t need = (lambda + 5) / 5;
    int l = 0;
    while (l < 8 && (1 << l) < need) ++l;
    return l;
}

__global__ __launch_bounds__(256) void k_autocov(unsigned block0, int64_t n_t, int64_t n_seg, int n_grp, const int64_t* __restrict__ seg_start,
                                                 int lambda, int lpg_log2, const double* __restrict__ x, const double* __restrict__ wlive,
                                                 double* __restrict__ sums, int64_t* __restrict__ pairs) {
    constexpr int C = PXL_ACOV_C, R = 5, NW = C / 64;
    __shared__ double zb[2 * C];                                            // z at t0 + k0 + j, j < C + W <= 2 C
    __shared__ double za[C];                                                // z at t0 + i, staged where k0 > 0
    __shared__ unsigned long long mb[2 * NW + 1], ma[NW];                   // the same samples' liveness, 64 to a word
    const int tid = threadIdx.x;
    const int W = R << lpg_log2, P = 256 >> lpg_log2;                       // P W = C
    const int p = tid >> lpg_log2, q = tid & ((1 << lpg_log2) - 1);
    const unsigned bid = block0 + blockIdx.x;                               // block0: launch_chunks in pxl_kernels.hip
    const int64_t det = bid / (unsigned)n_grp;
    const int k0 = (int)(bid - det * (unsigned)n_grp) * W;
    const int kq = k0 + R * q;                                              // the lane's first lag
    const double* __restrict__ xr = x + det * n_t;
    const double* __restrict__ wr = wlive ? wlive + det * n_t : nullptr;
    const int nb = (C + W + 63) & ~63;                                      // whole wavefronts stage, so every ballot is complete

    double acc[R];
    long long cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = 0.0;
        cnt[r] = 0;
    }
    if (tid <= 2 * NW) mb[tid] = 0;
    for (int64_t s = 0; s < n_seg; ++s) {                                   // uniform over the block: the barriers below are reached by all
        const FitSpan sp = fit_span(s + 1, seg_start, n_seg, n_t);          // pxl_fit.h: the polynomial filter's clamp
        for (int64_t t0 = sp.lo; t0 < sp.hi - k0; t0 += C) {
            __syncthreads();                                                // the previous tile has been read
            for (int j = tid; j < nb; j += 256) {
                const int64_t t = t0 + k0 + j;
                double wv = 0.0, xv = 0.0;
                if (j < C + W && t < sp.hi) {                               // inside [0, n_t): the only reads of x and wlive,
                    wv = wr ? wr[t] : 1.0;                                  // both in flight together
                    xv = xr[t];
                }
                const bool lv = wv > 0.0;
                zb[j] = lv ? xv : 0.0;
                const unsigned long long m = __ballot(lv);
                if ((tid & 63) == 0) mb[j >> 6] = m;
            }
            if (k0 > 0)
                for (int j = tid; j < C; j += 256) {
                    const int64_t t = t0 + j;
                    double wv = 0.0, xv = 0.0;
                    if (t < sp.hi) {
                        wv = wr ? wr[t] : 1.0;
                        xv = xr[t];
                    }
                    const bool lv = wv > 0.0;
                    za[j] = lv ? xv : 0.0;
                    const unsigned long long m = __ballot(lv);
                    if ((tid & 63) == 0) ma[j >> 6] = m;
                }
            __syncthreads();
            int64_t v = kq <= lambda ? sp.hi - t0 - kq - (int64_t)p * W : 0;   // the steps of this lane that have a pair
            v = v < 0 ? 0 : v > W ? W : v;
            const int n_i = (int)((v + R - 1) / R) * R;                     // whole rounds of the window: the rest are +-0.0 terms
            const double* a = (k0 > 0 ? za : zb) + p * W;
            const double* b = zb + R * tid;                                 // = p W + 5 q: the lane's lag 5 q at step 0
            double w[R];
#pragma unroll
            for (int r = 0; r < R - 1; ++r) w[r] = b[r];
            for (int i = 0; i < n_i; i += R) {
#pragma unroll
                for (int st = 0; st < R; ++st) {                            // the window's shifts are renamings
                    const double av = a[i + st];
                    w[(st + R - 1) % R] = b[i + st + R - 1];
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] = acc[r] + av * w[(st + r) % R];
                }
            }
            if (pairs) {
                const unsigned long long* am = k0 > 0 ? ma : mb;
#pragma unroll
                for (int m = 0; m < R; ++m) {
                    const int slot = tid + 256 * m, part = slot / W, j = slot - part * W;
                    if (k0 + j <= lambda) {
                        long long n = 0;
#pragma unroll 1
                        for (int wd = part; wd < NW; wd += P) {
                            const int o = 64 * wd + j, ix = o >> 6, sh = o & 63;
                            unsigned long long bits = mb[ix] >> sh;
                            if (sh) bits |= mb[ix + 1] << (64 - sh);
                            n += __popcll(am[wd] & bits);
                        }
                        cnt[m] += n;
                    }
                }
            }
        }
    }
    // THE TREE over the P partials of a lag: the lanes p LPG + q, p = 0 .. P - 1
    if (lpg_log2 < 8) {
        __syncthreads();                                                    // the last tile has been read: zb is free
        for (int off = 128 >> lpg_log2; off >= 1; off >>= 1) {
            if (p >= off && p < 2 * off) {                                  // a level reads [off, 2 off) and the next writes below off
#pragma unroll
                for (int r = 0; r < R; ++r) zb[R * tid + r] = acc[r];
            }
            __syncthreads();
            if (p < off) {
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = acc[r] + zb[R * (tid + (off << lpg_log2)) + r];
            }
        }
    }
    const int64_t row = det * ((int64_t)lambda + 1);
    if (p == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (kq + r <= lambda) sums[row + kq + r] = acc[r];
    }
    if (pairs) {                                                            // uniform over the block
        long long* pc = reinterpret_cast<long long*>(zb);                   // the 1280 slots' counts; integer sums need no order
        __syncthreads();                                                    // the tree has read zb
#pragma unroll
        for (int m = 0; m < R; ++m) pc[tid + 256 * m] = cnt[m];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int j = tid + 256 * m;
            if (j < W && k0 + j <= lambda) {
                long long n = 0;
                for (int part = 0; part < P; ++part) n += pc[part * W + j];
                pairs[row + k0 + j] = n;
            }
        }
    }
}
