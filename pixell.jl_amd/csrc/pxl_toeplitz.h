// pxl_toeplitz.h -- the banded-Toeplitz noise weight of a (D, T) timestream: out = G T G x, the time-domain inverse
// noise covariance of a stationary correlated noise process, one symmetric banded Toeplitz block per (detector, segment), zeroed at
// the cut samples ("gappy Toeplitz").  Included by pxl_kernels.hip (one translation unit, -ffp-contract=off: every product and every
// sum below is rounded once, nothing is fused).
//
// THE DEFINITION.  A sample is LIVE when it lies in a segment [seg_start[s], seg_start[s+1]) (both ends clamped to [0, n_t]) and
// wlive > 0 (a NaN weight is not; a null wlive is live everywhere).  z_j = x_j where j is live and +0.0 elsewhere, and +0.0 outside
// the segment of the output at hand: the blocks do not couple segments.  For a live sample t, with c_k = kern[det][k],
//     S = c_0 * z_t;   S = S + c_k * (z_(t-k) + z_(t+k))   for k = 1 .. lambda in that order;   out_t = S.
// Every other sample gets out = +0.0.  The order of the sum belongs to the output alone, not to the tiling: the bits are fixed by the
// arguments.  An x under a cut enters no arithmetic; a non-finite live x reaches the live samples within lambda of it in its segment.
//
// OWNERSHIP.  A block of 256 lanes owns one (detector, tile of PXL_TOEP_C = 1280 consecutive samples); a lane carries five outputs,
// so that the lambda-long dependent chain of one output's adds hides behind the four others.  seg_start lives on the device, so the
// grid cannot follow the segments: the block looks through ALL segments, 256 at a time (one per lane, a ballot per wavefront, the
// four masks through LDS), and makes one PASS for each that meets its tile, in the order of s.  That finds every segment whatever the
// order of seg_start; where segments overlap, the later s wins.  A pass stages z of the tile and lambda samples either side in LDS
// once -- the segment's ends and the cuts are applied there, so the tap loop has no branch -- and every lane runs the whole tap
// loop; an output is kept where its sample is live in that segment.  Each output is written once, at the end: no atomics, no scratch.
//
// WHICH FIVE OUTPUTS.  SLIDE = false (lambda <= 16, where the call is mostly a stream): lane l carries t0 + l + 256 r, its global
// reads and writes are coalesced, and every tap of every output is two LDS reads, consecutive doubles across a wavefront.
// SLIDE = true (lambda > 16, where the taps are most of the time): lane l carries the CONSECUTIVE outputs t0 + 5 l + r and keeps the
// five z to their left and the five to their right in registers; from tap k to k + 1 each window slides by one sample, so a tap of
// all five outputs costs two LDS reads instead of ten and the vector units, not the LDS, set the pace.  Neighbouring lanes then read
// doubles five apart: 10 banks of 64, and an odd stride in doubles is conflict-free for ds_read_b64 -- the reason a lane carries five
// outputs and not four.  Either way an output's sum is the definition's, term by term.
//
// LMAX, the largest lambda an instantiation takes, only sizes the static LDS: (1280 + 2 LMAX) doubles, 12 KiB at 128, 26 KiB at
// 1024 and 74 KiB of the CU's 160 at 4096.  c_k is uniform over the block.

constexpr int PXL_TOEP_C = 1280;

template <int LMAX, bool SLIDE>
__global__ __launch_bounds__(256) void k_toeplitz(unsigned block0, int64_t n_t, int64_t n_seg, int64_t tiles, const int64_t* __restrict__ seg_start, int lambda,
                                                  const double* __restrict__ kern, const double* __restrict__ x,
                                                  const double* __restrict__ wlive, double* __restrict__ out) {
    constexpr int C = PXL_TOEP_C, R = C / 256;
    __shared__ double z[C + 2 * LMAX];
    __shared__ unsigned long long hit[4];
    const int tid = threadIdx.x;
    const unsigned bid = block0 + blockIdx.x;                               // block0: launch_chunks in pxl_kernels.hip
    const int64_t det = bid / tiles;
    const int64_t t0 = (bid - det * tiles) * C;
    const int64_t t1 = t0 + C < n_t ? t0 + C : n_t;
    const double* __restrict__ xr = x + det * n_t;
    const double* __restrict__ wr = wlive ? wlive + det * n_t : nullptr;
    const double* __restrict__ c = kern + det * ((int64_t)lambda + 1);

    double acc[R];
    bool live[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t t = t0 + (SLIDE ? R * tid + r : tid + 256 * r);
        live[r] = t < t1 && (wr ? wr[t] > 0.0 : true);
        acc[r] = 0.0;
    }
    for (int64_t s0 = 0; s0 < n_seg; s0 += 256) {
        const int64_t sl = s0 + tid;
        bool meets = false;
        if (sl < n_seg) {
            const FitSpan sp = fit_span(sl + 1, seg_start, n_seg, n_t);     // pxl_fit.h: the polynomial filter's clamp
            meets = sp.hi > sp.lo && sp.lo < t1 && sp.hi > t0;
        }
        const unsigned long long m = __ballot(meets);
        __syncthreads();                                                    // the previous round's masks have been read
        if ((tid & 63) == 0) hit[tid >> 6] = m;
        __syncthreads();
        for (int wv = 0; wv < 4; ++wv) {
            const unsigned long long hw = hit[wv];
            unsigned long long todo = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(hw >> 32)) << 32) |
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)hw);
            while (todo) {                                                  // uniform over the block: the barriers below are reached by all
                const int64_t s = s0 + 64 * wv + __builtin_ctzll(todo);
                todo &= todo - 1;
                const FitSpan sp = fit_span(s + 1, seg_start, n_seg, n_t);
                __syncthreads();                                            // the previous pass has read z
                for (int i = tid; i < C + 2 * lambda; i += 256) {
                    const int64_t j = t0 - lambda + i;
                    double v = 0.0;
                    if (j >= sp.lo && j < sp.hi) {                          // inside [0, n_t): the only reads of x and wlive
                        const double wv_ = wr ? wr[j] : 1.0;
                        const double xv = xr[j];
                        v = wv_ > 0.0 ? xv : 0.0;
                    }
                    z[i] = v;
                }
                __syncthreads();
                const double c0 = c[0];
                double S[R];
                if constexpr (SLIDE) {
                    const double* zb = z + lambda + R * tid;                // the lane's first output; the others follow it
                    double lw[R], rw[R];                                    // at tap k: lw[r] = z_(t_r - k), rw[r] = z_(t_r + k)
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        lw[r] = rw[r] = zb[r];
                        S[r] = c0 * lw[r];
                    }
#pragma unroll 5
                    for (int k = 1; k <= lambda; ++k) {                     // unrolled by R, the windows' shifts are renamings
                        const double ck = c[k];
#pragma unroll
                        for (int r = R - 1; r > 0; --r) lw[r] = lw[r - 1];
                        lw[0] = zb[-k];
#pragma unroll
                        for (int r = 0; r < R - 1; ++r) rw[r] = rw[r + 1];
                        rw[R - 1] = zb[R - 1 + k];
#pragma unroll
                        for (int r = 0; r < R; ++r) S[r] = S[r] + ck * (lw[r] + rw[r]);
                    }
                } else {
                    const double* zc = z + lambda + tid;                    // the lane's first output; the others 256 r further
#pragma unroll
                    for (int r = 0; r < R; ++r) S[r] = c0 * zc[256 * r];
#pragma unroll 4
                    for (int k = 1; k <= lambda; ++k) {
                        const double ck = c[k];
#pragma unroll
                        for (int r = 0; r < R; ++r) S[r] = S[r] + ck * (zc[256 * r - k] + zc[256 * r + k]);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int64_t t = t0 + (SLIDE ? R * tid + r : tid + 256 * r);
                    if (live[r] && t >= sp.lo && t < sp.hi) acc[r] = S[r];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t t = t0 + (SLIDE ? R * tid + r : tid + 256 * r);
        if (t < t1) out[det * n_t + t] = acc[r];
    }
}
