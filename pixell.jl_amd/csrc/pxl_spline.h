// pxl_spline.h -- cubic B-spline (order 3) interpolation of CAR maps: the prefilter, the separable CAR->CAR evaluation and the
// scattered sampler; included by pxl_kernels.hip (one translation unit, -ffp-contract=off).
#pragma once

// The index rule (spline_fold), the tap weights (spline_weights) and the domain rule (spline_in_domain) are pxl_taps.h's.

// ------------------------------------------------------------------------------------------------
// Prefilter.  (c[i-1] + 4 c[i] + c[i+1]) / 6 = m[i] factors into a causal and an anti-causal first-order recursion with the
// pole z = sqrt(3) - 2:  p[k] = m[k] + z p[k-1];  q[k] = z (q[k+1] - p[k]);  c = 6 q.  |z|^32 = 5e-19, so a recursion started
// from zero PXL_SPL_WARM samples early equals the full-length one to well below Float64 rounding: no look-back between
// blocks.  The warm-up samples are those of the map extended by the boundary rule (spline_fold), of which the bounded
// system's solution is the restriction.
//
// One kernel for both axes.  A workgroup takes PXL_SPL_LINES lines (rows when filtering along RA, columns along DEC) by
// PXL_SPL_SEG positions plus the warm-up on each side into LDS; a lane owns one line and PXL_SPL_SUB consecutive outputs:
// 32 warm-up steps, 16 + 32 causal values kept in registers, the anti-causal sweep over them, 16 outputs.  Every output is
// computed by one lane from the tile alone, so the result does not depend on how blocks are scheduled.
// LDS pitch = 321 doubles (odd, = 1 mod 32): the 32 lanes of a half wave (16 lines x 2 sub-segments 16 apart) hit 32 banks.
//
// TRANS selects the TRANSPOSED system.  On a cyclic axis the system matrix B is symmetric and nothing
// changes.  On a mirrored axis B[1,2] = B[n,n-1] = 2/6 against B[2,1] = B[n-1,n] = 1/6, and with D = diag(1/2, 1, .., 1, 1/2)
// D B is symmetric, so B^-T = D B^-1 D^-1: a sample whose folded position is 1 or n is doubled as it enters the tile (the
// warm-up included: it sees the mirror extension of the scaled input), the same recursion runs, and outputs 1 and n are
// halved as they leave.  Both scalings are exact.  The test is on the position: an interior tile never holds
// position 1 and holds position n only as its last warm-up sample (n = 544 + 256 j).
// TRANS = false compiles to the code it was before the parameter existed.
// ------------------------------------------------------------------------------------------------
#define PXL_SPL_WARM   32      // smallest multiple of 8 with |z|^W < 2^-60
#define PXL_SPL_SUB    16      // outputs per lane
#define PXL_SPL_NSUB   16      // sub-segments per line
#define PXL_SPL_SEG    (PXL_SPL_SUB * PXL_SPL_NSUB)            // 256 outputs per line per tile
#define PXL_SPL_LINES  16
#define PXL_SPL_SPAN   (PXL_SPL_SEG + 2 * PXL_SPL_WARM)        // 320 positions staged per line
#define PXL_SPL_PITCH  (PXL_SPL_SPAN + 1)
#define PXL_SPL_POLE   (-0.26794919243112270647)               // sqrt(3) - 2

template <bool ALONG_X, bool TRANS>
__global__ __launch_bounds__(256) void k_spline_prefilter(const double* __restrict__ src, double* __restrict__ dst,
                                                          int64_t nx, int64_t ny, int periodic, int64_t ntf) {
    __shared__ double tile[PXL_SPL_LINES * PXL_SPL_PITCH];
    const int64_t n = ALONG_X ? nx : ny;              // length of the filtered axis
    const int64_t no = ALONG_X ? ny : nx;             // number of lines
    const int per = ALONG_X ? periodic : 0;
    const int64_t tf = (int64_t)blockIdx.x % ntf, to = (int64_t)blockIdx.x / ntf;
    const int64_t a = tf * PXL_SPL_SEG + 1 - PXL_SPL_WARM;     // 1-based position of tile index 0
    const int64_t o0 = to * PXL_SPL_LINES;                     // 0-based first line
    const bool interior = a >= 1 && a + PXL_SPL_SPAN - 1 <= n;
    const int64_t poff = (int64_t)blockIdx.y * nx * ny;
    src += poff; dst += poff;
    const int tid = threadIdx.x;

    for (int e = tid; e < PXL_SPL_LINES * PXL_SPL_SPAN; e += 256) {
        // the contiguous (RA) index runs fastest over the lanes
        const int l = ALONG_X ? e / PXL_SPL_SPAN : e % PXL_SPL_LINES;
        const int k = ALONG_X ? e % PXL_SPL_SPAN : e / PXL_SPL_LINES;
        double v = 0.0;
        if (o0 + l < no) {
            const int64_t t = interior ? a + k : spline_fold(a + k, n, per);
            v = ALONG_X ? src[(o0 + l) * nx + (t - 1)] : src[(t - 1) * nx + (o0 + l)];
            if (TRANS && !per && (t == 1 || t == n)) v = 2.0 * v;
        }
        tile[l * PXL_SPL_PITCH + k] = v;
    }
    __syncthreads();

    const int l = tid % PXL_SPL_LINES, q = tid / PXL_SPL_LINES;
    const double* base = &tile[l * PXL_SPL_PITCH + q * PXL_SPL_SUB];
    const double z = PXL_SPL_POLE;
    double p = 0.0;
#pragma unroll 8
    for (int k = 0; k < PXL_SPL_WARM; ++k) p = base[k] + z * p;
    double c[PXL_SPL_SUB + PXL_SPL_WARM];
#pragma unroll
    for (int k = 0; k < PXL_SPL_SUB + PXL_SPL_WARM; ++k) { p = base[PXL_SPL_WARM + k] + z * p; c[k] = p; }
    double qv = 0.0;
#pragma unroll
    for (int k = PXL_SPL_SUB + PXL_SPL_WARM - 1; k >= 0; --k) { qv = z * (qv - c[k]); c[k] = qv; }
    __syncthreads();                                  // every lane has read its warm-up before outputs replace the inputs
#pragma unroll
    // + 0.0: a zero result leaves as +0.0.  z < 0, so over a span of +0.0 inputs the sweep gives z * (+0.0 - +0.0) = -0.0, then
    // z * (-0.0 - +0.0) = +0.0, alternating; x + 0.0 is x for every other x (NaN and Inf included), so no value changes.
    for (int k = 0; k < PXL_SPL_SUB; ++k) tile[l * PXL_SPL_PITCH + PXL_SPL_WARM + q * PXL_SPL_SUB + k] = 6.0 * c[k] + 0.0;
    __syncthreads();

    for (int e = tid; e < PXL_SPL_LINES * PXL_SPL_SEG; e += 256) {
        const int l2 = ALONG_X ? e / PXL_SPL_SEG : e % PXL_SPL_LINES;
        const int k = ALONG_X ? e % PXL_SPL_SEG : e / PXL_SPL_LINES;
        const int64_t t = a + PXL_SPL_WARM + k;                // 1-based output position, >= 1
        if (o0 + l2 < no && t <= n) {
            double v = tile[l2 * PXL_SPL_PITCH + PXL_SPL_WARM + k];
            if (TRANS && !per && (t == 1 || t == n)) v = 0.5 * v;
            if (ALONG_X) dst[(o0 + l2) * nx + (t - 1)] = v; else dst[(t - 1) * nx + (o0 + l2)] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Evaluation.
// ------------------------------------------------------------------------------------------------
// CAR -> CAR, separable: a lane owns an output column (four weights and four folded source columns, once), a block walks
// PXL_SPL_TH output rows.  For every source row a lane forms the RA sum h = sum_a wx_a c[i_a, j] once and keeps the four
// sums of the current window in registers; output rows that share source rows (all of them when refining) reuse them.
// Neighbouring lanes read neighbouring or equal source columns, so a source row is fetched once per block; only the
// three window rows at a strip's start are read twice (by the strip above).
#define PXL_SPL_TH 32
struct SplineReproj {
    const double* coeffs; double* dst;
    const int32_t* xi0; const double* xfx; const int32_t* yj0; const double* yfy;
    int64_t nx, ny, nxo, nyo;
    int32_t periodic;
};
__global__ __launch_bounds__(256) void k_reproject_cubic(SplineReproj p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // 0-based output column
    const int64_t r0 = (int64_t)blockIdx.y * PXL_SPL_TH;
    const bool lane_on = i < p.nxo;
    const double* plane = p.coeffs + (int64_t)blockIdx.z * p.nx * p.ny;
    double* dplane = p.dst + (int64_t)blockIdx.z * p.nxo * p.nyo;
    double wx[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t col[4] = {0, 0, 0, 0};
    bool x_in = false;
    if (lane_on) {
        const int64_t i0 = p.xi0[i];
        const double fx = p.xfx[i];
        x_in = p.periodic || spline_in_domain(i0, fx, p.nx);
        spline_weights(fx, wx);
        if (x_in)
            for (int a = 0; a < 4; ++a) col[a] = spline_fold(i0 - 1 + a, p.nx, p.periodic) - 1;
    }
    double h[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t hbase = 0; bool hvalid = false;                             // h[b] belongs to the (unfolded) source row hbase + b
    const int64_t r1 = r0 + PXL_SPL_TH < p.nyo ? r0 + PXL_SPL_TH : p.nyo;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t j0 = p.yj0[r];
        const double fy = p.yfy[r];
        const bool y_in = spline_in_domain(j0, fy, p.ny);               // uniform over the block
        double v = 0.0;
        if (y_in) {
            const int64_t nb = j0 - 1;
            double hn[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t d = nb + b - hbase;
                if (hvalid && d >= 0 && d < 4) {
                    hn[b] = d == 0 ? h[0] : (d == 1 ? h[1] : (d == 2 ? h[2] : h[3]));
                } else {
                    double s = 0.0;
                    if (x_in) {
                        const double* row = plane + (spline_fold(nb + b, p.ny, 0) - 1) * p.nx;
                        s = ((wx[0] * row[col[0]] + wx[1] * row[col[1]]) + wx[2] * row[col[2]]) + wx[3] * row[col[3]];
                    }
                    hn[b] = s;
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) h[b] = hn[b];
            hbase = nb; hvalid = true;
            double wy[4];
            spline_weights(fy, wy);
            if (x_in) v = ((wy[0] * h[0] + wy[1] * h[1]) + wy[2] * h[2]) + wy[3] * h[3];
        }
        if (lane_on) dplane[r * p.nxo + i] = v;
    }
}

// Scattered points: sky2pix!(safe=true) in the reciprocal form, as k_sample_bilinear, then sixteen taps (cell4, gather4 and
// blend4 of pxl_taps.h), plane by plane.  A position that is not finite gives NaN, as the bilinear sampler does; one outside
// the domain gives 0.
__global__ __launch_bounds__(256) void k_sample_cubic(Sky2Pix s, const double* __restrict__ coeffs, int64_t nx, int64_t ny,
                                                      int32_t nc, int periodic, int64_t n, const double2* __restrict__ sky,
                                                      double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const Cell4<int64_t> cell = cell4<int64_t>(s, sky[k], nx, ny, periodic, true);
        for (int c = 0; c < nc; ++c) {
            double v = cell.fin ? 0.0 : __builtin_nan("");
            if (cell.in) {
                double t[4][4];
                gather4(coeffs + (int64_t)c * nx * ny, cell, t);
                v = blend4(cell, t);
            }
            out[(int64_t)c * n + k] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Scatter-add, the transpose E^T of k_sample_cubic's evaluation:
//   dst[c][row_b][col_a] += (wy[b] * wx[a]) * vals[c][k]   over the 4 x 4 taps of point k.
// Position, cell, fractions, domain rule, weights and folded taps are k_sample_cubic's: both call cell4, so the cells are the
// sampler's bit for bit.  A point that is past the batch, not finite or outside the domain adds nothing (the sampler gives
// NaN or 0 there); the adds are scatter4's.
// A lane carries PXL_CUNR points per trip (Trip: DESIGN.md 4.2) and keeps wx[4], wy[4], col[4], row[4] of each (the sixteen products are formed
// at the add: sixteen offsets and sixteen weights per point would not fit beside a second point); all of a trip's values
// are loaded before its first add.  Columns are int32 (spline_shape_check: an axis has at most 4e8 pixels).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scatter_cubic(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny, int32_t nc,
                                                       int periodic, int64_t n, const double2* __restrict__ sky,
                                                       const double* __restrict__ vals) {
    const int64_t plane = nx * ny;
    for (Trip<PXL_CUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_CUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        Cell4<int32_t> cell[PXL_CUNR];
#pragma unroll
        for (int u = 0; u < PXL_CUNR; ++u) cell[u] = cell4<int32_t>(s, ad[u], nx, ny, periodic, trip.k(u) < n);
        for (int c = 0; c < nc; ++c) {
            double* pl = dst + (int64_t)c * plane;
            double v[PXL_CUNR];
            trip.load(vals + (int64_t)c * n, n, v, 0.0);
#pragma unroll
            for (int u = 0; u < PXL_CUNR; ++u)
                if (cell[u].in) scatter4(pl, cell[u], v[u]);
        }
    }
}
