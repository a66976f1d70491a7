// pxl_scatter.h -- the transpose of the scattered bilinear sampler: scatter-add values at sky points into a CAR map;
// included by pxl_kernels.hip after pxl_sample.h (one translation unit, -ffp-contract=off).
#pragma once

// ---- scatter-add: dst[c][j_b][i_a] += (wy_b * wx_a) * vals[c][k] over the 2x2 cell of point k.
// The cell, the fractions, the seam rule and the window rule are k_sample_bilinear's: both call cell2 (pxl_taps.h), so a tap the
// sampler reads as 0 is a tap that is dropped here and <P m, d> = <m, P^T d> holds at rounding level.  A point past the end of
// the batch, or one whose position is not finite (the sampler returns NaN there), has no taps.
// The adds are scatter_add's no-return FP64 atomics.  A lane carries PXL_SUNR points per trip like the sampler (Trip: DESIGN.md 4.2);
// all of a trip's values are loaded before its first add.
__global__ __launch_bounds__(256) void k_scatter_bilinear(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                          int32_t nc, int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                          const double2* __restrict__ sky, const double* __restrict__ vals) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_SUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_SUNR];
        // spelled out: through trip.load this kernel numbers two more SGPRs (100 for 98)
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) ad[u] = (trip.k(u) < n) ? sky[trip.k(u)] : make_double2(0.0, 0.0);
        Cell2 cell[PXL_SUNR];
        Weights2 w[PXL_SUNR];
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            cell[u] = cell2<true>(s, ad[u], nx, ny, row0, nrows, periodic, trip.k(u) < n);
            w[u] = weights2(cell[u].fx, cell[u].fy);
        }
        for (int c = 0; c < nc; ++c) {
            double* pl = dst + (int64_t)c * plane;
            double v[PXL_SUNR];
            trip.load(vals + (int64_t)c * n, n, v, 0.0);
#pragma unroll
            for (int u = 0; u < PXL_SUNR; ++u) scatter2(pl, cell[u], w[u], v[u]);
        }
    }
}
