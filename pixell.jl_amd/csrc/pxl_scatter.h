// pxl_scatter.h -- the transpose of the scattered bilinear sampler: scatter-add values at sky points into a CAR map;
// included by pxl_kernels.hip after pxl_sample.h (one translation unit, -ffp-contract=off).
#pragma once

// ---- scatter-add: dst[c][j_b][i_a] += (wy_b * wx_a) * vals[c][k] over the 2x2 cell of point k.
// The cell, the fractions, the seam rule and the window rule are k_sample_bilinear's, from the same helpers (s2p_x / s2p_y
// in the reciprocal form with safe = 1, split_cell, wrap_col): a tap the sampler reads as 0 is a tap that is dropped here,
// so <P m, d> = <m, P^T d> holds at rounding level.  A point whose position is not finite adds nothing.
// The adds are no-return agent-scope FP64 atomics (one global_atomic_add_f64 each, executed at the memory side): the order
// of the additions into one pixel is whatever order they arrive in.  A lane carries PXL_SUNR points per trip like the
// sampler; all of a trip's values are loaded before its first add.
__device__ inline void scatter_add(double* p, double x) {
    __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the no-return form
}
__global__ __launch_bounds__(256) void k_scatter_bilinear(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                          int32_t nc, int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                          const double2* __restrict__ sky, const double* __restrict__ vals) {
    const int64_t chunk = (int64_t)blockDim.x * PXL_SUNR;
    const int64_t plane = nx * nrows;
    for (int64_t k0 = (int64_t)blockIdx.x * chunk + threadIdx.x; k0 < n; k0 += (int64_t)gridDim.x * chunk) {
        double2 ad[PXL_SUNR];
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            int64_t k = k0 + u * blockDim.x;
            ad[u] = (k < n) ? sky[k] : make_double2(0.0, 0.0);
        }
        int64_t o00[PXL_SUNR], o10[PXL_SUNR], o01[PXL_SUNR], o11[PXL_SUNR];   // element offsets, -1 = dropped tap
        double w00[PXL_SUNR], w10[PXL_SUNR], w01[PXL_SUNR], w11[PXL_SUNR];   // wy_b * wx_a
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            double x = s2p_x(s, ad[u].x), y = s2p_y(s, ad[u].y);
            // a point past the end of the batch, or one whose position is not finite (the sampler returns NaN there), has no taps
            const bool live = (k0 + u * blockDim.x < n) && isfinite(x) && isfinite(y);
            int32_t i0, j0;
            double fx, fy;
            split_cell(x, &i0, &fx);
            split_cell(y, &j0, &fy);
            int64_t ia = i0, ib = (int64_t)i0 + 1;
            bool oka = live, okb = live;
            if (periodic) { ia = wrap_col(ia, nx); ib = wrap_col(ib, nx); }
            else { oka = oka && (ia >= 1 && ia <= nx); okb = okb && (ib >= 1 && ib <= nx); }
            int64_t ja = (int64_t)j0 - 1 - row0, jb = ja + 1;                    // resident row indices
            bool rowa = (j0 >= 1 && j0 <= ny && ja >= 0 && ja < nrows);
            bool rowb = ((int64_t)j0 + 1 >= 1 && (int64_t)j0 + 1 <= ny && jb >= 0 && jb < nrows);
            o00[u] = (rowa && oka) ? ja * nx + (ia - 1) : -1;
            o10[u] = (rowa && okb) ? ja * nx + (ib - 1) : -1;
            o01[u] = (rowb && oka) ? jb * nx + (ia - 1) : -1;
            o11[u] = (rowb && okb) ? jb * nx + (ib - 1) : -1;
            w00[u] = (1 - fy) * (1 - fx); w10[u] = (1 - fy) * fx;
            w01[u] = fy * (1 - fx);       w11[u] = fy * fx;
        }
        for (int c = 0; c < nc; ++c) {
            double* pl = dst + (int64_t)c * plane;
            double v[PXL_SUNR];
#pragma unroll
            for (int u = 0; u < PXL_SUNR; ++u) {
                int64_t k = k0 + u * blockDim.x;
                v[u] = (k < n) ? vals[(int64_t)c * n + k] : 0.0;
            }
            // every tap that is on the map takes its add, zero weights included: a NaN or Inf value reaches all four
#pragma unroll
            for (int u = 0; u < PXL_SUNR; ++u) {
                if (o00[u] >= 0) scatter_add(pl + o00[u], w00[u] * v[u]);
                if (o10[u] >= 0) scatter_add(pl + o10[u], w10[u] * v[u]);
                if (o01[u] >= 0) scatter_add(pl + o01[u], w01[u] * v[u]);
                if (o11[u] >= 0) scatter_add(pl + o11[u], w11[u] * v[u]);
            }
        }
    }
}
