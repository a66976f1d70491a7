// pxl_normal.h -- the normal operator of the polarised map-maker: y += P^T W P x for the order-1 pointing
// matrix of pxl_pol.h and a diagonal W, in one pass; included by pxl_kernels.hip after pxl_pol.h (one translation unit,
// -ffp-contract=off).
//
// Nothing here is new arithmetic.  A lane restates k_sample_pol_bilinear on x (the wide row loads, the three nested lerps,
// (s_I + q s_Q) + u s_U), multiplies by w[k] with one rounding, and then makes k_scatter_pol_bilinear<3>'s adds for that
// value: the same helpers -- s2p_x / s2p_y in the reciprocal form with safe = 1, split_cell, wrap_col, pol_terms,
// scatter_add -- and the same expressions, so the multiset of terms is the composition's, bit for bit.  What is new:
// position, cell, fractions and the four offsets are formed ONCE per point, and the N-length stream of samples between the
// two kernels never exists.  Full maps only: no row window.
#pragma once

// A lane carries PXL_NUNR points per trip; the 6 row loads of each (2 per plane) are issued before the trip's first add.
// One point: 93 VGPRs, 5 waves/SIMD.  Two (151 VGPRs, 3 waves) time the same within 0.5 % on random and on raster-ordered
// points, four take all 256 VGPRs (1 wave): DESIGN.md 4.14.
#ifndef PXL_NUNR
#define PXL_NUNR 1
#endif
__global__ __launch_bounds__(256) void k_normal_pol_bilinear(Sky2Pix s, const double* __restrict__ x3, double* __restrict__ y3,
                                                             int64_t nx, int64_t ny, int periodic, int64_t n,
                                                             const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                             const double* __restrict__ w) {
    const int64_t chunk = (int64_t)blockDim.x * PXL_NUNR;
    const int64_t plane = nx * ny;
    for (int64_t k0 = (int64_t)blockIdx.x * chunk + threadIdx.x; k0 < n; k0 += (int64_t)gridDim.x * chunk) {
        double2 ad[PXL_NUNR], qu[PXL_NUNR];
        double wk[PXL_NUNR];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            const int64_t k = k0 + u * blockDim.x;
            ad[u] = (k < n) ? sky[k] : make_double2(0.0, 0.0);
            qu[u] = (k < n) ? resp[k] : make_double2(0.0, 0.0);
            wk[u] = (k < n) ? w[k] : 0.0;
        }
        // the scatter's offsets: -1 = a tap the sampler reads as 0 and the scatter drops; all four -1 for a point past the
        // batch or whose position is not finite, which then loads nothing from x and adds nothing
        int64_t o00[PXL_NUNR], o10[PXL_NUNR], o01[PXL_NUNR], o11[PXL_NUNR];
        double fx[PXL_NUNR], fy[PXL_NUNR];
        bool wide[PXL_NUNR];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            const double x = s2p_x(s, ad[u].x), y = s2p_y(s, ad[u].y);
            const bool live = (k0 + u * blockDim.x < n) && isfinite(x) && isfinite(y);
            int32_t i0, j0;
            split_cell(x, &i0, &fx[u]);
            split_cell(y, &j0, &fy[u]);
            int64_t ia = i0, ib = (int64_t)i0 + 1;
            bool oka = live, okb = live;
            if (periodic) { ia = wrap_col(ia, nx); ib = wrap_col(ib, nx); }
            else { oka = oka && (ia >= 1 && ia <= nx); okb = okb && (ib >= 1 && ib <= nx); }
            const int64_t ja = (int64_t)j0 - 1, jb = ja + 1;                      // row indices
            const bool rowa = (j0 >= 1 && j0 <= ny);
            const bool rowb = ((int64_t)j0 + 1 >= 1 && (int64_t)j0 + 1 <= ny);
            o00[u] = (rowa && oka) ? ja * nx + (ia - 1) : -1;
            o10[u] = (rowa && okb) ? ja * nx + (ib - 1) : -1;
            o01[u] = (rowb && oka) ? jb * nx + (ia - 1) : -1;
            o11[u] = (rowb && okb) ? jb * nx + (ib - 1) : -1;
            wide[u] = o00[u] >= 0 && o01[u] >= 0 && o10[u] == o00[u] + 1 && o11[u] == o01[u] + 1;
        }
        // k_sample_pol_bilinear's loads: interior points take one 2-element load per row and plane; the others still issue
        // the loads, from the first coordinate pair of the batch (16 readable bytes whenever n >= 1), and take their taps below
        struct __attribute__((packed, aligned(8))) TT { double a, b; };
        double m00[PXL_NUNR][3], m10[PXL_NUNR][3], m01[PXL_NUNR][3], m11[PXL_NUNR][3];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double* pl = x3 + (int64_t)c * plane;
                const TT ra = *(wide[u] ? reinterpret_cast<const TT*>(pl + o00[u]) : reinterpret_cast<const TT*>(sky));
                const TT rb = *(wide[u] ? reinterpret_cast<const TT*>(pl + o01[u]) : reinterpret_cast<const TT*>(sky));
                m00[u][c] = ra.a; m10[u][c] = ra.b; m01[u][c] = rb.a; m11[u][c] = rb.b;
            }
        }
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            if (__builtin_expect(!wide[u], 0)) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double* pl = x3 + (int64_t)c * plane;
                    m00[u][c] = o00[u] >= 0 ? pl[o00[u]] : 0.0;
                    m10[u][c] = o10[u] >= 0 ? pl[o10[u]] : 0.0;
                    m01[u][c] = o01[u] >= 0 ? pl[o01[u]] : 0.0;
                    m11[u][c] = o11[u] >= 0 ? pl[o11[u]] : 0.0;
                }
            }
        }
        // v = w * ((s_I + q s_Q) + u s_U), the sampler's expressions and one rounding for the weight
        double v[PXL_NUNR];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            double sc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double top = (1 - fx[u]) * m00[u][c] + fx[u] * m10[u][c];
                const double bot = (1 - fx[u]) * m01[u][c] + fx[u] * m11[u][c];
                sc[c] = (1 - fy[u]) * top + fy[u] * bot;
            }
            const double d = (sc[0] + qu[u].x * sc[1]) + qu[u].y * sc[2];
            v[u] = wk[u] * d;
        }
        // k_scatter_pol_bilinear<3>'s adds: every tap that is on the map takes its add in every plane, zero weights included
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            const double w00 = (1 - fy[u]) * (1 - fx[u]), w10 = (1 - fy[u]) * fx[u];
            const double w01 = fy[u] * (1 - fx[u]),       w11 = fy[u] * fx[u];
            double t[3];
            pol_terms<3>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double* pl = y3 + (int64_t)c * plane;
                if (o00[u] >= 0) scatter_add(pl + o00[u], w00 * t[c]);
                if (o10[u] >= 0) scatter_add(pl + o10[u], w10 * t[c]);
                if (o01[u] >= 0) scatter_add(pl + o01[u], w01 * t[c]);
                if (o11[u] >= 0) scatter_add(pl + o11[u], w11 * t[c]);
            }
        }
    }
}
