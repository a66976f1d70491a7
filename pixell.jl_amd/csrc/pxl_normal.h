// pxl_normal.h -- the normal operator of the polarised map-maker: y += P^T W P x for the order-1 pointing
// matrix of pxl_pol.h and a diagonal W, in one pass; included by pxl_kernels.hip after pxl_pol.h (one translation unit,
// -ffp-contract=off).
//
// Nothing here is new arithmetic.  A lane calls what k_sample_pol_bilinear calls on x (the gated cell, the wide row loads, the
// three lerps, (s_I + q s_Q) + u s_U), multiplies by w[k] with one rounding, and then calls what k_scatter_pol_bilinear<3>
// calls for that value (pol_terms<3>, scatter2) -- the helpers of pxl_taps.h, so the multiset of terms is the composition's,
// bit for bit.  What is new: position, cell, fractions and the four offsets are formed ONCE per point, and the N-length stream
// of samples between the two kernels never exists.  Full maps only: no row window (row0 = 0, nrows = ny).
#pragma once

// A lane carries PXL_NUNR points per trip (Trip: DESIGN.md 4.2); the 6 row loads of each (2 per plane) are issued before the
// trip's first add.
// One point: 93 VGPRs, 5 waves/SIMD.  Two (151 VGPRs, 3 waves) time the same within 0.5 % on random and on raster-ordered
// points, four take all 256 VGPRs (1 wave): DESIGN.md 4.14.
__global__ __launch_bounds__(256) void k_normal_pol_bilinear(Sky2Pix s, const double* __restrict__ x3, double* __restrict__ y3,
                                                             int64_t nx, int64_t ny, int periodic, int64_t n,
                                                             const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                             const double* __restrict__ w) {
    const int64_t plane = nx * ny;
    for (Trip<PXL_NUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_NUNR], qu[PXL_NUNR];
        double wk[PXL_NUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        trip.load(w, n, wk, 0.0);
        // the scatter's gated cell: a point past the batch or whose position is not finite has all four offsets -1, loads
        // nothing from x and adds nothing
        Cell2 cell[PXL_NUNR];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) cell[u] = cell2<true>(s, ad[u], nx, ny, 0, ny, periodic, trip.k(u) < n);
        Taps2 m[PXL_NUNR][3];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u)
#pragma unroll
            for (int c = 0; c < 3; ++c) m[u][c] = gather2_wide(x3 + (int64_t)c * plane, cell[u], sky);
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            if (__builtin_expect(!cell[u].wide, 0)) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gather2_fixup(x3 + (int64_t)c * plane, cell[u], m[u][c]);
            }
        }
        // v = w * ((s_I + q s_Q) + u s_U), the sampler's expressions and one rounding for the weight
        double v[PXL_NUNR];
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            double sc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) sc[c] = lerp2(m[u][c], cell[u].fx, cell[u].fy);
            const double d = (sc[0] + qu[u].x * sc[1]) + qu[u].y * sc[2];
            v[u] = wk[u] * d;
        }
#pragma unroll
        for (int u = 0; u < PXL_NUNR; ++u) {
            const Weights2 wt = weights2(cell[u].fx, cell[u].fy);
            double t[3];
            pol_terms<3>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < 3; ++c) scatter2(y3 + (int64_t)c * plane, cell[u], wt, t[c]);
        }
    }
}
