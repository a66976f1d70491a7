// pxl_nearest.h -- nearest-pixel (order 0) pointing on a CAR map: the sampler, its transpose, their
// polarised forms and the one-pass binned IQU accumulation; included by pxl_kernels.hip after pxl_pol.h (one translation
// unit, -ffp-contract=off).
//
// Every kernel here calls cell0 (pxl_taps.h): the position is the order-1 position bit for bit and the pixel is the one whose
// [i - 0.5, i + 0.5) holds it, so a point the sampler reads as +0.0 is a point the transposes drop.  With one pixel per point
// P^T W P is exactly the per-pixel 3 x 3 blocks: k_bin_pol_nearest accumulates them and P^T W d in one pass, and there is no
// normal-operator kernel for this order.  A lane carries PXL_ZUNR points per trip (Trip: DESIGN.md 4.2); all of a trip's loads are issued
// before its first add or store; the map is written only through scatter_add.
#pragma once

// ---- forward: out[c][k] = the pixel's value unchanged (value0: +0.0 off the map, NaN where the position is not finite)
__global__ __launch_bounds__(256) void k_sample_nearest(Sky2Pix s, const double* __restrict__ src, int64_t nx, int64_t ny, int32_t nc,
                                                        int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                        const double2* __restrict__ sky, double* __restrict__ out) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_ZUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_ZUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        Cell0 cell[PXL_ZUNR];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) cell[u] = cell0<false>(s, ad[u], nx, ny, row0, nrows, periodic, true);
        for (int c = 0; c < nc; ++c) {
            const double* pl = src + (int64_t)c * plane;
            double v[PXL_ZUNR];
#pragma unroll
            for (int u = 0; u < PXL_ZUNR; ++u) v[u] = load0(pl, cell[u], sky);
#pragma unroll
            for (int u = 0; u < PXL_ZUNR; ++u)
                if (trip.k(u) < n) out[(int64_t)c * n + trip.k(u)] = value0(cell[u], v[u]);
        }
    }
}

// ---- forward, polarised: out[k] = (s_I + q_k * s_Q) + u_k * s_U of those per-plane values: k_sample_pol_bilinear's combination
__global__ __launch_bounds__(256) void k_sample_pol_nearest(Sky2Pix s, const double* __restrict__ src, int64_t nx, int64_t ny,
                                                            int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                            const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                            double* __restrict__ out) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_ZUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_ZUNR], qu[PXL_ZUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        Cell0 cell[PXL_ZUNR];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) cell[u] = cell0<false>(s, ad[u], nx, ny, row0, nrows, periodic, true);
        double v[PXL_ZUNR][3];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[u][c] = load0(src + (int64_t)c * plane, cell[u], sky);
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) {
            double sc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) sc[c] = value0(cell[u], v[u][c]);
            if (trip.k(u) < n) out[trip.k(u)] = (sc[0] + qu[u].x * sc[1]) + qu[u].y * sc[2];
        }
    }
}

// ---- transpose: dst[c][pixel of point k] += vals[c][k], the value itself with no product; nothing where the offset is -1
__global__ __launch_bounds__(256) void k_scatter_nearest(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny, int32_t nc,
                                                         int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                         const double2* __restrict__ sky, const double* __restrict__ vals) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_ZUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_ZUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        Cell0 cell[PXL_ZUNR];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) cell[u] = cell0<true>(s, ad[u], nx, ny, row0, nrows, periodic, trip.k(u) < n);
        for (int c = 0; c < nc; ++c) {
            double* pl = dst + (int64_t)c * plane;
            double v[PXL_ZUNR];
            trip.load(vals + (int64_t)c * n, n, v, 0.0);
#pragma unroll
            for (int u = 0; u < PXL_ZUNR; ++u)
                if (cell[u].off >= 0) scatter_add(pl + cell[u].off, v[u]);
        }
    }
}

// ---- transpose, polarised: plane c takes t_c, t = pol_terms<NP>(vals[k], (q_k, u_k)): NP = 3 planes I Q U for the signal,
// NP = 6 planes II IQ IU QQ QU UU for the weights
template <int NP>
__global__ __launch_bounds__(256) void k_scatter_pol_nearest(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                             int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                             const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                             const double* __restrict__ vals) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_ZUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_ZUNR], qu[PXL_ZUNR];
        double v[PXL_ZUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        trip.load(vals, n, v, 0.0);
        Cell0 cell[PXL_ZUNR];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) cell[u] = cell0<true>(s, ad[u], nx, ny, row0, nrows, periodic, trip.k(u) < n);
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) {
            if (cell[u].off < 0) continue;
            double t[NP];
            pol_terms<NP>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < NP; ++c) scatter_add(dst + (int64_t)c * plane + cell[u].off, t[c]);
        }
    }
}

// ---- the fused map-making pass: rhs3 += P^T (w d) and weights6 += the six planes of P^T W P, nine adds per point.  v = w[k] * d[k]
// with one rounding, then what k_scatter_pol_nearest<3> adds for v and what k_scatter_pol_nearest<6> adds for w[k]: the same
// multiset of terms as that composition, bit for bit.  The cell is formed once and the N-length w * d never exists.  Lanes
// that hit one pixel are NOT pre-summed: that would change the multiset.  Full maps only (row0 = 0, nrows = ny).
__global__ __launch_bounds__(256) void k_bin_pol_nearest(Sky2Pix s, double* __restrict__ rhs3, double* __restrict__ weights6,
                                                         int64_t nx, int64_t ny, int periodic, int64_t n,
                                                         const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                         const double* __restrict__ d, const double* __restrict__ w) {
    const int64_t plane = nx * ny;
    for (Trip<PXL_ZUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_ZUNR], qu[PXL_ZUNR];
        double dk[PXL_ZUNR], wk[PXL_ZUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        trip.load(d, n, dk, 0.0);
        trip.load(w, n, wk, 0.0);
        Cell0 cell[PXL_ZUNR];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) cell[u] = cell0<true>(s, ad[u], nx, ny, 0, ny, periodic, trip.k(u) < n);
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) {
            if (cell[u].off < 0) continue;
            const double v = wk[u] * dk[u];
            double t[3], t6[6];
            pol_terms<3>(v, qu[u], t);
            pol_terms<6>(wk[u], qu[u], t6);
#pragma unroll
            for (int c = 0; c < 3; ++c) scatter_add(rhs3 + (int64_t)c * plane + cell[u].off, t[c]);
#pragma unroll
            for (int c = 0; c < 6; ++c) scatter_add(weights6 + (int64_t)c * plane + cell[u].off, t6[c]);
        }
    }
}
