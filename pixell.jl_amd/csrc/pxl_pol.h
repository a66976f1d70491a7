// pxl_pol.h -- the polarised pointing matrix: d = I + q Q + u U sampled from, and scatter-added into, the
// three planes of an IQU CAR map in one pass; included by pxl_kernels.hip after pxl_spline.h (one translation unit,
// -ffp-contract=off).
//
// Every kernel here calls what its scalar counterpart (k_sample_bilinear, k_sample_cubic, k_scatter_bilinear, k_scatter_cubic)
// calls -- the cells, gathers, blends and adds of pxl_taps.h -- so position, cell, weights, offsets and every per-plane value
// or term are the counterpart's bits.  What is new: position, cell, weights and offsets are formed ONCE per point and reused
// across the planes, the response pair (q, u) is one double2 load beside the coordinates, and the three (or six) per-plane
// streams of the composition never exist.  Q and U are three independent scalar planes: no spin-2 sign flip at the DEC
// mirror or across a pole (NOTES item 7).
#pragma once

// ---- forward, order 1: out[k] = (s_I + q_k * s_Q) + u_k * s_U, s_c what k_sample_bilinear<double> writes for plane c.
// A lane carries PXL_PSUNR points per trip (Trip: DESIGN.md 4.2); the 6 row loads of each (2 per plane) are issued before the first store.
__global__ __launch_bounds__(256) void k_sample_pol_bilinear(Sky2Pix s, const double* __restrict__ src, int64_t nx, int64_t ny,
                                                             int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                             const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                             double* __restrict__ out) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_PSUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_PSUNR], qu[PXL_PSUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        Cell2 cell[PXL_PSUNR];
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) cell[u] = cell2<false>(s, ad[u], nx, ny, row0, nrows, periodic, true);
        Taps2 m[PXL_PSUNR][3];
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u)
#pragma unroll
            for (int c = 0; c < 3; ++c) m[u][c] = gather2_wide(src + (int64_t)c * plane, cell[u], sky);
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
            if (__builtin_expect(!cell[u].wide, 0)) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gather2_fixup(src + (int64_t)c * plane, cell[u], m[u][c]);
            }
        }
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
            double sc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v = lerp2(m[u][c], cell[u].fx, cell[u].fy);
                sc[c] = cell[u].fin ? v : __builtin_nan("");
            }
            if (trip.k(u) < n) out[trip.k(u)] = (sc[0] + qu[u].x * sc[1]) + qu[u].y * sc[2];
        }
    }
}

// ---- forward, order 3: the same combination of k_sample_cubic's per-plane values, on coefficients.  One point per lane
// and trip, as the scalar kernel: the 48 tap loads of a point (16 per plane) are issued before its store.
__global__ __launch_bounds__(256) void k_sample_pol_cubic(Sky2Pix s, const double* __restrict__ coeffs, int64_t nx, int64_t ny,
                                                          int periodic, int64_t n, const double2* __restrict__ sky,
                                                          const double2* __restrict__ resp, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const double2 ad = sky[k], qu = resp[k];
        const Cell4<int64_t> cell = cell4<int64_t>(s, ad, nx, ny, periodic, true);
        double sc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) sc[c] = cell.fin ? 0.0 : __builtin_nan("");
        if (cell.in) {
            double t[3][4][4];
#pragma unroll
            for (int c = 0; c < 3; ++c) gather4(coeffs + (int64_t)c * nx * ny, cell, t[c]);
#pragma unroll
            for (int c = 0; c < 3; ++c) sc[c] = blend4(cell, t[c]);
        }
        out[k] = (sc[0] + qu.x * sc[1]) + qu.y * sc[2];
    }
}

// ---- transpose.  Plane c of dst takes (wy_b * wx_a) * t_c, t = pol_terms<NP>(vals[k], (q_k, u_k)): NP = 3 planes I Q U for
// the signal, NP = 6 planes II IQ IU QQ QU UU for the weights.
// order 1: k_scatter_bilinear's taps, window and live rule; a lane carries PXL_SUNR points per trip like it and all of a
// trip's loads (coordinates, responses, values) are issued before its first add
template <int NP>
__global__ __launch_bounds__(256) void k_scatter_pol_bilinear(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                              int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                              const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                              const double* __restrict__ vals) {
    const int64_t plane = nx * nrows;
    for (Trip<PXL_SUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_SUNR], qu[PXL_SUNR];
        double v[PXL_SUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        trip.load(vals, n, v, 0.0);
        Cell2 cell[PXL_SUNR];
        Weights2 w[PXL_SUNR];
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            cell[u] = cell2<true>(s, ad[u], nx, ny, row0, nrows, periodic, trip.k(u) < n);
            w[u] = weights2(cell[u].fx, cell[u].fy);
        }
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            double t[NP];
            pol_terms<NP>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < NP; ++c) scatter2(dst + (int64_t)c * plane, cell[u], w[u], t[c]);
        }
    }
}

// order 3 (E^T only): k_scatter_cubic's sixteen taps, domain and live rule, PXL_CUNR points per lane and trip like it.  A
// plane's base moves by a pointer bump.
template <int NP>
__global__ __launch_bounds__(256) void k_scatter_pol_cubic(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                           int periodic, int64_t n, const double2* __restrict__ sky,
                                                           const double2* __restrict__ resp, const double* __restrict__ vals) {
    const int64_t plane = nx * ny;
    for (Trip<PXL_CUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_CUNR], qu[PXL_CUNR];
        double v[PXL_CUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        trip.load(vals, n, v, 0.0);
#pragma unroll
        for (int u = 0; u < PXL_CUNR; ++u) {
            const Cell4<int32_t> cell = cell4<int32_t>(s, ad[u], nx, ny, periodic, trip.k(u) < n);
            if (!cell.in) continue;
            double t[NP];
            pol_terms<NP>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < NP; ++c) scatter4(dst + (int64_t)c * plane, cell, t[c]);
        }
    }
}
