// pxl_pol.h -- the polarised pointing matrix: d = I + q Q + u U sampled from, and scatter-added into, the
// three planes of an IQU CAR map in one pass; included by pxl_kernels.hip after pxl_spline.h (one translation unit,
// -ffp-contract=off).
//
// Every kernel here restates its scalar counterpart (k_sample_bilinear, k_sample_cubic, k_scatter_bilinear, k_scatter_cubic)
// with the same helpers -- s2p_x / s2p_y in the reciprocal form with safe = 1, split_cell, wrap_col, spline_weights,
// spline_fold, spline_in_domain, scatter_add -- and the same expressions, so position, cell, weights, offsets and every
// per-plane value or term are the counterpart's bits.  What is new: position, cell, weights and offsets are formed ONCE per
// point and reused across the planes, the response pair (q, u) is one double2 load beside the coordinates, and the three
// (or six) per-plane streams of the composition never exist.  Q and U are three independent scalar planes: no spin-2 sign
// flip at the DEC mirror or across a pole (NOTES item 7).
#pragma once

// ---- forward, order 1: out[k] = (s_I + q_k * s_Q) + u_k * s_U, s_c what k_sample_bilinear<double> writes for plane c.
// A lane carries PXL_PSUNR points per trip; the 6 row loads of each (2 per plane) are issued before the first store.
#define PXL_PSUNR 2
__global__ __launch_bounds__(256) void k_sample_pol_bilinear(Sky2Pix s, const double* __restrict__ src, int64_t nx, int64_t ny,
                                                             int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                             const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                             double* __restrict__ out) {
    const int64_t chunk = (int64_t)blockDim.x * PXL_PSUNR;
    const int64_t plane = nx * nrows;
    for (int64_t k0 = (int64_t)blockIdx.x * chunk + threadIdx.x; k0 < n; k0 += (int64_t)gridDim.x * chunk) {
        double2 ad[PXL_PSUNR], qu[PXL_PSUNR];
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
            const int64_t k = k0 + u * blockDim.x;
            ad[u] = (k < n) ? sky[k] : make_double2(0.0, 0.0);
            qu[u] = (k < n) ? resp[k] : make_double2(0.0, 0.0);
        }
        int64_t o00[PXL_PSUNR], o10[PXL_PSUNR], o01[PXL_PSUNR], o11[PXL_PSUNR];   // element offsets, -1 = reads as 0
        double fx[PXL_PSUNR], fy[PXL_PSUNR];
        bool fin[PXL_PSUNR], wide[PXL_PSUNR];
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
            const double x = s2p_x(s, ad[u].x), y = s2p_y(s, ad[u].y);
            fin[u] = isfinite(x) && isfinite(y);
            int32_t i0, j0;
            split_cell(x, &i0, &fx[u]);
            split_cell(y, &j0, &fy[u]);
            int64_t ia = i0, ib = (int64_t)i0 + 1;
            bool oka = true, okb = true;
            if (periodic) { ia = wrap_col(ia, nx); ib = wrap_col(ib, nx); }
            else { oka = (ia >= 1 && ia <= nx); okb = (ib >= 1 && ib <= nx); }
            const int64_t ja = (int64_t)j0 - 1 - row0, jb = ja + 1;               // resident row indices
            const bool rowa = (j0 >= 1 && j0 <= ny && ja >= 0 && ja < nrows);
            const bool rowb = ((int64_t)j0 + 1 >= 1 && (int64_t)j0 + 1 <= ny && jb >= 0 && jb < nrows);
            o00[u] = (rowa && oka) ? ja * nx + (ia - 1) : -1;
            o10[u] = (rowa && okb) ? ja * nx + (ib - 1) : -1;
            o01[u] = (rowb && oka) ? jb * nx + (ia - 1) : -1;
            o11[u] = (rowb && okb) ? jb * nx + (ib - 1) : -1;
            wide[u] = o00[u] >= 0 && o01[u] >= 0 && o10[u] == o00[u] + 1 && o11[u] == o01[u] + 1;
        }
        // interior points take one 2-element load per row and plane, as the scalar sampler does; the others still issue the
        // loads, from the first coordinate pair of the batch (16 readable bytes whenever n >= 1), and take their taps below
        struct __attribute__((packed, aligned(8))) TT { double a, b; };
        double m00[PXL_PSUNR][3], m10[PXL_PSUNR][3], m01[PXL_PSUNR][3], m11[PXL_PSUNR][3];
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double* pl = src + (int64_t)c * plane;
                const TT ra = *(wide[u] ? reinterpret_cast<const TT*>(pl + o00[u]) : reinterpret_cast<const TT*>(sky));
                const TT rb = *(wide[u] ? reinterpret_cast<const TT*>(pl + o01[u]) : reinterpret_cast<const TT*>(sky));
                m00[u][c] = ra.a; m10[u][c] = ra.b; m01[u][c] = rb.a; m11[u][c] = rb.b;
            }
        }
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
            if (__builtin_expect(!wide[u], 0)) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double* pl = src + (int64_t)c * plane;
                    m00[u][c] = o00[u] >= 0 ? pl[o00[u]] : 0.0;
                    m10[u][c] = o10[u] >= 0 ? pl[o10[u]] : 0.0;
                    m01[u][c] = o01[u] >= 0 ? pl[o01[u]] : 0.0;
                    m11[u][c] = o11[u] >= 0 ? pl[o11[u]] : 0.0;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PXL_PSUNR; ++u) {
            const int64_t k = k0 + u * blockDim.x;
            double sc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double top = (1 - fx[u]) * m00[u][c] + fx[u] * m10[u][c];
                const double bot = (1 - fx[u]) * m01[u][c] + fx[u] * m11[u][c];
                const double v = (1 - fy[u]) * top + fy[u] * bot;
                sc[c] = fin[u] ? v : __builtin_nan("");
            }
            if (k < n) out[k] = (sc[0] + qu[u].x * sc[1]) + qu[u].y * sc[2];
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
        const double x = s2p_x(s, ad.x), y = s2p_y(s, ad.y);
        const bool fin = isfinite(x) && isfinite(y);
        int32_t i0, j0;
        double fx, fy;
        split_cell(x, &i0, &fx);
        split_cell(y, &j0, &fy);
        const bool in = fin && (periodic || spline_in_domain(i0, fx, nx)) && spline_in_domain(j0, fy, ny);
        double wx[4], wy[4];
        spline_weights(fx, wx);
        spline_weights(fy, wy);
        int64_t col[4], row[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            col[a] = in ? spline_fold((int64_t)i0 - 1 + a, nx, periodic) - 1 : 0;
            row[a] = in ? (spline_fold((int64_t)j0 - 1 + a, ny, 0) - 1) * nx : 0;
        }
        double sc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) sc[c] = fin ? 0.0 : __builtin_nan("");
        if (in) {
            double t[3][4][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int a = 0; a < 4; ++a) t[c][b][a] = coeffs[(int64_t)c * nx * ny + row[b] + col[a]];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double hb[4];
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    hb[b] = ((wx[0] * t[c][b][0] + wx[1] * t[c][b][1]) + wx[2] * t[c][b][2]) + wx[3] * t[c][b][3];
                sc[c] = ((wy[0] * hb[0] + wy[1] * hb[1]) + wy[2] * hb[2]) + wy[3] * hb[3];
            }
        }
        out[k] = (sc[0] + qu.x * sc[1]) + qu.y * sc[2];
    }
}

// ---- transpose.  Plane c of dst takes (wy_b * wx_a) * t_c for the value v = vals[k] of point k:
//   t_0 = v, t_1 = q v, t_2 = u v                      (NP = 3: signal, planes I Q U)
//   t_3 = q t_1, t_4 = q t_2, t_5 = u t_2              (NP = 6: weights, planes II IQ IU QQ QU UU)
// each product one rounding, which is what the scalar scatter adds for vals[c][k] = t_c formed the same way.
template <int NP>
__device__ inline void pol_terms(double v, double2 qu, double* t) {
    t[0] = v; t[1] = qu.x * v; t[2] = qu.y * v;
    if (NP == 6) { t[3] = qu.x * t[1]; t[4] = qu.x * t[2]; t[5] = qu.y * t[2]; }
}

// order 1: k_scatter_bilinear's taps, window and live rule; a lane carries PXL_SUNR points per trip like it and all of a
// trip's loads (coordinates, responses, values) are issued before its first add
template <int NP>
__global__ __launch_bounds__(256) void k_scatter_pol_bilinear(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                              int64_t row0, int64_t nrows, int periodic, int64_t n,
                                                              const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                              const double* __restrict__ vals) {
    const int64_t chunk = (int64_t)blockDim.x * PXL_SUNR;
    const int64_t plane = nx * nrows;
    for (int64_t k0 = (int64_t)blockIdx.x * chunk + threadIdx.x; k0 < n; k0 += (int64_t)gridDim.x * chunk) {
        double2 ad[PXL_SUNR], qu[PXL_SUNR];
        double v[PXL_SUNR];
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            const int64_t k = k0 + u * blockDim.x;
            ad[u] = (k < n) ? sky[k] : make_double2(0.0, 0.0);
            qu[u] = (k < n) ? resp[k] : make_double2(0.0, 0.0);
            v[u] = (k < n) ? vals[k] : 0.0;
        }
        int64_t o00[PXL_SUNR], o10[PXL_SUNR], o01[PXL_SUNR], o11[PXL_SUNR];   // element offsets, -1 = dropped tap
        double w00[PXL_SUNR], w10[PXL_SUNR], w01[PXL_SUNR], w11[PXL_SUNR];   // wy_b * wx_a
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            const double x = s2p_x(s, ad[u].x), y = s2p_y(s, ad[u].y);
            const bool live = (k0 + u * blockDim.x < n) && isfinite(x) && isfinite(y);
            int32_t i0, j0;
            double fx, fy;
            split_cell(x, &i0, &fx);
            split_cell(y, &j0, &fy);
            int64_t ia = i0, ib = (int64_t)i0 + 1;
            bool oka = live, okb = live;
            if (periodic) { ia = wrap_col(ia, nx); ib = wrap_col(ib, nx); }
            else { oka = oka && (ia >= 1 && ia <= nx); okb = okb && (ib >= 1 && ib <= nx); }
            const int64_t ja = (int64_t)j0 - 1 - row0, jb = ja + 1;               // resident row indices
            const bool rowa = (j0 >= 1 && j0 <= ny && ja >= 0 && ja < nrows);
            const bool rowb = ((int64_t)j0 + 1 >= 1 && (int64_t)j0 + 1 <= ny && jb >= 0 && jb < nrows);
            o00[u] = (rowa && oka) ? ja * nx + (ia - 1) : -1;
            o10[u] = (rowa && okb) ? ja * nx + (ib - 1) : -1;
            o01[u] = (rowb && oka) ? jb * nx + (ia - 1) : -1;
            o11[u] = (rowb && okb) ? jb * nx + (ib - 1) : -1;
            w00[u] = (1 - fy) * (1 - fx); w10[u] = (1 - fy) * fx;
            w01[u] = fy * (1 - fx);       w11[u] = fy * fx;
        }
        // every tap that is on the map takes its add in every plane, zero weights included
#pragma unroll
        for (int u = 0; u < PXL_SUNR; ++u) {
            double t[NP];
            pol_terms<NP>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < NP; ++c) {
                double* pl = dst + (int64_t)c * plane;
                if (o00[u] >= 0) scatter_add(pl + o00[u], w00[u] * t[c]);
                if (o10[u] >= 0) scatter_add(pl + o10[u], w10[u] * t[c]);
                if (o01[u] >= 0) scatter_add(pl + o01[u], w01[u] * t[c]);
                if (o11[u] >= 0) scatter_add(pl + o11[u], w11[u] * t[c]);
            }
        }
    }
}

// order 3 (E^T only): k_scatter_cubic's sixteen taps, domain and live rule, PXL_CUNR points per lane and trip like it.  The
// sixteen products wy[b] * wx[a] of a point are formed once and serve every plane; a plane's base moves by a pointer bump.
template <int NP>
__global__ __launch_bounds__(256) void k_scatter_pol_cubic(Sky2Pix s, double* __restrict__ dst, int64_t nx, int64_t ny,
                                                           int periodic, int64_t n, const double2* __restrict__ sky,
                                                           const double2* __restrict__ resp, const double* __restrict__ vals) {
    const int64_t chunk = (int64_t)blockDim.x * PXL_CUNR;
    const int64_t plane = nx * ny;
    for (int64_t k0 = (int64_t)blockIdx.x * chunk + threadIdx.x; k0 < n; k0 += (int64_t)gridDim.x * chunk) {
        double2 ad[PXL_CUNR], qu[PXL_CUNR];
        double v[PXL_CUNR];
#pragma unroll
        for (int u = 0; u < PXL_CUNR; ++u) {
            const int64_t k = k0 + u * blockDim.x;
            ad[u] = (k < n) ? sky[k] : make_double2(0.0, 0.0);
            qu[u] = (k < n) ? resp[k] : make_double2(0.0, 0.0);
            v[u] = (k < n) ? vals[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PXL_CUNR; ++u) {
            const double x = s2p_x(s, ad[u].x), y = s2p_y(s, ad[u].y);
            int32_t i0, j0;
            double fx, fy;
            split_cell(x, &i0, &fx);
            split_cell(y, &j0, &fy);
            const bool live = (k0 + u * blockDim.x < n) && isfinite(x) && isfinite(y) &&
                              (periodic || spline_in_domain(i0, fx, nx)) && spline_in_domain(j0, fy, ny);
            if (!live) continue;
            double wx[4], wy[4];
            spline_weights(fx, wx);
            spline_weights(fy, wy);
            int32_t col[4];
            int64_t row[4];                                                     // element offset of the tap row
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                col[a] = (int32_t)(spline_fold((int64_t)i0 - 1 + a, nx, periodic) - 1);
                row[a] = (spline_fold((int64_t)j0 - 1 + a, ny, 0) - 1) * nx;
            }
            double t[NP];
            pol_terms<NP>(v[u], qu[u], t);
#pragma unroll
            for (int c = 0; c < NP; ++c) {
                double* pl = dst + (int64_t)c * plane;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    double* rw = pl + row[b];
#pragma unroll
                    for (int a = 0; a < 4; ++a) scatter_add(rw + col[a], (wy[b] * wx[a]) * t[c]);
                }
            }
        }
    }
}
