// pxl_distance.h -- distance_transform on CAR maps (transform_distance.jl): for every pixel the angular distance to the
// nearest pixel whose value is zero, exactly, in O(nx * ny) work whatever the mask.
//
// On a CAR map RA depends only on the column and DEC only on the row.  For pixel (i, j) and a zero at (z, j'),
//     d^2 = 2 - 2 (cos d_j cos d_j' cos(a_i - a_z) + sin d_j sin d_j').
// While cos d >= 0 on every row, the best zero of row j' for column i is the one with the largest cos(a_i - a_z), whatever
// the query row j: the nearest zero to the left or to the right, wrapping round to the last or the first zero of the row
// (the way round the RA seam or the gap of a partial map).  k_sdt_rows finds it for every (i, j') in one pass over the map.
// Each row j' then gives column i one point P = (cos d_j' c(i, j'), sin d_j') and pixel (i, j) wants the largest u_j . P,
// u_j = (cos d_j, sin d_j): a vertex of the right-hand convex chain of the column's points.  The points come sorted by
// sin d and u_j turns monotonically with j, so k_sdt_columns builds the chain (monotone chain rule: drop a vertex on a
// clockwise or collinear turn) and answers the column with a pointer that only moves forward.  The distance of the chosen
// zero is then recomputed in the reference's difference form (transform_distance.jl:81-92) and written as acos(1 - d^2/2).
// DESIGN.md 4.8 has the derivation and the error bound.
#pragma once

#define PXL_SDT_ROW_THREADS 1024
#define PXL_SDT_MAX_NX 131072          // a row's zero mask and its two word scans live in LDS: 16 B per 64 pixels
#define PXL_SDT_NONE_R 0x7fffffff      // "no zero to the right"

// cos / sin of the pixel centres' RA (per column) and DEC (per row), as PrecomputedSkyAngles (transform_distance.jl:28-37)
// takes them from pix2sky(m, 1:nx, 1) / pix2sky(m, 1, 1:ny): the affine map, then rewind (car_proj.jl:146-150)
__global__ __launch_bounds__(256) void k_sdt_tables(CarAffine c, int64_t nx, int64_t ny, double2* __restrict__ csa,
                                                    double2* __restrict__ csd) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nx + ny; k += (int64_t)gridDim.x * blockDim.x) {
        if (k < nx) {
            const double a = rewind(p2s_ra(c, (double)(k + 1)), PXL_TWOPI_D, 0.0);
            csa[k] = make_double2(cos(a), sin(a));
        } else {
            const double d = rewind(p2s_dec(c, (double)(k - nx + 1)), PXL_TWOPI_D, 0.0);
            csd[k - nx] = make_double2(cos(d), sin(d));
        }
    }
}

// One block per row.  The row's zero mask goes to LDS one wave ballot (64 pixels) at a time, with each 64-bit word's last
// zero (prefix max-scan -> nearest zero at or left of a word) and minus its first zero (suffix max-scan -> nearest zero at
// or right of it).  Then every pixel picks between its left and right candidates by cos(a_i - a_c) from the tables.
// best[row * nx + i]: the column of the row's best zero for column i, or -1 if the row has no zero.
__global__ __launch_bounds__(PXL_SDT_ROW_THREADS) void k_sdt_rows(const double* __restrict__ m, int64_t nx,
                                                                   const double2* __restrict__ csa, int32_t* __restrict__ best) {
    extern __shared__ unsigned long long sdt_lds[];
    __shared__ int32_t wl[PXL_SDT_ROW_THREADS / 64], wr[PXL_SDT_ROW_THREADS / 64];
    __shared__ int32_t carry_l, carry_r;
    const int W = (int)((nx + 63) >> 6);
    unsigned long long* bits = sdt_lds;
    int32_t* lsc = (int32_t*)(bits + W);
    int32_t* rsc = lsc + W;
    const int64_t row = blockIdx.x;
    const double* mr = m + row * nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwave = PXL_SDT_ROW_THREADS / 64;

    // zero mask: four wave chunks per trip so that four loads are in flight per lane
    for (int w0 = wave; w0 < W; w0 += 4 * nwave) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = (int64_t)(w0 + u * nwave) * 64 + lane;
            v[u] = (w0 + u * nwave < W && i < nx) ? mr[i] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int w = w0 + u * nwave;
            const unsigned long long b = __ballot(v[u] == 0.0);        // iszero: -0.0 counts, NaN does not
            if (w < W && lane == 0) {
                bits[w] = b;
                lsc[w] = b ? w * 64 + 63 - __clzll((long long)b) : -1;
                rsc[w] = b ? -(w * 64 + __ffsll((long long)b) - 1) : -PXL_SDT_NONE_R;
            }
        }
    }
    if (threadIdx.x == 0) { carry_l = -1; carry_r = -PXL_SDT_NONE_R; }
    __syncthreads();
    // prefix max of lsc and suffix max of rsc, 1024 words per trip: wave shuffle scans + wave totals in LDS + a carry
    for (int b0 = 0; b0 < W; b0 += PXL_SDT_ROW_THREADS) {
        const int k = b0 + threadIdx.x;
        int32_t il = k < W ? lsc[k] : -1;
        int32_t ir = k < W ? rsc[W - 1 - k] : -PXL_SDT_NONE_R;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t ol = __shfl_up(il, off, 64), orr = __shfl_up(ir, off, 64);
            if (lane >= off) { il = max(il, ol); ir = max(ir, orr); }
        }
        if (lane == 63) { wl[wave] = il; wr[wave] = ir; }
        __syncthreads();
        int32_t pl = carry_l, pr = carry_r;
        for (int w = 0; w < wave; ++w) { pl = max(pl, wl[w]); pr = max(pr, wr[w]); }
        il = max(il, pl); ir = max(ir, pr);
        if (k < W) { lsc[k] = il; rsc[W - 1 - k] = ir; }
        __syncthreads();
        if (threadIdx.x == PXL_SDT_ROW_THREADS - 1) { carry_l = il; carry_r = ir; }
        __syncthreads();
    }
    const int32_t last = lsc[W - 1], first = -rsc[0];
    for (int64_t i = threadIdx.x; i < nx; i += PXL_SDT_ROW_THREADS) {
        int32_t c = -1;
        if (last >= 0) {
            const int w = (int)(i >> 6), b = (int)(i & 63);
            const unsigned long long mw = bits[w];
            const unsigned long long lo = mw & (b == 63 ? ~0ull : ((2ull << b) - 1)), hi = mw & (~0ull << b);
            int32_t l = lo ? w * 64 + 63 - __clzll((long long)lo) : (w > 0 ? lsc[w - 1] : -1);
            int32_t r = hi ? w * 64 + __ffsll((long long)hi) - 1 : (w + 1 < W ? -rsc[w + 1] : PXL_SDT_NONE_R);
            if (l < 0) l = last;                 // none to the left: round the other way to the row's last zero
            if (r == PXL_SDT_NONE_R) r = first;  // none to the right: its first zero
            if (l == r) {
                c = l;
            } else {
                const double2 ai = csa[i], al = csa[l], ar = csa[r];
                const double cl = ai.x * al.x + ai.y * al.y, cr = ai.x * ar.x + ai.y * ar.y;
                c = cr > cl ? r : l;
            }
        }
        best[row * nx + i] = c;
    }
}

// chain entry: row in the high 32 bits, column of the row's best zero in the low 32
__device__ inline long long sdt_pack(int64_t j, int32_t c) { return (long long)(((uint64_t)j << 32) | (uint32_t)c); }
__device__ inline void sdt_point(const double2* __restrict__ csa, const double2* __restrict__ csd, double2 ai, long long e,
                                 double* x, double* y) {
    const double2 d = csd[(int32_t)(e >> 32)], a = csa[(int32_t)(e & 0xffffffffLL)];
    *x = fmax(d.x, 0.0) * (ai.x * a.x + ai.y * a.y);    // cos d rounds to a few 1e-17 below zero at a pole: read it as 0
    *y = d.y;
}

// One thread per column: build the right chain over the rows that have a zero, bottom (smallest sin d) first, into the
// column's own stretch of `chain` (ny entries, contiguous per column so each thread fills whole lines); then sweep the
// query rows in the same order.  up: DEC increases with the row index.
#define PXL_SDT_BATCH 4
__global__ __launch_bounds__(64) void k_sdt_columns(const int32_t* __restrict__ best, int64_t nx, int64_t ny, int up,
                                                    const double2* __restrict__ csa, const double2* __restrict__ csd,
                                                    long long* __restrict__ chain, double* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= nx) return;
    const double2 ai = csa[i];
    long long* ch = chain + i * ny;
    int64_t n = 0;
    double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;     // top and second vertex of the chain
    for (int64_t t0 = 0; t0 < ny; t0 += PXL_SDT_BATCH) {
        int32_t c[PXL_SDT_BATCH];
        int64_t jj[PXL_SDT_BATCH];
#pragma unroll
        for (int u = 0; u < PXL_SDT_BATCH; ++u) {
            jj[u] = up ? t0 + u : ny - 1 - (t0 + u);
            c[u] = t0 + u < ny ? best[jj[u] * nx + i] : -1;
        }
#pragma unroll
        for (int u = 0; u < PXL_SDT_BATCH; ++u) {
            if (c[u] < 0) continue;
            const double2 d = csd[jj[u]], a = csa[c[u]];
            const double px = fmax(d.x, 0.0) * (ai.x * a.x + ai.y * a.y), py = d.y;
            while (n >= 2 && (x0 - x1) * (py - y1) - (y0 - y1) * (px - x1) <= 0.0) {
                --n;
                x0 = x1; y0 = y1;
                if (n >= 2) sdt_point(csa, csd, ai, ch[n - 2], &x1, &y1);
            }
            ch[n++] = sdt_pack(jj[u], c[u]);
            x1 = x0; y1 = y0; x0 = px; y0 = py;
        }
    }
    if (n == 0) {        // no zero anywhere in the map
        for (int64_t j = 0; j < ny; ++j) dist[j * nx + i] = __builtin_huge_val();
        return;
    }
    int64_t k = 0;
    long long ek = ch[0], en = 0;
    double xk, yk, xn = 0.0, yn = 0.0;
    sdt_point(csa, csd, ai, ek, &xk, &yk);
    if (n > 1) { en = ch[1]; sdt_point(csa, csd, ai, en, &xn, &yn); }
    for (int64_t t = 0; t < ny; ++t) {
        const int64_t j = up ? t : ny - 1 - t;
        const int64_t o = j * nx + i;
        const int32_t self = best[o];
        const double2 u = csd[j];
        while (k + 1 < n && u.x * xn + u.y * yn >= u.x * xk + u.y * yk) {
            ++k;
            xk = xn; yk = yn; ek = en;
            if (k + 1 < n) { en = ch[k + 1]; sdt_point(csa, csd, ai, en, &xn, &yn); }
        }
        double r = 0.0;                      // a zero pixel: its row's best zero for its column is itself (best == i only then)
        if (self != (int32_t)i) {
            const double2 dz = csd[(int32_t)(ek >> 32)], az = csa[(int32_t)(ek & 0xffffffffLL)];
            const double xa = u.x * ai.x, ya = u.x * ai.y, za = u.y;
            const double xb = dz.x * az.x, yb = dz.x * az.y, zb = dz.y;
            const double d2 = (xa - xb) * (xa - xb) + (ya - yb) * (ya - yb) + (za - zb) * (za - zb);
            r = acos(1.0 - d2 / 2.0);
        }
        dist[o] = r;
    }
}
