// pxl_taps.h -- what one sky point touches on a CAR map: the one pixel of the nearest-pixel kernels, the 2 x 2 cell of the bilinear
// kernels and the 4 x 4 cell of the cubic ones, with the gathers, blends and adds over them; included by pxl_kernels.hip before pxl_sample.h (one translation unit,
// -ffp-contract=off).
//
// This is the single definition of the cell, seam, window and domain rules.  The samplers (pxl_sample.h, pxl_spline.h, pxl_pol.h,
// pxl_nearest.h), their transposes (pxl_scatter.h, pxl_spline.h, pxl_pol.h, pxl_nearest.h) and the normal operator (pxl_normal.h) all call it, so a tap the
// sampler reads as 0 is a tap the transpose drops -- <P m, d> = <m, P^T d> at rounding level -- and a fused kernel's terms are
// the composition's bits, by construction.  Every helper is inlined and every floating-point expression is written once, in
// the operand order and grouping the tests' references have (tests/*_ref.py).
#pragma once

// Points per lane and trip.  All of a trip's loads are issued before its first arithmetic, add or store.
#ifndef PXL_SUNR
#define PXL_SUNR 4          // k_sample_bilinear, k_sample_pairs, k_scatter_bilinear, k_scatter_pol_bilinear: 4x the gathers in flight per lane
#endif
#define PXL_PSUNR 2         // k_sample_pol_bilinear: 6 row loads per point (2 per plane)
#define PXL_CUNR 2          // k_scatter_cubic, k_scatter_pol_cubic: wx wy col row of each point; sixteen offsets and weights would not fit beside a second
#ifndef PXL_NUNR
#define PXL_NUNR 1          // k_normal_pol_bilinear: 93 VGPRs, 5 waves/SIMD; two points (151, 3 waves) time the same within 0.5 %
#endif
#ifndef PXL_ZUNR
#define PXL_ZUNR 4          // the order-0 kernels of pxl_nearest.h: one offset per point, so four points fit
#endif

// ---- the adds of every transpose: no-return agent-scope FP64 atomics (one global_atomic_add_f64 each, executed at the memory
// side).  The order of the additions into one pixel is whatever order they arrive in.
__device__ __forceinline__ void scatter_add(double* p, double x) {
    __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the no-return form
}
// ---- the per-plane terms of the polarised transpose for the value v of a point with response (q, u):
//   t_0 = v, t_1 = q v, t_2 = u v                      (NP = 3: signal, planes I Q U)
//   t_3 = q t_1, t_4 = q t_2, t_5 = u t_2              (NP = 6: weights, planes II IQ IU QQ QU UU)
// each product one rounding, which is what the scalar scatter adds for vals[c][k] = t_c formed the same way.
template <int NP>
__host__ __device__ __forceinline__ void pol_terms(double v, double2 qu, double* t) {
    t[0] = v; t[1] = qu.x * v; t[2] = qu.y * v;
    if (NP == 6) { t[3] = qu.x * t[1]; t[4] = qu.x * t[2]; t[5] = qu.y * t[2]; }
}

// ================================================================================================
// Order 0: the one-pixel cell
// ================================================================================================
// Element offset of the pixel that owns the point, into one plane of the resident rows [row0, row0 + nrows); -1 = the point is
// not on the map (past an edge of a map that is not periodic, a row outside the map or the window): the samplers read it as
// +0.0, the transposes add nothing.  fin: the position is finite (a sampler writes NaN where it is not).
struct Cell0 {
    int64_t off;
    bool fin;
};
// The position is the order-1 position bit for bit (the same Sky2Pix, safe = 1).  Pixel i owns [i - 0.5, i + 0.5): with
// x = i0 + fx, fx = x - floor(x) EXACT, the pixel is i0 + (fx >= 0.5), so a tie goes to the higher index and the rule has no
// rounding of its own (floor(x + 0.5) would round x + 0.5 first).  Column: wrapped on a periodic map, otherwise on the map iff
// 1 <= i <= nx.  Row: on the map iff 1 <= j <= ny and inside the window.  GATED as for cell2: a transpose's point past the
// batch, or with a position that is not finite, has offset -1; a sampler does not gate and writes NaN by `fin`.
template <bool GATED>
__device__ __forceinline__ Cell0 cell0(const Sky2Pix& s, double2 ad, int64_t nx, int64_t ny, int64_t row0, int64_t nrows,
                                       int periodic, bool in_batch) {
    Cell0 c;
    const double x = s2p_x(s, ad.x), y = s2p_y(s, ad.y);
    c.fin = isfinite(x) && isfinite(y);
    const bool live = GATED ? in_batch && c.fin : true;
    int32_t i0, j0;
    double fx, fy;
    split_cell(x, &i0, &fx);
    split_cell(y, &j0, &fy);
    int64_t i = (int64_t)i0 + (fx >= 0.5 ? 1 : 0);
    const int64_t j = (int64_t)j0 + (fy >= 0.5 ? 1 : 0);
    bool ok = live;
    if (periodic) i = wrap_col(i, nx);
    else ok = ok && (i >= 1 && i <= nx);
    const int64_t jr = j - 1 - row0;                                          // resident row index
    ok = ok && (j >= 1 && j <= ny && jr >= 0 && jr < nrows);
    c.off = ok ? jr * nx + (i - 1) : -1;
    return c;
}
// the pixel's value as it is stored: a select, no arithmetic, so -0.0, subnormals, +-Inf and NaN payloads come back as bits.
// The load is unconditional (no branch in front of the gathers), from `fallback` where the point is off the map: the first
// coordinate pair of the batch, readable whenever n >= 1, as for gather2_wide.  pl + offset is never formed from -1.
__device__ __forceinline__ double load0(const double* pl, const Cell0& c, const double2* fallback) {
    return *(c.off >= 0 ? pl + c.off : reinterpret_cast<const double*>(fallback));
}
__device__ __forceinline__ double value0(const Cell0& c, double loaded) {
    return c.fin ? (c.off >= 0 ? loaded : 0.0) : __builtin_nan("");
}

// ================================================================================================
// Order 1: the 2 x 2 cell
// ================================================================================================
// Element offsets of the four taps into one plane of the resident rows [row0, row0 + nrows); -1 = a tap that is not on the map
// (past an edge of a map that is not periodic, a row outside the map or the window): the samplers read it as 0, the transposes
// drop it.  fin: the position is finite (a sampler writes NaN where it is not).  wide: all four taps are on the map and the
// two columns adjacent, so a row's two taps are one 2-element load.
struct Cell2 {
    int64_t o00, o10, o01, o11;
    double fx, fy;
    bool fin, wide;
};
// sky2pix(safe = 1) through the inlined evaluators (fast path + library fmod per coordinate): the out-of-line fallback of
// sample_coords() buys k_sample_bilinear a fourth wave per SIMD and costs it 15 % (48.6-50.2 vs 55.9-57.3 ms per 1e9 points,
// same box) -- with four separate taps per point more waves in flight evict each other's sectors.
// GATED (the transposes and the normal operator): a point past the end of the batch, or one whose position is not finite, has
// no taps at all.  The samplers do not gate: they read whatever cell split_cell gives and write NaN by `fin`, and pass
// in_batch = true (it has no default: a transpose that forgot it would add taps for the lanes past the batch).
// A caller without a row window passes row0 = 0, nrows = ny and the window tests fold away.
template <bool GATED>
__device__ __forceinline__ Cell2 cell2(const Sky2Pix& s, double2 ad, int64_t nx, int64_t ny, int64_t row0, int64_t nrows,
                                       int periodic, bool in_batch) {
    Cell2 c;
    const double x = s2p_x(s, ad.x), y = s2p_y(s, ad.y);
    c.fin = isfinite(x) && isfinite(y);
    const bool live = GATED ? in_batch && c.fin : true;
    int32_t i0, j0;
    split_cell(x, &i0, &c.fx);
    split_cell(y, &j0, &c.fy);
    int64_t ia = i0, ib = (int64_t)i0 + 1;
    bool oka = live, okb = live;
    if (periodic) { ia = wrap_col(ia, nx); ib = wrap_col(ib, nx); }
    else { oka = oka && (ia >= 1 && ia <= nx); okb = okb && (ib >= 1 && ib <= nx); }
    const int64_t ja = (int64_t)j0 - 1 - row0, jb = ja + 1;                    // resident row indices
    const bool rowa = (j0 >= 1 && j0 <= ny && ja >= 0 && ja < nrows);
    const bool rowb = ((int64_t)j0 + 1 >= 1 && (int64_t)j0 + 1 <= ny && jb >= 0 && jb < nrows);
    c.o00 = (rowa && oka) ? ja * nx + (ia - 1) : -1;
    c.o10 = (rowa && okb) ? ja * nx + (ib - 1) : -1;
    c.o01 = (rowb && oka) ? jb * nx + (ia - 1) : -1;
    c.o11 = (rowb && okb) ? jb * nx + (ib - 1) : -1;
    c.wide = c.o00 >= 0 && c.o01 >= 0 && c.o10 == c.o00 + 1 && c.o11 == c.o01 + 1;
    return c;
}

// ---- gather, in two stages: a caller issues stage 1 for every point and plane of its trip before any arithmetic.
struct Taps2 { double m00, m10, m01, m11; };
template <typename T> struct __attribute__((packed, aligned(sizeof(T)))) TT { T a, b; };
// Stage 1, unconditional: ONE 2-element load per row of a wide point (element-aligned only; 54.9 vs 57.8 ms per 1e9 points
// against four separate taps, same box).  The other points still issue the loads (no branch in front of the gathers), from an
// address that always exists: `fallback`, the first coordinate pair of the batch (16 readable bytes whenever n >= 1).  The map
// itself may not have two elements to read -- an empty resident window (pl == NULL) or a 1 x 1 one -- and pl + offset is never
// formed from a negative offset.
template <typename T>
__device__ __forceinline__ Taps2 gather2_wide(const T* pl, const Cell2& c, const double2* fallback) {
    const TT<T> ra = *(c.wide ? reinterpret_cast<const TT<T>*>(pl + c.o00) : reinterpret_cast<const TT<T>*>(fallback));
    const TT<T> rb = *(c.wide ? reinterpret_cast<const TT<T>*>(pl + c.o01) : reinterpret_cast<const TT<T>*>(fallback));
    return Taps2{(double)ra.a, (double)ra.b, (double)rb.a, (double)rb.b};
}
// Stage 2, for the rare point that is not wide (seam, edges, rows outside the window): the four taps one by one.
template <typename T>
__device__ __forceinline__ void gather2_fixup(const T* pl, const Cell2& c, Taps2& m) {
    m.m00 = c.o00 >= 0 ? (double)pl[c.o00] : 0.0;
    m.m10 = c.o10 >= 0 ? (double)pl[c.o10] : 0.0;
    m.m01 = c.o01 >= 0 ? (double)pl[c.o01] : 0.0;
    m.m11 = c.o11 >= 0 ? (double)pl[c.o11] : 0.0;
}
__host__ __device__ __forceinline__ double lerp2(const Taps2& m, double fx, double fy) {
    const double top = (1 - fx) * m.m00 + fx * m.m10;
    const double bot = (1 - fx) * m.m01 + fx * m.m11;
    return (1 - fy) * top + fy * bot;
}

// ---- scatter: plane pl takes (wy_b * wx_a) * t at the four taps.  Every tap that is on the map takes its add, zero weights
// included: a NaN or Inf value reaches all four.
struct Weights2 { double w00, w10, w01, w11; };
__host__ __device__ __forceinline__ Weights2 weights2(double fx, double fy) {
    return Weights2{(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx};
}
__device__ __forceinline__ void scatter2(double* pl, const Cell2& c, const Weights2& w, double t) {
    if (c.o00 >= 0) scatter_add(pl + c.o00, w.w00 * t);
    if (c.o10 >= 0) scatter_add(pl + c.o10, w.w10 * t);
    if (c.o01 >= 0) scatter_add(pl + c.o01, w.w01 * t);
    if (c.o11 >= 0) scatter_add(pl + c.o11, w.w11 * t);
}

// ================================================================================================
// Order 3: the 4 x 4 cell of the cubic B-spline
// ================================================================================================
// Index rule of both the prefilter's warm-up and the evaluation's taps: any integer position t (1-based) -> [1, n].
// Cyclic on a periodic RA axis, whole-sample mirror (t -> 2 - t, t -> 2n - t, repeated) otherwise.  n >= 2.
__host__ __device__ inline int64_t spline_fold(int64_t t, int64_t n, int periodic) {
    if (t >= 1 && t <= n) return t;
    if (periodic) { int64_t u = (t - 1) % n; if (u < 0) u += n; return u + 1; }
    const int64_t p = 2 * n - 2;
    int64_t u = (t - 1) % p;
    if (u < 0) u += p;
    if (u >= n) u = p - u;
    return u + 1;
}
// Weights of the four taps i0-1 .. i0+2 at fraction f, written op for op as tests/spline_ref.py has them.
__host__ __device__ inline void spline_weights(double f, double* w) {
    const double t = 1 - f, f2 = f * f, f3 = f2 * f;
    w[0] = ((t * t) * t) / 6;
    w[1] = ((3 * f3 - 6 * f2) + 4) / 6;
    w[2] = (((-3 * f3 + 3 * f2) + 3 * f) + 1) / 6;
    w[3] = f3 / 6;
}
// x = cell + frac inside [0.5, n + 0.5]: the map ends at its pixel edges (frac = x - floor(x) is exact)
__host__ __device__ inline bool spline_in_domain(int64_t cell, double frac, int64_t n) {
    return (cell >= 1 || (cell == 0 && frac >= 0.5)) && (cell < n || (cell == n && frac <= 0.5));
}

// Weights, folded 0-based columns and element offsets of the tap rows of one point (full maps only: no row window).
// fin: the position is finite (a sampler writes NaN where it is not).  in: the point is in the batch, finite and inside the
// domain; only then are col and row taps (they are 0 otherwise): a sampler gives 0 outside the domain, a transpose adds nothing.
// COL: the samplers hold columns as int64, the transposes as int32 for register room beside a second point
// (spline_shape_check: an axis has at most 4e8 pixels).
template <typename COL>
struct Cell4 {
    double wx[4], wy[4];
    COL col[4];
    int64_t row[4];
    bool fin, in;
};
template <typename COL>
__device__ __forceinline__ Cell4<COL> cell4(const Sky2Pix& s, double2 ad, int64_t nx, int64_t ny, int periodic, bool in_batch) {
    Cell4<COL> c;
    const double x = s2p_x(s, ad.x), y = s2p_y(s, ad.y);
    c.fin = isfinite(x) && isfinite(y);
    int32_t i0, j0;
    double fx, fy;
    split_cell(x, &i0, &fx);
    split_cell(y, &j0, &fy);
    c.in = in_batch && c.fin && (periodic || spline_in_domain(i0, fx, nx)) && spline_in_domain(j0, fy, ny);
    spline_weights(fx, c.wx);
    spline_weights(fy, c.wy);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        c.col[a] = c.in ? (COL)(spline_fold((int64_t)i0 - 1 + a, nx, periodic) - 1) : 0;
        c.row[a] = c.in ? (spline_fold((int64_t)j0 - 1 + a, ny, 0) - 1) * nx : 0;
    }
    return c;
}
// the sixteen taps of one plane, and their blend: separate steps, so that a caller can issue several planes' loads first
template <typename COL>
__device__ __forceinline__ void gather4(const double* pl, const Cell4<COL>& c, double t[4][4]) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const double* rw = pl + c.row[b];
#pragma unroll
        for (int a = 0; a < 4; ++a) t[b][a] = rw[c.col[a]];
    }
}
template <typename COL>
__host__ __device__ __forceinline__ double blend4(const Cell4<COL>& c, const double t[4][4]) {
    double hb[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) hb[b] = ((c.wx[0] * t[b][0] + c.wx[1] * t[b][1]) + c.wx[2] * t[b][2]) + c.wx[3] * t[b][3];
    return ((c.wy[0] * hb[0] + c.wy[1] * hb[1]) + c.wy[2] * hb[2]) + c.wy[3] * hb[3];
}
// scatter: plane pl takes (wy[b] * wx[a]) * t at the sixteen taps (the products are formed at the add).  Taps that fold onto
// one pixel next to a mirrored edge are each added on their own; a zero-weight tap still adds, so a NaN or Inf value reaches
// all sixteen.  The caller tests c.in.
template <typename COL>
__device__ __forceinline__ void scatter4(double* pl, const Cell4<COL>& c, double t) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        double* rw = pl + c.row[b];
#pragma unroll
        for (int a = 0; a < 4; ++a) scatter_add(rw + c.col[a], (c.wy[b] * c.wx[a]) * t);
    }
}
