// pxl_fit.h -- the weighted least-squares fit that the timestream filters share: "fit a few basis functions to
// the live samples of an item, subtract the model from all of them".  pxl_polyfilter.h fits Legendre polynomials along a segment of one
// detector, pxl_modefilter.h the caller's couplings across a group of detectors at one time sample; each keeps only which lane takes
// which sample, in which order, and how its lanes' sums meet.  Included by pxl_kernels.hip before both (one translation unit,
// -ffp-contract=off: every product and every sum below is rounded once, nothing is fused).
//
// THE ITEMS (fit_span).  n_items + 1 offsets along an axis of n_axis samples make n_items fitted items [offsets[s], offsets[s+1]) and
// two more that are only copied: the samples before the first offset and from the last offset on.  Both ends of an item are clamped
// to [0, n_axis]; an end that is not above its start makes the item empty.  A copied item skips the first pass: its sums stay +0.0,
// pivot 0 is rejected (0 > 0 fails), and the second pass copies it.  So every lane runs the same code and no shuffle or barrier is
// divergent.
//
// THE MOMENTS.  A sample is LIVE when wfit > 0 (a NaN weight is not; a null wfit is 1.0 everywhere).  With B the NP basis
// values at the sample, over the live samples of the item
//     G_ik = sum (w * B_i) * B_k   for i >= k,        b_i = sum (w * B_i) * d
// each term two roundings; a sample that is not live adds no term, and its d enters no arithmetic at all.  A lane's sums, each
// starting from +0.0: the NG moments in g, G_ik at fit_idx(i, k), and the NP right-hand sides in b.  A kernel may keep b directly
// behind g in one array of NV (pxl_modefilter.h does, for its LDS chunks).
//
// THE TREE.  Lanes are joined level by level, v_l = v_l + v_(l ^ off) -- IEEE addition commutes, so every lane ends
// with the bits lane 0 has, which are those of the tree l += l + off.  Which offs there are, and the levels that cross wavefronts
// through LDS, are the kernel's own.  The bits depend on the arguments alone: no atomics.
//
// The moment terms and the tree level are three lines each and stand in both kernels' loops, marked with these headings, not in a
// helper here: as helpers they compiled to the same arithmetic with more register moves in the first-pass loop of orders 5 to 7
// and in the tree of order 3 (NOTES.md), and the filters' speed is part of what this file must leave alone.
//
// THE SOLVE (fit_solve, every lane redundantly, in registers): LDL^T of G without pivoting, in the order of the basis.  Row i, for
// k = 0 .. i-1 in order:  U_ik = G_ik - U_i0 * L_k0 - ... - U_i,k-1 * L_k,k-1 (left to right), L_ik = U_ik / D_k;
// D_i = G_ii - U_i0 * L_i0 - ... - U_i,i-1 * L_i,i-1 (left to right).  Pivot i is ACCEPTED when D_i > rcond_min * G_ii (a NaN
// fails); the fit is truncated at the first rejected pivot, n_used = the number of accepted leading pivots.  Then
// y_i = b_i - L_i0 * y_0 - ... - L_i,i-1 * y_i-1 for i < n_used, and from i = n_used - 1 down
// c_i = y_i / D_i - L_i+1,i * c_i+1 - ... - L_nu-1,i * c_nu-1 (left to right); c_i = +0.0 for i >= n_used.
//
// THE SECOND PASS (fit_model), over every sample of the item, live or not:  f = c_0 * B_0, then f = f + c_n * B_n for n = 1 .. NP - 1
// in order, and out = d - f.  With n_used = 0 out = d, the bits copied (and not written at all when out is d).  out may be exactly
// d: a sample is read and written by the same lane, and every first-pass read of an item precedes its first write.

template <int NP_>
struct Fit {
    static constexpr int NP = NP_;                      // coefficients
    static constexpr int NG = NP * (NP + 1) / 2;        // moments G_ik, i >= k, at fit_idx(i, k)
    static constexpr int NV = NG + NP;                  // a lane's sums
};
__device__ __forceinline__ constexpr int fit_idx(int i, int k) { return i * (i + 1) / 2 + k; }

// item sp of n_items + 2: 0 the samples before the first offset, s + 1 fitted item s, n_items + 1 the rest
struct FitSpan {
    int64_t lo, hi;
    bool fit;
};
__device__ __forceinline__ FitSpan fit_span(int64_t sp, const int64_t* __restrict__ offsets, int64_t n_items, int64_t n_axis) {
    int64_t lo = sp == 0 ? 0 : offsets[sp - 1];
    int64_t hi = sp == n_items + 1 ? n_axis : offsets[sp];
    lo = lo < 0 ? 0 : lo > n_axis ? n_axis : lo;
    hi = hi < lo ? lo : hi > n_axis ? n_axis : hi;
    return {lo, hi, sp >= 1 && sp <= n_items};
}

// LDL^T in place in g (L below the diagonal, D on it, for the rows that were reached), then the two substitutions.  Returns n_used.
template <int NP>
__device__ __forceinline__ int fit_solve(double (&g)[Fit<NP>::NG], const double (&b)[NP], double rmin, double (&c)[NP]) {
    int nu = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (nu == i) {
            double u[NP];
            const double gii = g[fit_idx(i, i)];
            double dd = gii;
#pragma unroll
            for (int k = 0; k < i; ++k) {
                double s = g[fit_idx(i, k)];
#pragma unroll
                for (int m = 0; m < k; ++m) s = s - u[m] * g[fit_idx(k, m)];
                u[k] = s;
                const double l = s / g[fit_idx(k, k)];
                g[fit_idx(i, k)] = l;
                dd = dd - s * l;
            }
            g[fit_idx(i, i)] = dd;
            if (dd > rmin * gii) nu = i + 1;
        }
    }
    double y[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        double s = b[i];
#pragma unroll
        for (int m = 0; m < i; ++m) s = s - g[fit_idx(i, m)] * y[m];
        y[i] = s;                                                           // rows from n_used on are never read
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        double s = 0.0;
        if (i < nu) {
            s = y[i] / g[fit_idx(i, i)];
#pragma unroll
            for (int m = i + 1; m < NP; ++m)
                if (m < nu) s = s - g[fit_idx(m, i)] * c[m];
        }
        c[i] = s;
    }
    return nu;
}

// the model's value at one sample
template <int NP, class Basis>
__device__ __forceinline__ double fit_model(const double (&c)[NP], const Basis& B) {
    double f = c[0] * B[0];
#pragma unroll
    for (int n = 1; n < NP; ++n) f = f + c[n] * B[n];
    return f;
}
