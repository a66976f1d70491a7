// pxl_polsolve.h -- the per-pixel IQU block solve and block product: the symmetric 3 x 3 system that the six
// weight planes II IQ IU QQ QU UU of k_scatter_pol_*<6> hold for every pixel, solved against a three-plane right-hand side,
// ill-conditioned pixels masked and their conditioning reported; included by pxl_kernels.hip after pxl_pol.h (one translation
// unit, -ffp-contract=off).
//
// The arithmetic is the contract of include/pixell_hip.h and tests/polsolve_ref.py restates it operation by operation: LDL^T with
// diagonal pivoting, every operation one IEEE rounding, no fma, no transcendental.  The permutation is a handful of selects on
// named scalars: a runtime-indexed local array goes to scratch silently (NOTES).  Both kernels are streams: 96 B read and 24 B
// (or 32 B with the rcond plane) written per pixel, eight divisions.
#pragma once

struct PolSolved { double x0, x1, x2, rc; };

// one pixel; a b c d e f = II IQ IU QQ QU UU
__device__ __forceinline__ PolSolved pol_block_solve1(double a, double b, double c, double d, double e, double f, double r0, double r1,
                                                      double r2, double rcond_min) {
    // first pivot: the largest diagonal entry, the first of equals; the other two keep their order
    const bool f0 = (a >= d) && (a >= f), f1 = !f0 && (d >= f);
    const double m11 = f0 ? a : (f1 ? d : f);
    const double m21 = f0 ? b : (f1 ? b : c);
    const double m31 = f0 ? c : e;
    const double m22 = f0 ? d : a;
    const double m32 = f0 ? e : (f1 ? c : b);
    const double m33 = f0 ? f : (f1 ? f : d);
    const double R1 = f0 ? r0 : (f1 ? r1 : r2);
    double R2 = f0 ? r1 : r0;
    double R3 = f0 ? r2 : (f1 ? r2 : r1);
    // first elimination
    const double p1 = m11;
    double l21 = m21 / p1, l31 = m31 / p1;
    double s22 = m22 - l21 * m21;
    double s33 = m33 - l31 * m31;
    const double s32 = m32 - l31 * m21;
    // second pivot
    const bool swap = s33 > s22;
    if (swap) {
        double t = s22; s22 = s33; s33 = t;
        t = l21; l21 = l31; l31 = t;
        t = R2; R2 = R3; R3 = t;
    }
    // second elimination
    const double p2 = s22;
    const double l32 = s32 / p2;
    const double p3 = s33 - l32 * s32;
    // conditioning: every comparison is false on NaN
    const double rc2 = p2 / p1, rc3 = p3 / p1;
    const double rc = (rc3 < rc2) ? rc3 : rc2;
    const bool fin = isfinite(r0) && isfinite(r1) && isfinite(r2);
    const bool ok = fin && (p1 > 0) && (rc2 >= rcond_min) && (rc3 >= rcond_min);
    const bool pos = fin && (p1 > 0) && (rc2 > 0) && (rc3 > 0);
    // solve
    const double y1 = R1;
    const double y2 = R2 - l21 * y1;
    const double y3 = (R3 - l31 * y1) - l32 * y2;
    const double x3 = y3 / p3;
    const double x2 = y2 / p2 - l32 * x3;
    const double x1 = (y1 / p1 - l21 * x2) - l31 * x3;
    // un-permute: the permutation is (0,1,2) (1,0,2) (2,0,1), its last two entries exchanged by `swap`
    const double xa = swap ? x3 : x2, xb = swap ? x2 : x3;        // the earlier and the later of the two remaining planes
    PolSolved s;
    s.x0 = ok ? (f0 ? x1 : xa) : 0.0;
    s.x1 = ok ? (f0 ? xa : (f1 ? x1 : xb)) : 0.0;
    s.x2 = ok ? ((f0 || f1) ? xb : x1) : 0.0;
    s.rc = pos ? rc : 0.0;
    return s;
}

// VEC: a lane carries two adjacent pixels, every plane access 16 bytes (npix even, every base 16-byte aligned: the host checks);
// else one pixel per lane.  `items` is npix / 2 or npix.  All nine plane loads of a trip are issued before the arithmetic.  out
// may be exactly rhs: a lane reads its pixels before it writes them, so those two carry no __restrict__.
template <bool VEC, bool RCOND>
__global__ __launch_bounds__(256) void k_pol_block_solve(const double* __restrict__ w, const double* rhs, double* out,
                                                         double* __restrict__ rcond, int64_t npix, int64_t items, double rcond_min) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
        if (VEC) {
            const double2 a = *reinterpret_cast<const double2*>(w + 2 * i), b = *reinterpret_cast<const double2*>(w + npix + 2 * i),
                          c = *reinterpret_cast<const double2*>(w + 2 * npix + 2 * i), d = *reinterpret_cast<const double2*>(w + 3 * npix + 2 * i),
                          e = *reinterpret_cast<const double2*>(w + 4 * npix + 2 * i), f = *reinterpret_cast<const double2*>(w + 5 * npix + 2 * i),
                          r0 = *reinterpret_cast<const double2*>(rhs + 2 * i), r1 = *reinterpret_cast<const double2*>(rhs + npix + 2 * i),
                          r2 = *reinterpret_cast<const double2*>(rhs + 2 * npix + 2 * i);
            const PolSolved s = pol_block_solve1(a.x, b.x, c.x, d.x, e.x, f.x, r0.x, r1.x, r2.x, rcond_min);
            const PolSolved t = pol_block_solve1(a.y, b.y, c.y, d.y, e.y, f.y, r0.y, r1.y, r2.y, rcond_min);
            *reinterpret_cast<double2*>(out + 2 * i) = make_double2(s.x0, t.x0);
            *reinterpret_cast<double2*>(out + npix + 2 * i) = make_double2(s.x1, t.x1);
            *reinterpret_cast<double2*>(out + 2 * npix + 2 * i) = make_double2(s.x2, t.x2);
            if (RCOND) *reinterpret_cast<double2*>(rcond + 2 * i) = make_double2(s.rc, t.rc);
        } else {
            const double a = w[i], b = w[npix + i], c = w[2 * npix + i], d = w[3 * npix + i], e = w[4 * npix + i], f = w[5 * npix + i],
                         r0 = rhs[i], r1 = rhs[npix + i], r2 = rhs[2 * npix + i];
            const PolSolved s = pol_block_solve1(a, b, c, d, e, f, r0, r1, r2, rcond_min);
            out[i] = s.x0;
            out[npix + i] = s.x1;
            out[2 * npix + i] = s.x2;
            if (RCOND) rcond[i] = s.rc;
        }
    }
}

// the block product y = A x, each row (m0 * x0 + m1 * x1) + m2 * x2
__device__ __forceinline__ void pol_block_apply1(double a, double b, double c, double d, double e, double f, double x0, double x1, double x2,
                                                 double* y0, double* y1, double* y2) {
    *y0 = (a * x0 + b * x1) + c * x2;
    *y1 = (b * x0 + d * x1) + e * x2;
    *y2 = (c * x0 + e * x1) + f * x2;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_pol_block_apply(const double* __restrict__ w, const double* x, double* out, int64_t npix,
                                                         int64_t items) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
        if (VEC) {
            const double2 a = *reinterpret_cast<const double2*>(w + 2 * i), b = *reinterpret_cast<const double2*>(w + npix + 2 * i),
                          c = *reinterpret_cast<const double2*>(w + 2 * npix + 2 * i), d = *reinterpret_cast<const double2*>(w + 3 * npix + 2 * i),
                          e = *reinterpret_cast<const double2*>(w + 4 * npix + 2 * i), f = *reinterpret_cast<const double2*>(w + 5 * npix + 2 * i),
                          x0 = *reinterpret_cast<const double2*>(x + 2 * i), x1 = *reinterpret_cast<const double2*>(x + npix + 2 * i),
                          x2 = *reinterpret_cast<const double2*>(x + 2 * npix + 2 * i);
            double2 y0, y1, y2;
            pol_block_apply1(a.x, b.x, c.x, d.x, e.x, f.x, x0.x, x1.x, x2.x, &y0.x, &y1.x, &y2.x);
            pol_block_apply1(a.y, b.y, c.y, d.y, e.y, f.y, x0.y, x1.y, x2.y, &y0.y, &y1.y, &y2.y);
            *reinterpret_cast<double2*>(out + 2 * i) = y0;
            *reinterpret_cast<double2*>(out + npix + 2 * i) = y1;
            *reinterpret_cast<double2*>(out + 2 * npix + 2 * i) = y2;
        } else {
            const double a = w[i], b = w[npix + i], c = w[2 * npix + i], d = w[3 * npix + i], e = w[4 * npix + i], f = w[5 * npix + i],
                         x0 = x[i], x1 = x[npix + i], x2 = x[2 * npix + i];
            double y0, y1, y2;
            pol_block_apply1(a, b, c, d, e, f, x0, x1, x2, &y0, &y1, &y2);
            out[i] = y0;
            out[npix + i] = y1;
            out[2 * npix + i] = y2;
        }
    }
}
