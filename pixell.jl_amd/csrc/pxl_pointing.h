// pxl_pointing.h -- detector pointing expansion: boresight quaternions (one per time sample) and detector
// quaternions (one per detector) to the (ra, dec) and the response pairs gamma (cos 2 psi, sin 2 psi) the pointing operators
// consume.  Included by pxl_kernels.hip (one translation unit, -ffp-contract=off) after pxl_fastmath.h and, on the host, by
// tests/native/pointing_check.cpp, which measures pxl_pointing_sample against long double (tests/test_pointing_native.py).
//
// Quaternions are (w, x, y, z), scalar first, R(q) v = q v q*, and need not be normalised: every output is a ratio of
// quantities that scale alike.  With q = q_bore (x) q_det, S = |q|^2, A = w^2 + z^2, B = x^2 + y^2:
//   S n = S R(q) z^ = (2 (xz + wy), 2 (yz - wx), A - B)           the line of sight
//   h^2 = n_x^2 + n_y^2 = 4 A B / S^2
//   c = e . N = e_z / h,  s = e . E = (R(q) y^)_z / h             e = R(q) x^, E = (-n_y, n_x, 0) / h, N = n^ x E  (e . n = 0)
//   S e_z = 2 (xz - wy),  S (R(q) y^)_z = 2 (yz + wx)
// so with the half-scale numbers  nx = xz + wy, ny = yz - wx, a = xz - wy, b = yz + wx  (a^2 + b^2 = nx^2 + ny^2 = A B):
//   ra = atan2(ny, nx),  dec = atan2(A - B, 2 sqrt(nx^2 + ny^2)),  resp = gamma (a^2 - b^2, 2 a b) / (a^2 + b^2).
// Every sum above is of two products of comparable size relative to h: nothing cancels beyond the rounding of q itself, which
// is the 1 / h conditioning of a position angle next to a pole.  No trigonometric function, two atan2 and one square root.
#pragma once

#ifndef PXL_FM_HD
#define PXL_FM_HD __host__ __device__ inline
#endif

// a quaternion (or gamma, passed four times) the expansion refuses: a component that is NaN or Inf, or all four zero.  Integer
// tests on the bit patterns: for a detector's quaternion, uniform over a block, they stay off the vector FP64 pipe.
PXL_FM_HD bool pxl_pointing_bad4(double w, double x, double y, double z) {
    unsigned long long b[4];
    __builtin_memcpy(&b[0], &w, 8); __builtin_memcpy(&b[1], &x, 8); __builtin_memcpy(&b[2], &y, 8); __builtin_memcpy(&b[3], &z, 8);
    bool nonfinite = false;
    unsigned long long any = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nonfinite |= ((b[i] >> 52) & 0x7ffull) == 0x7ffull;
        any |= b[i] << 1;                                       // the sign does not make a zero a number
    }
    return nonfinite || any == 0;
}

// One sample: boresight (bw, bx, by, bz), detector (dw, dx, dy, dz), polarisation efficiency gamma; `bad`: the caller found a
// refused input (pxl_pointing_bad4 of either quaternion, a non-finite gamma) and all four outputs are NaN.
//   q      the Hamilton product, each component three fma on one product
//   pole   h2 = nx^2 + ny^2 == 0 as computed: ra = +0.0, dec = +-pi/2 (atan2(nz, 0)), E = (0, 1, 0), N = n^ x E = (-+1, 0, 0), so
//          c = -sign(n_z) e_x and s = e_y, with S e_x = w^2 + x^2 - y^2 - z^2 and S e_y = 2 (xy + wz)
//   ra     ny + 0.0 turns a -0.0 into +0.0, so atan2 answers +pi and never -pi: (-pi, pi]
//   rs     1 / sqrt(a^2 + b^2) once: (a rs, b rs) is the unit vector (cos psi, sin psi), and sqrt(h2) = h2 rs with one correction step
PXL_FM_HD void pxl_pointing_sample(double bw, double bx, double by, double bz, double dw, double dx, double dy, double dz, double gamma,
                                   bool bad, double* ra, double* dec, double* rq, double* ru) {
    const double w = __builtin_fma(-bz, dz, __builtin_fma(-by, dy, __builtin_fma(-bx, dx, bw * dw)));
    const double x = __builtin_fma(-bz, dy, __builtin_fma(by, dz, __builtin_fma(bx, dw, bw * dx)));
    const double y = __builtin_fma(bz, dx, __builtin_fma(by, dw, __builtin_fma(-bx, dz, bw * dy)));
    const double z = __builtin_fma(bz, dw, __builtin_fma(-by, dx, __builtin_fma(bx, dy, bw * dz)));
    const double wy = w * y, wx = w * x;
    const double nx = __builtin_fma(x, z, wy), ny = __builtin_fma(y, z, -wx);
    double a = __builtin_fma(x, z, -wy), b = __builtin_fma(y, z, wx);
    const double A = __builtin_fma(w, w, z * z), B = __builtin_fma(x, x, y * y);
    const double nz = A - B;
    const double h2 = __builtin_fma(nx, nx, ny * ny);
    const bool pole = h2 == 0.0;
    double d2 = __builtin_fma(a, a, b * b);
    if (pole) {
        const double ex = __builtin_fma(w, w, x * x) - __builtin_fma(y, y, z * z), ey = 2.0 * __builtin_fma(x, y, w * z);
        a = nz > 0.0 ? -ex : ex;
        b = ey;
        d2 = __builtin_fma(a, a, b * b);
    }
    const double rs = pxl_fm_rsqrt(d2);                          // off the pole d2 is h2 up to rounding, and the step below squares that away
    const double h0 = h2 * rs;
    const double hh = __builtin_fma(__builtin_fma(-h0, h0, h2), 0.5 * rs, h0);          // sqrt(h2); 0 at the pole
    const double r = pole ? 0.0 : pxl_fm_atan2(ny + 0.0, nx);
    const double dc = pxl_fm_atan2(nz, hh + hh);
    const double cp = a * rs, sp = b * rs;
    const double q2 = ((cp - sp) * (cp + sp)) * gamma, u2 = ((cp + cp) * sp) * gamma;
    const double nan = __builtin_nan("");
    *ra = bad ? nan : r;
    *dec = bad ? nan : dc;
    *rq = bad ? nan : q2;
    *ru = bad ? nan : u2;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// k_pointing_expand: a write stream of 32 B per sample (posmap's pattern: nothing but 16-byte stores, 1 KiB contiguous per wave
// instruction).  A block takes PXL_PT_BLOCK consecutive time samples, one per lane -- two 16-byte loads of q_bore[t], kept in
// registers -- and loops over a group of PXL_PT_GROUP consecutive detectors, so the boresight is read once per group, not once
// per detector.  q_det[d] and gamma[d] are uniform over the block: the compiler reads them with scalar loads.  Output index
// k = d * nt + t (detector-major).  Blocks are numbered time-fastest, so blocks that run together write the same few rows.
// ------------------------------------------------------------------------------------------------
#define PXL_PT_BLOCK 256
#define PXL_PT_GROUP 8
__global__ __launch_bounds__(PXL_PT_BLOCK) void k_pointing_expand(unsigned block0, int64_t nt, int64_t nd, unsigned ntb, const double2* __restrict__ qbore,
                                                                  const double* __restrict__ qdet, const double* __restrict__ gamma,
                                                                  double2* __restrict__ sky, double2* __restrict__ resp) {
    const unsigned bid = block0 + blockIdx.x;                               // block0: launch_chunks in pxl_kernels.hip
    const unsigned tb = bid % ntb, dg = bid / ntb;
    const int64_t t = (int64_t)tb * PXL_PT_BLOCK + threadIdx.x;
    if (t >= nt) return;
    const double2 b01 = qbore[2 * t], b23 = qbore[2 * t + 1];
    const bool bad_b = pxl_pointing_bad4(b01.x, b01.y, b23.x, b23.y);
    const int64_t d0 = (int64_t)dg * PXL_PT_GROUP, d1 = d0 + PXL_PT_GROUP < nd ? d0 + PXL_PT_GROUP : nd;
    for (int64_t d = d0; d < d1; ++d) {
        const double dw = qdet[4 * d], dx = qdet[4 * d + 1], dy = qdet[4 * d + 2], dz = qdet[4 * d + 3];
        const double g = gamma ? gamma[d] : 1.0;
        const bool bad = bad_b || pxl_pointing_bad4(dw, dx, dy, dz) || pxl_pointing_bad4(g, 1.0, 1.0, 1.0);
        double ra, dec, rq, ru;
        pxl_pointing_sample(b01.x, b01.y, b23.x, b23.y, dw, dx, dy, dz, g, bad, &ra, &dec, &rq, &ru);
        const int64_t k = d * nt + t;
        sky[k] = make_double2(ra, dec);
        resp[k] = make_double2(rq, ru);
    }
}
#endif
