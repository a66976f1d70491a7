// fastmath_device.hip -- the DEVICE build of pixell.jl_amd/csrc/pxl_fastmath.h (the hardware v_rcp_f64 / v_rsq_f64 seeds, the
// inline-asm v_fma_f64 with scalar operands, the compile-time specialisations) per element against long double libm on the host,
// for the sample sets of fastmath_check.cpp (same generators, same seed).  Built and run by tests/test_fastmath.py on the GPU;
// prints one JSON object with the keys of fastmath_check.cpp.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -I pixell.jl_amd/csrc tests/native/fastmath_device.hip
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pxl_fastmath.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("{\"error\": \"%s: %s\"}\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

enum { M_ATAN2 = 0, M_ASIN, M_ASIN_W, M_RSQRT, M_SINCOS };

// one element per thread; every store is a plain (vector) store of this thread's own element
__global__ void k_eval(int mode, int64_t n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o0,
                       double* __restrict__ o1, double* __restrict__ o2) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double x = a[k], y = b[k];
    double r0 = 0, r1 = 0, r2 = 0;
    if (mode == M_ATAN2) {                         // atan2(x, y); the TAME form where its precondition holds
        r0 = pxl_fm_atan2(x, y);
        const bool tame = pxl_fm_atan2_is_tame(x, y);
        r1 = tame ? pxl_fm_atan2<true>(x, y) : r0;
        r2 = tame ? 1.0 : 0.0;
    } else if (mode == M_ASIN) {                   // asin(x); the one-half forms
        r0 = pxl_fm_asin(x);
        r1 = __builtin_fabs(x) <= 0.5 ? pxl_fm_asin<1>(x) : pxl_fm_asin<2>(x);
    } else if (mode == M_ASIN_W) {                 // asin_w(x, w = y); the big-half form
        r0 = pxl_fm_asin_w(x, y);
        r1 = __builtin_fabs(x) > 0.5 ? pxl_fm_asin_w<2>(x, y) : r0;
        r2 = pxl_fm_asin_w(x, pxl_fm_lift_tiny_negative(__builtin_fma(-0.5, __builtin_fabs(x), 0.5)));
    } else if (mode == M_RSQRT) {
        r0 = pxl_fm_rsqrt(x);
    } else {
        double s = 7, c = 7;
        r2 = pxl_fm_sincos(x, &s, &c) ? 1.0 : 0.0;
        r0 = s;
        r1 = c;
    }
    o0[k] = r0;
    o1[k] = r1;
    o2[k] = r2;
}

struct Out { std::vector<double> r0, r1, r2; };
static Out run(int mode, const std::vector<double>& a, const std::vector<double>& b_in) {
    const int64_t n = (int64_t)a.size();
    std::vector<double> b = b_in.empty() ? std::vector<double>(a.size(), 0.0) : b_in;
    double *da, *db, *d0, *d1, *d2;
    const size_t bytes = (size_t)n * sizeof(double);
    CHECK(hipMalloc(&da, bytes)); CHECK(hipMalloc(&db, bytes));
    CHECK(hipMalloc(&d0, bytes)); CHECK(hipMalloc(&d1, bytes)); CHECK(hipMalloc(&d2, bytes));
    CHECK(hipMemcpy(da, a.data(), bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(db, b.data(), bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, mode, n, da, db, d0, d1, d2);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    Out o{std::vector<double>(n), std::vector<double>(n), std::vector<double>(n)};
    CHECK(hipMemcpy(o.r0.data(), d0, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(o.r1.data(), d1, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(o.r2.data(), d2, bytes, hipMemcpyDeviceToHost));
    CHECK(hipFree(da)); CHECK(hipFree(db)); CHECK(hipFree(d0)); CHECK(hipFree(d1)); CHECK(hipFree(d2));
    return o;
}

static double ulp_of(long double v) {
    double d = std::fabs((double)v);
    if (d < 2.2250738585072014e-308) return 4.9406564584124654e-324;
    int e;
    std::frexp(d, &e);
    return std::ldexp(1.0, e - 53);
}
static double err_ulp(double got, long double want) {
    if (std::isnan(got) || std::isnan((double)want)) return (std::isnan(got) && std::isnan((double)want)) ? 0.0 : 1e30;
    return (double)(fabsl((long double)got - want) / (long double)ulp_of(want));
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 4000000;
    // ---- the sample sets of fastmath_check.cpp, drawn in its order from the same generator
    std::mt19937_64 rng(20261004);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> ay, ax, av, wv_v, wv_w, ru;
    for (long k = 0; k < n; ++k) {
        double ang = (k & 1) ? (U(rng) * 2 - 1) * M_PI : std::round(U(rng) * 64) * (M_PI / 32) + (U(rng) - 0.5) * 1e-6;
        if ((k & 7) == 3) ang = std::atan(0.75) + (U(rng) - 0.5) * 1e-9;
        if ((k & 7) == 5) ang = M_PI / 8 + (U(rng) - 0.5) * 1e-9;
        double rad = std::exp2((U(rng) - 0.5) * 600);
        ay.push_back(rad * std::sin(ang));
        ax.push_back(rad * std::cos(ang));
        double v = U(rng) * 2 - 1;
        if ((k & 3) == 1) v = std::copysign(0.5 + (U(rng) - 0.5) * 1e-3, v);
        if ((k & 3) == 2) v = std::copysign(1.0 - U(rng) * U(rng) * 1e-2, v);
        if ((k & 15) == 7) v = std::exp2(-U(rng) * 60) * (v < 0 ? -1 : 1);
        av.push_back(v);
        double w = (k & 1) ? U(rng) * 0.25 : 0.25 * std::exp2(-U(rng) * 60);
        const double sgn = (k & 2) ? -1.0 : 1.0;
        wv_v.push_back(sgn * (1.0 - 2.0 * w));
        wv_w.push_back(w);
        double uu = std::exp2((U(rng) - 0.5) * 200);
        if (k & 1) uu = 1.0 + U(rng) * 3;
        ru.push_back(uu);
    }
    std::vector<double> xs_small, xs_big;
    for (long k = 0; k < n; ++k) {
        double xs = (U(rng) * 2 - 1) * 8;
        if ((k & 3) == 1) xs = std::round((U(rng) * 2 - 1) * 16) * (M_PI / 2) + (U(rng) - 0.5) * std::exp2(-U(rng) * 30);
        xs_small.push_back(xs);
        xs_big.push_back((U(rng) * 2 - 1) * 823549.0);
    }
    std::vector<double> xs_near;
    {
        const long double pio2l = 1.57079632679489661923132169163975144L;
        for (long k = 1; k <= 524287; ++k) {
            const double xc = (double)(k * pio2l);
            for (double xs : {xc, std::nextafter(xc, 0.0), std::nextafter(xc, 1e9), -xc}) xs_near.push_back(xs);
        }
    }
    // special arguments
    const double inf = INFINITY, nan = NAN;
    const double sp[] = {0.0, -0.0, 1.0, -1.0, inf, -inf, nan, 5e-324, -5e-324, 1e308, -1e308, 0.5, 0.75, 2.0};
    std::vector<double> spy, spx;
    for (double y : sp) for (double x : sp) { spy.push_back(y); spx.push_back(x); }
    const std::vector<double> sat = {1.0000000000000002, -1.0000000000000002, 1.0000000000000004, 1.0 + 0x1p-49, -(1.0 + 0x1p-49)};
    const std::vector<double> beyond = {1.0 + 0x1p-48, -(1.0 + 0x1p-48), 1.00000001, -1.00000001, 2.0};
    const std::vector<double> asp = {0.0, -0.0, 1.0, -1.0, 0.5, -0.5, -1.5, inf, nan, 5e-324, 1e-200};

    // ---- device
    const Out o_at = run(M_ATAN2, ay, ax), o_as = run(M_ASIN, av, {}), o_w = run(M_ASIN_W, wv_v, wv_w), o_r = run(M_RSQRT, ru, {});
    const Out o_ss = run(M_SINCOS, xs_small, {}), o_sb = run(M_SINCOS, xs_big, {}), o_sn = run(M_SINCOS, xs_near, {});
    const Out o_spa = run(M_ATAN2, spy, spx), o_sat = run(M_ASIN, sat, {}), o_bey = run(M_ASIN, beyond, {}), o_asp = run(M_ASIN, asp, {});
    const Out o_sch = run(M_SINCOS, {1e6, inf, nan, 0.0}, {}), o_rsp = run(M_RSQRT, {inf, nan, 4.0}, {});

    // ---- host: long double references
    double e_atan2 = 0, e_asin = 0, e_asin_w = 0, e_rsqrt = 0, e_sin = 0, e_cos = 0, e_sin_big = 0, e_cos_big = 0, e_near_abs = 0;
    double w_atan2[2] = {0, 0}, w_asin = 0, w_asin_w = 0, w_rsqrt = 0, w_sin = 0, w_cos = 0, w_near = 0;
    long n_tame = 0, tame_bad = 0, half_bad = 0;
    int special_bad = 0;
    for (long k = 0; k < n; ++k) {
        const double y = ay[k], x = ax[k];
        double e = err_ulp(o_at.r0[k], atan2l((long double)y, (long double)x));
        if (e > e_atan2) { e_atan2 = e; w_atan2[0] = y; w_atan2[1] = x; }
        if (o_at.r2[k] != 0.0) { ++n_tame; if (!same_bits(o_at.r1[k], o_at.r0[k])) ++tame_bad; }
        else if (x > 0 && std::isfinite(y) && std::fmax(std::fabs(x), std::fabs(y)) >= 0x1p-700 && std::fmax(std::fabs(x), std::fabs(y)) <= 0x1p+700) ++tame_bad;
        e = err_ulp(o_as.r0[k], asinl((long double)av[k]));
        if (e > e_asin) { e_asin = e; w_asin = av[k]; }
        if (!same_bits(o_as.r1[k], o_as.r0[k])) ++half_bad;
        if (std::fabs(wv_v[k]) > 0.5) {
            const long double want = (wv_v[k] < 0 ? -1.0L : 1.0L) * (1.57079632679489661923132169163975144L - 2.0L * asinl(sqrtl((long double)wv_w[k])));
            e = err_ulp(o_w.r0[k], want);
            if (e > e_asin_w) { e_asin_w = e; w_asin_w = wv_w[k]; }
            if (!same_bits(o_w.r1[k], o_w.r0[k])) ++half_bad;
        }
        e = err_ulp(o_r.r0[k], 1.0L / sqrtl((long double)ru[k]));
        if (e > e_rsqrt) { e_rsqrt = e; w_rsqrt = ru[k]; }
    }
    // asin_w with w = (1 - |v|) / 2 formed from v is asin itself
    {
        const Out o_wv = run(M_ASIN_W, av, std::vector<double>(av.size(), 0.0));
        for (long k = 0; k < n; ++k) if (!same_bits(o_wv.r2[k], o_as.r0[k])) ++half_bad;
    }
    for (long k = 0; k < n; ++k) {
        if (o_ss.r2[k] == 0.0 || o_sb.r2[k] == 0.0) { printf("{\"error\": \"fast path refused %g\"}\n", o_ss.r2[k] == 0.0 ? xs_small[k] : xs_big[k]); return 1; }
        double es = err_ulp(o_ss.r0[k], sinl((long double)xs_small[k])), ec = err_ulp(o_ss.r1[k], cosl((long double)xs_small[k]));
        if (es > e_sin) { e_sin = es; w_sin = xs_small[k]; }
        if (ec > e_cos) { e_cos = ec; w_cos = xs_small[k]; }
        e_sin_big = std::max(e_sin_big, err_ulp(o_sb.r0[k], sinl((long double)xs_big[k])));
        e_cos_big = std::max(e_cos_big, err_ulp(o_sb.r1[k], cosl((long double)xs_big[k])));
    }
    for (size_t k = 0; k < xs_near.size(); ++k) {
        if (o_sn.r2[k] == 0.0) { printf("{\"error\": \"fast path refused %g\"}\n", xs_near[k]); return 1; }
        const long double xl = (long double)xs_near[k];
        const double ea = (double)std::max(fabsl((long double)o_sn.r0[k] - sinl(xl)), fabsl((long double)o_sn.r1[k] - cosl(xl)));
        if (ea > e_near_abs) { e_near_abs = ea; w_near = xs_near[k]; }
    }
    for (size_t k = 0; k < spy.size(); ++k) {
        const double g = o_spa.r0[k], w = std::atan2(spy[k], spx[k]);
        if (!(same_bits(g, w) || err_ulp(g, atan2l((long double)spy[k], (long double)spx[k])) <= 1.0) || std::signbit(g) != std::signbit(w))
            if (!(std::isnan(g) && std::isnan(w))) { ++special_bad; fprintf(stderr, "atan2(%g, %g) = %a, libm %a\n", spy[k], spx[k], g, w); }
        if (o_spa.r2[k] != 0.0 && !same_bits(o_spa.r1[k], g)) ++tame_bad;
    }
    for (size_t k = 0; k < sat.size(); ++k) {
        const double want = std::copysign(std::asin(1.0), sat[k]);
        for (double g : {o_sat.r0[k], o_sat.r1[k]})
            if (!same_bits(g, want)) { ++special_bad; fprintf(stderr, "asin(%a) = %a, expected the pole %a\n", sat[k], g, want); }
    }
    for (size_t k = 0; k < beyond.size(); ++k)
        for (double g : {o_bey.r0[k], o_bey.r1[k]})
            if (!std::isnan(g)) { ++special_bad; fprintf(stderr, "asin(%a) = %a, expected NaN\n", beyond[k], g); }
    for (size_t k = 0; k < asp.size(); ++k) {
        const double g = o_asp.r0[k], w = std::asin(asp[k]);
        if (!(same_bits(g, w) || err_ulp(g, asinl((long double)asp[k])) <= 1.0) || (!std::isnan(w) && std::signbit(g) != std::signbit(w))) { ++special_bad; fprintf(stderr, "asin(%g) = %a, libm %a\n", asp[k], g, w); }
        if (!same_bits(o_asp.r1[k], g)) ++half_bad;
    }
    if (o_sch.r2[0] != 0.0 || o_sch.r2[1] != 0.0 || o_sch.r2[2] != 0.0 || o_sch.r0[0] != 7 || o_sch.r1[0] != 7) ++special_bad;
    if (!(o_sch.r2[3] != 0.0 && o_sch.r0[3] == 0.0 && o_sch.r1[3] == 1.0)) ++special_bad;
    if (!(std::isnan(o_rsp.r0[0]) && std::isnan(o_rsp.r0[1]) && o_rsp.r0[2] == 0.5)) ++special_bad;
    printf("{\"samples\": %ld, \"atan2_max_ulp\": %.3f, \"atan2_worst\": [%.17g, %.17g], \"asin_max_ulp\": %.3f, \"asin_worst\": %.17g, "
           "\"sin_max_ulp\": %.3f, \"sin_worst\": %.17g, \"cos_max_ulp\": %.3f, \"cos_worst\": %.17g, \"sin_max_ulp_big\": %.3f, \"cos_max_ulp_big\": %.3f, \"rsqrt_max_ulp\": %.3f, "
           "\"rsqrt_worst\": %.17g, \"asin_w_max_ulp\": %.3f, \"asin_w_worst\": %.17g, \"tame_samples\": %ld, \"tame_bad\": %ld, \"asin_half_bad\": %ld, \"special_bad\": %d, \"sincos_near_kpio2_max_abs\": %.4g, \"sincos_near_kpio2_worst\": %.17g}\n",
           n, e_atan2, w_atan2[0], w_atan2[1], e_asin, w_asin, e_sin, w_sin, e_cos, w_cos, e_sin_big, e_cos_big, e_rsqrt, w_rsqrt, e_asin_w, w_asin_w, n_tame, tame_bad, half_bad, special_bad, e_near_abs, w_near);
    return 0;
}
