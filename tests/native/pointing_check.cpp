// pointing_check.cpp -- accuracy of pxl_pointing_sample (pixell.jl_amd/csrc/pxl_pointing.h) on the host against the definition
// of include/pixell_hip.h written out literally in long double (x87: 64-bit significand).  The header is the text the device
// compiles, with pxl_fastmath.h's 24-bit stand-ins for the two hardware seeds.  Built and run by tests/test_pointing_native.py:
//   g++ -O2 -std=c++17 -ffp-contract=off -I pixell.jl_amd/csrc tests/native/pointing_check.cpp -o /tmp/pointing_check
//   pointing_check [n [dump.bin]]      n random unnormalised pairs + n / 4 polar samples; dump.bin receives the samples, nine
//                                      doubles each (q_bore, q_det, gamma), so that the numpy yardstick can run on the same inputs
// Prints one JSON line: the worst position error (great-circle separation, units of 2^-52 rad) and the worst response error
// (max(|dq|, |du|) in units of 2^-52 gamma / h), each for the random and the polar set, and the count of special values answered wrongly.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#define PXL_FM_HD static inline
#include "pxl_fastmath.h"
#include "pxl_pointing.h"

typedef long double LD;
struct Out { double ra, dec, q, u; };

static Out device_text(const double* s) {
    const bool bad = pxl_pointing_bad4(s[0], s[1], s[2], s[3]) || pxl_pointing_bad4(s[4], s[5], s[6], s[7]) || pxl_pointing_bad4(s[8], 1.0, 1.0, 1.0);
    Out o;
    pxl_pointing_sample(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], bad, &o.ra, &o.dec, &o.q, &o.u);
    return o;
}

// the definition, literally: rotate z^ and x^, build east and north, project.  h_out: h of the unit line of sight
static void truth(const double* s, LD* ra, LD* dec, LD* q, LD* u, LD* h_out) {
    const LD bw = s[0], bx = s[1], by = s[2], bz = s[3], dw = s[4], dx = s[5], dy = s[6], dz = s[7], g = s[8];
    const LD w = bw * dw - bx * dx - by * dy - bz * dz, x = bw * dx + bx * dw + by * dz - bz * dy;
    const LD y = bw * dy - bx * dz + by * dw + bz * dx, z = bw * dz + bx * dy - by * dx + bz * dw;
    const LD n[3] = {2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z};
    const LD e[3] = {w * w + x * x - y * y - z * z, 2 * (x * y + w * z), 2 * (x * z - w * y)};
    const LD h = sqrtl(n[0] * n[0] + n[1] * n[1]), nn = sqrtl(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const bool pole = h == 0;
    *ra = pole ? 0.0L : atan2l(n[1] + 0.0L, n[0]);
    *dec = atan2l(n[2], h);
    const LD E[3] = {pole ? 0.0L : -n[1] / h, pole ? 1.0L : n[0] / h, 0.0L};
    const LD nh[3] = {n[0] / nn, n[1] / nn, n[2] / nn};
    const LD N[3] = {nh[1] * E[2] - nh[2] * E[1], nh[2] * E[0] - nh[0] * E[2], nh[0] * E[1] - nh[1] * E[0]};
    const LD c = e[0] * N[0] + e[1] * N[1] + e[2] * N[2], sn = e[0] * E[0] + e[1] * E[1] + e[2] * E[2];
    const LD d = c * c + sn * sn;
    *q = g * (c * c - sn * sn) / d;
    *u = g * (2 * c * sn) / d;
    *h_out = h / nn;
}

static const LD EPS = 0x1p-52L;
static void errors(const double* s, double* pos, double* resp) {
    const Out o = device_text(s);
    LD ra, dec, q, u, h;
    truth(s, &ra, &dec, &q, &u, &h);
    const LD v[3] = {cosl((LD)o.dec) * cosl((LD)o.ra) - cosl(dec) * cosl(ra), cosl((LD)o.dec) * sinl((LD)o.ra) - cosl(dec) * sinl(ra),
                     sinl((LD)o.dec) - sinl(dec)};
    *pos = (double)(2 * asinl(sqrtl(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / 2) / EPS);
    const LD err = fmaxl(fabsl((LD)o.q - q), fabsl((LD)o.u - u));
    *resp = s[8] == 0.0 ? (err == 0 ? 0.0 : 1e300) : (double)(err * h / (EPS * fabsl((LD)s[8])));
    if (!(*pos == *pos)) *pos = 1e300;                   // a NaN where the truth has a number
    if (!(*resp == *resp)) *resp = 1e300;
}

static void quat_mul(const double* a, const double* b, double* r) {
    r[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    r[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    r[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    r[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
// Rz(ra) (x) Ry(pi/2 - dec) (x) Rz(pi - psi)
static void quat_from_radec(double ra, double dec, double psi, double* q) {
    const double t = (M_PI / 2 - dec) / 2;
    const double a[4] = {std::cos(ra / 2), 0, 0, std::sin(ra / 2)}, b[4] = {std::cos(t), 0, std::sin(t), 0};
    const double c[4] = {std::cos((M_PI - psi) / 2), 0, 0, std::sin((M_PI - psi) / 2)};
    double ab[4];
    quat_mul(a, b, ab);
    quat_mul(ab, c, q);
}

static bool is_plus_zero(double v) { return v == 0.0 && !std::signbit(v); }

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 800000;
    const long npolar = n / 4;
    std::mt19937_64 rng(20261019);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> G(0.0, 1.0);
    std::vector<double> samples((size_t)(n + npolar) * 9);
    auto random_quat = [&](double* q) {
        double nrm = 0;
        for (int i = 0; i < 4; ++i) { q[i] = G(rng); nrm += q[i] * q[i]; }
        const double sc = (0.5 + 1.5 * U(rng)) / std::sqrt(nrm);
        for (int i = 0; i < 4; ++i) q[i] *= sc;
    };
    double worst[4] = {0, 0, 0, 0};                      // position, response: random set; position, response: polar set
    double worst_at[4][9] = {};
    for (long k = 0; k < n + npolar; ++k) {
        double* s = &samples[(size_t)k * 9];
        if (k < n) {
            random_quat(s);
            random_quat(s + 4);
            s[8] = (k & 1) ? 1.0 : U(rng);
        } else {                                         // within h of a pole, h log-uniform in [1e-12, 1e-1]; the detector looks along the boresight,
            const double h = std::exp(std::log(1e-12) + U(rng) * (std::log(1e-1) - std::log(1e-12)));
            quat_from_radec((U(rng) * 2 - 1) * M_PI, ((k & 1) ? 1.0 : -1.0) * (M_PI / 2 - h), (U(rng) * 2 - 1) * M_PI, s);
            const double sc = 0.5 + 1.5 * U(rng), sd = 0.5 + 1.5 * U(rng);
            for (int i = 0; i < 4; ++i) s[i] *= sc;
            s[4] = sd; s[5] = s[6] = s[7] = 0.0;
            s[8] = 1.0;
            if (k & 2) {                                 // or anywhere else, the boresight being what brings it to the pole: q_b = q (x) conj(q_d)
                double qd[4], qp[4] = {s[0], s[1], s[2], s[3]};
                random_quat(qd);
                const double cj[4] = {qd[0], -qd[1], -qd[2], -qd[3]};
                quat_mul(qp, cj, s);
                std::memcpy(s + 4, qd, 32);
                s[8] = U(rng);
            }
        }
        double pos, resp;
        errors(s, &pos, &resp);
        const int set = k < n ? 0 : 2;
        if (pos > worst[set]) { worst[set] = pos; std::memcpy(worst_at[set], s, 72); }
        if (resp > worst[set + 1]) { worst[set + 1] = resp; std::memcpy(worst_at[set + 1], s, 72); }
    }
    if (argc > 2) {
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(samples.data(), 8, samples.size(), f) != samples.size()) { std::printf("{\"error\": \"cannot write %s\"}\n", argv[2]); return 1; }
        std::fclose(f);
    }

    // special values
    int special_bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { ++special_bad; std::fprintf(stderr, "special: %s\n", what); } };
    const double nan = std::nan(""), inf = INFINITY;
    {
        // the poles: ra = +0.0 by bits, dec = +-pi/2, psi = pi - a for q = Rz(a) at the north pole
        const double a = 0.3;
        const double north[9] = {1.5 * std::cos(a / 2), 0, 0, 1.5 * std::sin(a / 2), 1, 0, 0, 0, 0.5};
        Out o = device_text(north);
        expect(is_plus_zero(o.ra) && std::fabs(o.dec - M_PI / 2) < 3e-16, "north pole position");
        expect(std::fabs(o.q - 0.5 * std::cos(2 * (M_PI - a))) < 1e-15 && std::fabs(o.u - 0.5 * std::sin(2 * (M_PI - a))) < 1e-15, "north pole response");
        const double south[9] = {0, 1, 0, 0, 1, 0, 0, 0, 1};
        o = device_text(south);
        expect(is_plus_zero(o.ra) && std::fabs(o.dec + M_PI / 2) < 3e-16, "south pole position");
        LD ra, dec, q, u, h;
        truth(south, &ra, &dec, &q, &u, &h);
        expect(std::fabs(o.q - (double)q) < 1e-15 && std::fabs(o.u - (double)u) < 1e-15, "south pole response");
        const double minus_zero[9] = {1, -0.0, -0.0, 1, 1, 0, 0, 0, 1};          // n_x = -0.0, n_y = +0.0: atan2 alone answers pi
        o = device_text(minus_zero);
        expect(is_plus_zero(o.ra) && o.dec > 1.5, "pole with n_x = -0.0");
        for (int bits = 0; bits < 32; ++bits) {                                  // every signed-zero form of a polar boresight
            const double sg[4] = {bits & 1 ? -1.0 : 1.0, bits & 2 ? -1.0 : 1.0, bits & 4 ? -1.0 : 1.0, bits & 8 ? -1.0 : 1.0};
            const double one = bits & 16 ? 0.0 : 1.0, other = 1.0 - one;
            const double s[9] = {sg[0] * one, sg[1] * other, sg[2] * other, sg[3] * one, 1, 0, 0, 0, 1};
            o = device_text(s);
            expect(is_plus_zero(o.ra) && std::fabs(std::fabs(o.dec) - M_PI / 2) < 3e-16 && (o.dec > 0) == (one == 1.0), "a signed-zero form of the pole");
        }
        const double cut[9] = {1, 0, -1, -0.0, 1, 0, 0, 0, 1};                   // n = (-2, -0.0, 0): ra = +pi, never -pi
        o = device_text(cut);
        expect(o.ra == M_PI && is_plus_zero(o.dec), "ra = +pi on the branch cut");
        const double dead[9] = {0.3, -0.2, 0.5, 0.7, 0.9, 0.1, -0.4, 0.2, 0.0};  // gamma = 0: response 0, position stands
        o = device_text(dead);
        expect(o.q == 0.0 && o.u == 0.0 && std::isfinite(o.ra) && std::isfinite(o.dec), "gamma = 0");
    }
    const double vals[3] = {nan, inf, -inf};
    for (int slot = 0; slot < 9; ++slot)
        for (double v : vals) {
            double s[9] = {0.3, -0.2, 0.5, 0.7, 0.9, 0.1, -0.4, 0.2, 0.8};
            s[slot] = v;
            const Out o = device_text(s);
            expect(std::isnan(o.ra) && std::isnan(o.dec) && std::isnan(o.q) && std::isnan(o.u), "a NaN or Inf component makes the sample NaN");
        }
    for (int which = 0; which < 2; ++which) {
        double s[9] = {0.3, -0.2, 0.5, 0.7, 0.9, 0.1, -0.4, 0.2, 0.8};
        for (int i = 0; i < 4; ++i) s[4 * which + i] = (i == 1) ? -0.0 : 0.0;
        const Out o = device_text(s);
        expect(std::isnan(o.ra) && std::isnan(o.dec) && std::isnan(o.q) && std::isnan(o.u), "an all-zero quaternion makes the sample NaN");
    }

    std::printf("{\"n_random\": %ld, \"n_polar\": %ld, \"pos_random\": %.4f, \"resp_random\": %.4f, \"pos_polar\": %.4f, \"resp_polar\": %.4f, "
                "\"special_bad\": %d}\n", n, npolar, worst[0], worst[1], worst[2], worst[3], special_bad);
    for (int i = 0; i < 4; ++i) {
        std::fprintf(stderr, "worst[%d] = %.4f at", i, worst[i]);
        for (int j = 0; j < 9; ++j) std::fprintf(stderr, " %.17g", worst_at[i][j]);
        std::fprintf(stderr, "\n");
    }
    return 0;
}
