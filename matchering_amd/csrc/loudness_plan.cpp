// Host plan of the loudness meter: see loudness_plan.h.
#include "loudness_plan.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace mgx {
namespace {

typedef long double ld;

// largest root modulus of z^2 + a1 z + a2
double pole_modulus(double a1, double a2) {
    const double disc = a1 * a1 - 4.0 * a2;
    if (disc < 0.0) return std::sqrt(a2);
    const double r = std::sqrt(disc);
    return std::max(std::fabs(-a1 + r), std::fabs(-a1 - r)) * 0.5;
}

void mat_mul(const ld* x, const ld* y, ld* out) {
    ld t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            ld s = 0.0L;
            for (int k = 0; k < 4; ++k) s += x[4 * i + k] * y[4 * k + j];
            t[4 * i + j] = s;
        }
    std::copy(t, t + 16, out);
}

// I0 by its power series (every term positive: no cancellation), as resample_plan.cpp sums it
ld bessel_i0(ld x) {
    const ld q = 0.25L * x * x;
    ld term = 1.0L, sum = 1.0L;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((ld)k * (ld)k);
        const ld next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

const double LOUDNESS_OFFSET = -0.691, ABSOLUTE_GATE = -70.0;
const double MINUS_INF = -std::numeric_limits<double>::infinity();

double lufs(double z) { return z > 0.0 ? LOUDNESS_OFFSET + 10.0 * std::log10(z) : MINUS_INF; }

// mean square of the blocks of `len` sub-blocks that start at sub-blocks 0, step, 2 step, ...
std::vector<double> block_powers(const double* e, int64_t nsub, int S, int len, int step) {
    std::vector<double> z;
    for (int64_t j = 0; j + len <= nsub; j += step) {
        double s = 0.0;
        for (int64_t k = j; k < j + len; ++k) s += e[2 * k] + e[2 * k + 1];
        z.push_back(s / ((double)len * (double)S));
    }
    return z;
}

double largest(const std::vector<double>& z) {
    double m = MINUS_INF;
    for (double v : z) m = std::max(m, lufs(v));
    return m;
}

// the blocks above the absolute gate and above `relative` LU under the loudness of those
std::vector<double> gated(const std::vector<double>& z, double relative) {
    double sum = 0.0;
    int64_t count = 0;
    for (double v : z)
        if (lufs(v) > ABSOLUTE_GATE) {
            sum += v;
            ++count;
        }
    std::vector<double> kept;
    if (count == 0) return kept;
    const double gate = lufs(sum / (double)count) + relative;
    for (double v : z) {
        const double l = lufs(v);
        if (l > ABSOLUTE_GATE && l > gate) kept.push_back(v);
    }
    return kept;
}

}  // namespace

void loudness_true_peak_taps(double* taps49) {
    const ld pi = 3.14159265358979323846264338327950288L;
    const ld i0_beta = bessel_i0(8.0L);
    for (int k = -24; k <= 24; ++k) {
        const ld r = (ld)k / 24.0L;                                         // numpy.kaiser: (n - alpha) / alpha, alpha = 24
        const ld w = bessel_i0(8.0L * std::sqrt(std::max((ld)0.0L, 1.0L - r * r))) / i0_beta;
        const ld at = pi * (ld)k / 4.0L;
        const ld sinc = k == 0 ? 1.0L : (k % 4 == 0 ? 0.0L : std::sin(at) / at);
        taps49[k + 24] = (double)(sinc * w);
    }
}

LoudnessPlan loudness_design(int rate) {
    LoudnessPlan p;
    p.rate = rate;
    const double pi = 3.141592653589793;
    const double fs = (double)rate;
    {   // high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs);
        const double Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        p.c[0] = (Vh + Vb * K / Q + K * K) / a0;
        p.c[1] = 2.0 * (K * K - Vh) / a0;
        p.c[2] = (Vh - Vb * K / Q + K * K) / a0;
        p.c[3] = 2.0 * (K * K - 1.0) / a0;
        p.c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {   // high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        p.c[5] = 1.0;
        p.c[6] = -2.0;
        p.c[7] = 1.0;
        p.c[8] = 2.0 * (K * K - 1.0) / a0;
        p.c[9] = (1.0 - K / Q + K * K) / a0;
    }
    const ld b0 = p.c[0], b1 = p.c[1], b2 = p.c[2], a1 = p.c[3], a2 = p.c[4];
    const ld c0 = p.c[5], c1 = p.c[6], c2 = p.c[7], d1 = p.c[8], d2 = p.c[9];
    // y1 = b0 x + s1, y2 = c0 y1 + t1, and the state updates of loudness_plan.h written out in z and x
    const ld A[16] = {-a1, 1.0L, 0.0L, 0.0L,
                      -a2, 0.0L, 0.0L, 0.0L,
                      c1 - d1 * c0, 0.0L, -d1, 1.0L,
                      c2 - d2 * c0, 0.0L, -d2, 0.0L};
    const ld B[4] = {b1 - a1 * b0, b2 - a2 * b0, (c1 - d1 * c0) * b0, (c2 - d2 * c0) * b0};
    for (int i = 0; i < 16; ++i) p.A[i] = (double)A[i];
    for (int i = 0; i < 4; ++i) p.B[i] = (double)B[i];
    p.rho = std::max(pole_modulus(p.c[3], p.c[4]), pole_modulus(p.c[8], p.c[9]));
    p.warmup_poles = (int)std::ceil(std::log(1.0e-12) / std::log(p.rho));
    // rho^H alone is not the bound: the high-pass's poles are a near-double pair (Q = 0.5003), so A^k decays like
    // k rho^k -- at k = warmup_poles its norm is still 9e-9 at 44.1 kHz.  The warm-up is the first k >= warmup_poles at which
    // the largest row sum of |A^k| itself is down to 1e-12: whatever state a workgroup does not know, this is all that
    // can be left of it when its own sub-blocks begin.
    {
        ld power[16];
        for (int i = 0; i < 16; ++i) power[i] = i % 5 == 0 ? 1.0L : 0.0L;
        for (int k = 1;; ++k) {
            mat_mul(power, A, power);
            ld norm = 0.0L;
            for (int i = 0; i < 4; ++i)
                norm = std::max(norm, std::fabs(power[4 * i]) + std::fabs(power[4 * i + 1]) + std::fabs(power[4 * i + 2]) +
                                          std::fabs(power[4 * i + 3]));
            if ((k >= p.warmup_poles && norm <= 1.0e-12L) || k >= (1 << 24)) {
                p.warmup = k;
                break;
            }
        }
    }

    p.table.assign(LOUD_TABLE_DOUBLES, 0.0);
    double taps[49];
    loudness_true_peak_taps(taps);
    for (int ph = 1; ph <= 3; ++ph)
        for (int i = 0; i < LOUD_TP_TAPS; ++i) {
            // entry i multiplies x[m + LOUD_TP_AFTER - i] = x[m - j] with j = i - LOUD_TP_AFTER: tap h[ph + 4 j]
            const int k = ph + 4 * (i - LOUD_TP_AFTER);
            p.table[LOUD_TABLE_TAPS + (ph - 1) * LOUD_TP_TAPS + i] = taps[k + 24];
        }
    ld power[16];
    std::copy(A, A + 16, power);
    for (int r = LOUD_RUN; r > 1; r >>= 1) mat_mul(power, power, power);    // A^16 by four squarings
    for (int k = 0; k < LOUD_SCAN_STEPS; ++k) {
        for (int i = 0; i < 16; ++i) p.table[LOUD_TABLE_POWERS + 16 * k + i] = (double)power[i];
        mat_mul(power, power, power);
    }
    return p;
}

LoudnessGeometry loudness_geometry(const LoudnessPlan& plan, int64_t n) {
    LoudnessGeometry g;
    g.S = (plan.rate + 5) / 10;
    g.nsub = n / g.S;
    g.warmup = plan.warmup;
    // an 8-minute track: 4800 sub-blocks in 400 workgroups of 12; a 30 s one: 300 workgroups of 1, each with its warm-up
    g.own = (int)std::min<int64_t>(LOUD_OWN, std::max<int64_t>(1, (g.nsub + LOUD_WORKGROUPS - 1) / LOUD_WORKGROUPS));
    g.workgroups = std::max<int64_t>(1, (g.nsub + g.own - 1) / g.own);
    return g;
}

LoudnessGated loudness_gate(const double* e, int64_t nsub, int S) {
    LoudnessGated out;
    const std::vector<double> momentary = block_powers(e, nsub, S, 4, 1);
    const std::vector<double> short_term = block_powers(e, nsub, S, 30, 1);
    out.momentary_max = largest(momentary);
    out.short_term_max = largest(short_term);
    {
        const std::vector<double> kept = gated(momentary, -10.0);
        double sum = 0.0;
        for (double v : kept) sum += v;
        out.integrated = kept.empty() ? MINUS_INF : lufs(sum / (double)kept.size());
    }
    {
        std::vector<double> kept = gated(block_powers(e, nsub, S, 30, 10), -20.0);
        out.range = 0.0;
        if (!kept.empty()) {
            std::vector<double> l(kept.size());
            for (size_t i = 0; i < kept.size(); ++i) l[i] = lufs(kept[i]);
            std::sort(l.begin(), l.end());
            const double m1 = (double)(l.size() - 1);
            out.range = l[(size_t)(m1 * 0.95 + 0.5)] - l[(size_t)(m1 * 0.10 + 0.5)];
        }
    }
    return out;
}

}  // namespace mgx
