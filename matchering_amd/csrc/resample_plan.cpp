// Host plan of the sample-rate converter: see resample_plan.h.  A restatement of resample.kaiser_best(), _Plan and
// _prototype (matchering_amd/resample.py) operation by operation, so that the rows agree with the numpy form to the
// rounding of the two libraries' sin and I0.
#include "resample_plan.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <numeric>

namespace mgx {
namespace {

constexpr int NUM_ZEROS = 64, NUM_TABLE = 512;                  // zero crossings, entries per crossing (precision 9)
constexpr int NWIN = NUM_ZEROS * NUM_TABLE + 1;
constexpr double BETA = 14.769656459379492, ROLLOFF = 0.9475937167399596;

// I0 by its power series, summed until a term no longer changes the sum: every term is positive, so the sum carries
// a few roundings and no cancellation (numpy.i0 is Cephes' Chebyshev form, good to the same last bits)
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

const std::vector<double>& kaiser_best() {
    static std::vector<double> table;
    static std::once_flag once;
    std::call_once(once, [] {
        const double pi = 3.141592653589793;
        const int n = NWIN - 1;
        const double i0_beta = bessel_i0(BETA);
        table.resize(NWIN);
        for (int k = 0; k <= n; ++k) {
            const double at = ROLLOFF * ((double)k * ((double)NUM_ZEROS / (double)n));      // numpy.linspace: k * step
            const double y = pi * (at == 0.0 ? 1.0e-20 : at);                               // numpy.sinc
            const double sinc_win = ROLLOFF * (std::sin(y) / y);
            const double r = (double)k / (double)n;
            const double taper = bessel_i0(BETA * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0_beta;
            table[k] = taper * sinc_win;
        }
    });
    return table;
}

}  // namespace

int resample_geometry(int rate_in, int rate_out, ResampleGeometry* g, std::string* why) {
    const int d = std::gcd(rate_in, rate_out);
    g->L = rate_out / d;
    g->M = rate_in / d;
    g->ratio = (double)rate_out / (double)rate_in;
    g->scale = std::min(1.0, g->ratio);
    g->index_step = (int)(g->scale * NUM_TABLE);
    if (g->L > RESAMPLE_MAX_PHASES) {
        *why = "the ratio " + std::to_string(g->L) + "/" + std::to_string(g->M) + " has more than " +
               std::to_string(RESAMPLE_MAX_PHASES) + " phases";
        return -1;
    }
    if (g->index_step < 1) {
        *why = "the output rate is below 1/512 of the input rate";
        return -1;
    }
    g->taps = NWIN / g->index_step + 1;
    g->W = 2 * g->taps;
    const long long reach = ((long long)(RESAMPLE_BLOCK - 1) * g->M + g->L - 1) / g->L + g->W;
    if (reach > RESAMPLE_SPAN_MAX) {
        *why = std::to_string(RESAMPLE_BLOCK) + " outputs reach " + std::to_string(reach) + " input frames, more than the " +
               std::to_string(RESAMPLE_SPAN_MAX) + " a workgroup stages";
        return -1;
    }
    g->span = (int)reach;
    if ((size_t)g->L * g->W * sizeof(double) > RESAMPLE_MATRIX_MAX) {
        *why = "the weights of " + std::to_string(g->L) + " phases of " + std::to_string(g->W) + " taps exceed " +
               std::to_string(RESAMPLE_MATRIX_MAX >> 20) + " MiB";
        return -1;
    }
    return 0;
}

int64_t resample_length(int64_t n, int rate_in, int rate_out) {
    const double ratio = (double)rate_out / (double)rate_in;
    return (int64_t)((double)n * ratio);
}

std::shared_ptr<const ResamplePlan> resample_design(int rate_in, int rate_out) {
    auto plan = std::make_shared<ResamplePlan>();
    std::string why;
    if (resample_geometry(rate_in, rate_out, &plan->g, &why) != 0) return nullptr;
    const ResampleGeometry& g = plan->g;
    const std::vector<double>& table = kaiser_best();
    std::vector<double> win(NWIN), delta(NWIN, 0.0);
    for (int k = 0; k < NWIN; ++k) win[k] = g.ratio < 1.0 ? table[k] * g.ratio : table[k];
    for (int k = 0; k + 1 < NWIN; ++k) delta[k] = win[k + 1] - win[k];
    plan->rows.assign((size_t)g.L * g.W, 0.0);
    for (int p = 0; p < g.L; ++p) {
        double* row = plan->rows.data() + (size_t)p * g.W;
        const double position = (double)p / (double)g.L;
        for (int right = 0; right < 2; ++right) {
            double frac = g.scale * position;
            if (right) frac = g.scale - frac;
            const double index_frac = frac * NUM_TABLE;
            const int offset = (int)index_frac;
            const double eta = index_frac - offset;
            const int count = std::min(g.taps, (NWIN - offset) / g.index_step);
            for (int i = 0; i < count; ++i) {
                const int at = offset + i * g.index_step;
                const double w = win[at] + eta * delta[at];
                // left wing: x[n - i], entry taps + i; right wing: x[n + i + 1], entry taps - 1 - i
                row[right ? g.taps - 1 - i : g.taps + i] = w;
            }
        }
        double sum = 0.0;
        for (int k = 0; k < g.W; ++k) sum += std::fabs(row[k]);
        plan->max_row_sum = std::max(plan->max_row_sum, sum);
    }
    return plan;
}

std::vector<double> resample_device_matrix(const ResamplePlan& plan) {
    const ResampleGeometry& g = plan.g;
    std::vector<double> m((size_t)g.W * g.L);
    for (int j = 0; j < g.L; ++j) {
        const int p = (int)(((long long)j * g.M) % g.L);
        for (int k = 0; k < g.W; ++k) m[(size_t)k * g.L + j] = plan.rows[(size_t)p * g.W + k];
    }
    return m;
}

}  // namespace mgx
