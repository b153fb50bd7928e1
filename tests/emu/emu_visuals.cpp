// The visuals' phase functions (csrc/visuals_kernel.h: SpectroBlock's load, power and write phases over Analysis2Block's
// row pass; spectro_pool_value; the overview's record) behind a C interface, driven by a loop over thread ids where the
// GPU has a workgroup and a sequence point where it has a barrier, with the launch geometry of mgx_spectrogram and
// mgx_overview (visuals_plan.h).  Test infrastructure.
#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

#include "../../matchering_amd/csrc/visuals_kernel.h"

using namespace mgx;

#define FOR_THREADS(T_) for (int tid = 0; tid < (T_); ++tid)

// (as tests/emu/emu.cpp: phases between pass 0 and the row pass run wave by wave where the plan is WAVE_LOCAL)
using Phase = std::function<void(int)>;
template <class F>
static void local_phases(const std::vector<Phase>& phases) {
    if (F::WAVE_LOCAL) {
        for (int w = 0; w < F::T / 64; ++w)
            for (const Phase& ph : phases)
                for (int tid = 64 * w; tid < 64 * w + 64; ++tid) ph(tid);
    } else {
        for (const Phase& ph : phases) { FOR_THREADS(F::T) ph(tid); }
    }
}

static std::vector<float> hann(int n, double* sum) {
    std::vector<float> w(n);
    const double pi = 3.14159265358979323846;
    *sum = 0.0;
    for (int i = 0; i < n; ++i) {
        w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)n));
        *sum += (double)w[i];
    }
    return w;
}

template <int LOG2N>
static int spectrogram_impl(const float* x, long long n, int hop, int columns, int channels, int bands, const int* edges,
                            float* out) {
    using SB = SpectroBlock<LOG2N>;
    using AB = Analysis2Block<LOG2N>;
    using F = Fft2<LOG2N>;
    std::vector<float2> tw(F::N);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < F::N; ++k)
        tw[k] = make_float2((float)std::cos(2.0 * pi * k / F::N), (float)-std::sin(2.0 * pi * k / F::N));
    double sum = 0.0;
    const std::vector<float> window = hann(F::N, &sum);
    SpectroArgs a;
    a.x = reinterpret_cast<const float2*>(x);
    a.n = n;
    a.hop = hop, a.hops = spectro_hops(n, hop);
    a.columns = columns == 0 ? (int)a.hops : columns;
    a.parts = visuals_parts(a.hops, a.columns, SPECTRO_RUN_CAP);
    a.channels = channels, a.bands = bands;
    a.window = window.data(), a.tw = tw.data();
    const int half = F::N / 2;
    const long long groups = (long long)a.columns * a.parts;
    std::vector<float> part((size_t)groups * 2 * (half + 1), -1.f);     // (every word must be written: -1 is no power)
    a.part = part.data();
    a.edges = edges;
    a.scale = (2.0 / sum) * (2.0 / sum) * 0.25;
    a.out = out;
    std::vector<float2> lds(F::LDS_ELEMS), mid_table(F::MID_TABLE + 1);
    std::vector<typename SB::Thread> th(F::T);
    std::vector<typename AB::Row> own(F::T);
    std::vector<typename AB::Persist> ps(F::T);
    FOR_THREADS(F::T) AB::load_persist(tid, a.tw, mid_table.data(), ps[tid]);
    for (long long wg = 0; wg < groups; ++wg) {
        const int c = (int)(wg / a.parts), p = (int)(wg % a.parts);
        long long t0, t1, h0, h1;
        visuals_column(a.hops, a.columns, c, t0, t1);
        visuals_part(t0, t1, p, SPECTRO_RUN_CAP, h0, h1);
        FOR_THREADS(F::T) SB::init(th[tid]);
        for (long long t = h0; t < h1; ++t) {
            FOR_THREADS(F::T) SB::phase_load(tid, SB::hop_start(t, a.hop), a, ps[tid], lds.data());
            std::vector<Phase> phases;
            if (F::P >= 3) phases.push_back([&](int tid) { F::fwd_mid(tid, lds.data(), mid_table.data()); });
            if (F::P == 4) phases.push_back([&](int tid) { F::fwd_mid2(tid, lds.data(), mid_table.data()); });
            phases.push_back([&](int tid) { AB::phase_row(tid, own[tid], lds.data()); });
            local_phases<F>(phases);
            FOR_THREADS(F::T) SB::phase_power(tid, own[tid], th[tid], lds.data());
        }
        FOR_THREADS(F::T) SB::phase_write(tid, wg, a, th[tid]);
    }
    for (float v : part)
        if (v < 0.f) return -2;
    const long long values = (long long)a.columns * 2 * bands;
    for (long long i = 0; i < values; ++i) out[i] = spectro_pool_value(a, i, half);
    return 0;
}

extern "C" {

// out: [W][2][bands]; 0, or -1 for a transform length outside 8 .. 14, -2 for a partial word no thread wrote
int emu_spectrogram(const float* x, long long n, int log2_fft, int hop, int columns, int channels, int bands,
                    const int* edges, float* out) {
    if (n <= 0) return 0;
    switch (log2_fft) {
#define CASE(L) case L: return spectrogram_impl<L>(x, n, hop, columns, channels, bands, edges, out);
        CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
    }
    return -1;
}

// minmax [W][2][2], sumsq [W][2]: the workgroups' shares thread by thread, lanes and waves folded in order, then the fold
int emu_overview(const float* x, long long n, int columns, float* minmax, double* sumsq) {
    const float2* frames = reinterpret_cast<const float2*>(x);
    const int parts = visuals_parts(n, columns, OVERVIEW_SHARE);
    for (int c = 0; c < columns; ++c) {
        OverviewThread total;
        overview_init(total);
        long long f0, f1;
        visuals_column(n, columns, c, f0, f1);
        for (int p = 0; p < parts; ++p) {
            long long begin, end;
            visuals_part(f0, f1, p, OVERVIEW_SHARE, begin, end);
            std::vector<OverviewThread> th(OVERVIEW_THREADS);
            FOR_THREADS(OVERVIEW_THREADS) {
                overview_init(th[tid]);
                for (long long f = begin + tid; f < end; f += OVERVIEW_THREADS) overview_push(th[tid], frames[f]);
            }
            for (int ch = 0; ch < 2; ++ch) {
                double share = 0.0;
                for (int w = 0; w < OVERVIEW_THREADS / 64; ++w) {
                    double lanes[64];
                    for (int l = 0; l < 64; ++l) lanes[l] = th[64 * w + l].sq[ch];
                    for (int o = 32; o > 0; o >>= 1)                    // the butterfly of k_overview, as lane 0 sees it
                        for (int l = 0; l < o; ++l) lanes[l] += lanes[l + o];
                    share += lanes[0];
                }
                total.sq[ch] += share;
                FOR_THREADS(OVERVIEW_THREADS) {
                    total.lo[ch] = fminf(total.lo[ch], th[tid].lo[ch]);
                    total.hi[ch] = fmaxf(total.hi[ch], th[tid].hi[ch]);
                }
            }
        }
        for (int ch = 0; ch < 2; ++ch) {
            minmax[(c * 2 + ch) * 2] = total.lo[ch], minmax[(c * 2 + ch) * 2 + 1] = total.hi[ch];
            sumsq[c * 2 + ch] = total.sq[ch];
        }
    }
    return 0;
}

void emu_visuals_constants(long long* out) {
    out[0] = SPECTRO_RUN_CAP, out[1] = OVERVIEW_SHARE, out[2] = OVERVIEW_THREADS, out[3] = OVERVIEW_COLUMNS_MAX;
    out[4] = VISUALS_FRAMES_MAX, out[5] = VISUALS_BYTES_MAX;
}

}  // extern "C"

#ifdef EMU_VISUALS_MAIN
// Stand-alone: a short track through 256- and 4096-point pictures -- hops that hang over both ends, a column split over
// several workgroups, every bin and three bands -- against a direct float64 DFT, and an overview with a split column;
// for a run under the host sanitizers.
static double direct_power(const std::vector<float>& x, long long n, int N, int hop, long long t, int ch, int k, double sum) {
    const double pi = 3.14159265358979323846;
    double re = 0.0, im = 0.0;
    for (int i = 0; i < N; ++i) {
        const long long f = t * hop - N / 2 + i;
        if (f < 0 || f >= n) continue;
        const double w = (double)(float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)N));
        const double v = (double)x[2 * f + ch] * w;
        re += v * std::cos(2.0 * pi * (double)k * i / N), im -= v * std::sin(2.0 * pi * (double)k * i / N);
    }
    return (re * re + im * im) * (2.0 / sum) * (2.0 / sum);
}

int main() {
    unsigned state = 2463534242u;
    auto noise = [&]() { return (float)((double)((state = state * 1664525u + 1013904223u) >> 8) / 8388608.0 - 1.0); };
    int bad = 0;
    for (int log2n : {8, 12}) {
        const int N = 1 << log2n, hop = log2n == 8 ? 3 : 1000;
        const long long n = log2n == 8 ? 300 : 9000;
        std::vector<float> x(2 * n);
        for (auto& v : x) v = 0.5f * noise();
        double sum = 0.0;
        hann(N, &sum);
        const long long T = spectro_hops(n, hop);
        std::vector<int> all(N / 2 + 2);
        for (int k = 0; k < N / 2 + 2; ++k) all[k] = k;
        const int columns = log2n == 8 ? 2 : 0;                  // 100 hops in two columns: two workgroups each
        const int W = columns ? columns : (int)T;
        std::vector<float> got((size_t)W * 2 * (N / 2 + 1));
        if (emu_spectrogram(x.data(), n, log2n, hop, columns, 0, N / 2 + 1, all.data(), got.data()) != 0) return 2;
        double peak = 0.0, worst = 0.0;
        for (int c = 0; c < W; c += (W > 4 ? W - 1 : 1))
            for (int k = 0; k <= N / 2; k += (log2n == 8 ? 1 : 97)) {
                long long t0, t1;
                visuals_column(T, W, c, t0, t1);
                double want = 0.0;
                for (long long t = t0; t < t1; ++t) want += direct_power(x, n, N, hop, t, 1, k, sum);
                want /= (double)(t1 - t0);
                peak = std::fmax(peak, want);
                worst = std::fmax(worst, std::fabs(want - (double)got[((size_t)c * 2 + 1) * (N / 2 + 1) + k]));
            }
        std::printf("N %d: worst %.3e of peak %.3e\n", N, worst, peak);
        if (!(worst <= 4e-6 * peak)) ++bad;
        const int three[4] = {0, 1, 7, N / 2 + 1};
        std::vector<float> banded((size_t)W * 2 * 3);
        if (emu_spectrogram(x.data(), n, log2n, hop, columns, 1, 3, three, banded.data()) != 0) return 2;
    }
    {
        const long long n = 40000;
        std::vector<float> x(2 * n);
        for (auto& v : x) v = noise();
        std::vector<float> minmax(3 * 4);
        std::vector<double> sumsq(3 * 2);
        emu_overview(x.data(), n, 3, minmax.data(), sumsq.data());
        emu_overview(x.data(), n, 1, minmax.data(), sumsq.data());   // one column: three shares
        double want = 0.0;
        for (long long f = 0; f < n; ++f) want += (double)x[2 * f] * (double)x[2 * f];
        if (!(std::fabs(want - sumsq[0]) <= 1e-9 * want)) ++bad;
    }
    std::printf(bad ? "mismatch\n" : "ok\n");
    return bad ? 1 : 0;
}
#endif
