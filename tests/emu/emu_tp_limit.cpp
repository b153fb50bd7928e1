// CPU emulation of the deliveries' true-peak limiter -- TEST INFRASTRUCTURE (tests/test_tp_limiter_host.py).
//
// Compiled by tests/emu/build.py ("tp_limit") with a plain host compiler and -DMGX_HOST_EMU: the SAME per-thread phase
// functions k_tp_envelope, k_tp_aggregate and k_tp_apply inline (matchering_amd/csrc/tp_limit_kernel.h) and the same
// host plan, driven by a loop over thread ids where the GPU has a workgroup, a plain sequence point where it has a
// barrier and one loop after the other where it has three launches.  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../matchering_amd/csrc/loudness_plan.h"
#include "../../matchering_amd/csrc/tp_limit_kernel.h"

using namespace mgx;

// out = {T, B, THREADS, LOOKAHEAD_MAX, the LDS bytes of k_tp_apply at look-ahead L, chunk, chunk2}
extern "C" void emu_tp_limit_constants(int L, long long* out) {
    out[0] = TPL_TILE;
    out[1] = TPL_BLOCK;
    out[2] = TPL_THREADS;
    out[3] = TPL_LOOKAHEAD_MAX;
    out[4] = (long long)tpl_apply_lds_bytes(L);
    out[5] = tpl_odd_chunk(TPL_TILE + 2 * L + 1);
    out[6] = tpl_odd_chunk(TPL_TILE + L + 1);
}

#define EACH_THREAD for (int t = 0; t < TPL_THREADS; ++t)

// The three launches of mgx_tp_limit on the CPU: x[n][2] -> out[n][2]; d0 (may be null) receives the plane's first n
// entries.  `lookback` < 0: the plan's own; otherwise it replaces it (a test cuts the carry short to see that it matters).
// Returns the largest s.
extern "C" double emu_tp_limit(const float* x, long long n, double pre_gain, double ceiling, int L, double release, float* out,
                               float* d0, int lookback) {
    if (n <= 0) return 0.0;
    TpLimitArgs a;
    double taps[49];
    loudness_true_peak_taps(taps);
    tpl_plan(a, n, pre_gain, ceiling, L, release, taps);
    if (lookback >= 0) a.lookback = lookback;
    std::vector<float> plane((size_t)a.tiles * TPL_TILE, -1.0f);
    std::vector<double> agg((size_t)a.tiles, -1.0), peak((size_t)a.tiles, -1.0);
    a.x = x;
    a.out = out;
    a.d0 = plane.data();
    a.agg = agg.data();
    a.peak = peak.data();
    const size_t region_a = tpl_region_a(L), region_b = tpl_region_b(L);
    std::vector<char> smem(std::max(tpl_apply_lds_bytes(L), TPL_ENVELOPE_LDS_BYTES));
    std::vector<TplThread> th(TPL_THREADS);

    for (long long tile = 0; tile < a.tiles; ++tile) {                      // ---- k_tp_envelope
        std::fill(smem.begin(), smem.end(), (char)0x7f);                    // (what a previous workgroup left behind must not matter)
        float2* lx = reinterpret_cast<float2*>(smem.data());
        EACH_THREAD tpl_envelope_stage(a, tile * TPL_TILE, lx, t);
        EACH_THREAD tpl_envelope(a, tile * TPL_TILE, lx, t);
    }
    for (long long block = 0; block + 1 < a.tiles; ++block) {               // ---- k_tp_aggregate
        std::fill(smem.begin(), smem.end(), (char)0x7f);
        const TplLds l = tpl_lds(smem.data(), 0, 0);
        EACH_THREAD tpl_aggregate_run(a, block, l, t);
        EACH_THREAD tpl_decay_group(l, t, a.rho_run, th[t]);
        EACH_THREAD tpl_aggregate_finish(a, block, l, t, th[t]);
    }
    const int steps = tpl_hold_steps(L), pieces = (TPL_TILE + 4 * L + 1 + TPL_TILE - 1) / TPL_TILE;
    for (long long tile = 0; tile < a.tiles; ++tile) {                      // ---- k_tp_apply
        std::fill(smem.begin(), smem.end(), (char)0x7f);
        const TplLds l = tpl_lds(smem.data(), region_a, region_b);
        EACH_THREAD tpl_apply_stage(a, tile, l, t);
        EACH_THREAD tpl_max_groups(l, t);
        EACH_THREAD tpl_apply_run(a, l, t, th[t]);                          // (reads g only; s is written behind it ...
        EACH_THREAD tpl_put_total(l, t, th[t]);                             //  ... which no thread still reads)
        EACH_THREAD tpl_decay_group(l, t, a.rho_chunk, th[t]);
        EACH_THREAD tpl_apply_release(a, l, t, th[t]);
        for (int step = 0; step < steps; ++step)
            for (int piece = 0; piece < pieces; ++piece) {
                EACH_THREAD tpl_hold_read(a, step, piece, l, t, th[t]);
                EACH_THREAD tpl_hold_write(a, piece, l, t, th[t]);
            }
        EACH_THREAD tpl_apply_q(a, tile, steps, l, t);
        EACH_THREAD tpl_apply_edges(a, tile, l, th[t]);
        EACH_THREAD {
            tpl_apply_sum1(a, tile, l, t, th[t]);
            tpl_put_total(l, t, th[t]);
        }
        EACH_THREAD tpl_sum_group(l, t, th[t]);
        EACH_THREAD tpl_apply_offset1(a, l, t, th[t]);
        EACH_THREAD {
            tpl_apply_sum2(a, l, t, th[t]);
            tpl_put_total(l, t, th[t]);
        }
        EACH_THREAD tpl_sum_group(l, t, th[t]);
        EACH_THREAD tpl_apply_offset2(a, l, t, th[t]);
        EACH_THREAD tpl_apply_store(a, tile, l, t, th[t]);
        EACH_THREAD tpl_max_groups(l, t);
        EACH_THREAD tpl_apply_peak(a, tile, l, t);
    }
    if (d0) std::copy(plane.begin(), plane.begin() + n, d0);
    return *std::max_element(peak.begin(), peak.end());
}

#ifdef EMU_TP_LIMIT_MAIN
// A stand-alone run of the emulation under the sanitizers (tests/test_emu_drivers_host.py; build.py build_driver):
// exactly sized buffers at the sizes around a tile and the extreme look-aheads.
#include <cstdio>
int main() {
    const long long sizes[] = {1, 2, 66, 133, 4095, 4096, 4097, 8195, 20000};
    const int lookaheads[] = {1, 8, 66, 2048};
    const double releases[] = {0.0, 32.0, 2205.0};
    for (long long n : sizes)
        for (int L : lookaheads)
            for (double R : releases) {
                std::vector<float> x((size_t)n * 2), out((size_t)n * 2), d0((size_t)n);
                for (long long i = 0; i < 2 * n; ++i) x[i] = (float)((i * 37 % 201) - 100) / 90.0f;
                const double s = emu_tp_limit(x.data(), n, 1.3, 0.8, L, R, out.data(), d0.data(), -1);
                if (!(s >= 0.0 && s < 1.0)) return 1;
            }
    std::puts("ok");
    return 0;
}
#endif
