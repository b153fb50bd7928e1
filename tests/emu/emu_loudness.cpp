// CPU emulation of the loudness meter -- TEST INFRASTRUCTURE (tests/test_loudness_host.py).
//
// Compiled by tests/emu/build.py ("loudness") with a plain host compiler and -DMGX_HOST_EMU: the host plan
// (matchering_amd/csrc/loudness_plan.cpp) as the library compiles it, the launch as mgx_loudness fills it
// (loudness_launch) and the SAME per-thread phase functions k_loudness inlines (loudness_kernel.h), driven by a loop
// over thread ids where the GPU has a workgroup and a plain sequence point where it has a barrier.  Not part of the
// product.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../matchering_amd/csrc/loudness_kernel.h"
#include "../../matchering_amd/csrc/loudness_plan.h"

using namespace mgx;

// c[10], A[16], B[4], table[LOUD_TABLE_DOUBLES], misc = {rho, warmup, warmup_poles}
extern "C" int emu_loudness_plan(int rate, double* c, double* A, double* B, double* table, double* misc) {
    const LoudnessPlan p = loudness_design(rate);
    std::memcpy(c, p.c, sizeof p.c);
    std::memcpy(A, p.A, sizeof p.A);
    std::memcpy(B, p.B, sizeof p.B);
    std::memcpy(table, p.table.data(), p.table.size() * sizeof(double));
    misc[0] = p.rho;
    misc[1] = (double)p.warmup;
    misc[2] = (double)p.warmup_poles;
    return (int)p.table.size();
}

extern "C" void emu_loudness_taps(double* taps49) { loudness_true_peak_taps(taps49); }

// out = {S, nsub, warmup, own, workgroups}
extern "C" void emu_loudness_geometry(int rate, long long n, long long* out) {
    const LoudnessGeometry g = loudness_geometry(loudness_design(rate), n);
    out[0] = g.S;
    out[1] = g.nsub;
    out[2] = g.warmup;
    out[3] = g.own;
    out[4] = g.workgroups;
}

// out = {integrated, range, momentary_max, short_term_max}
extern "C" void emu_loudness_gate(const double* e, long long nsub, int S, double* out) {
    const LoudnessGated g = loudness_gate(e, nsub, S);
    out[0] = g.integrated;
    out[1] = g.range;
    out[2] = g.momentary_max;
    out[3] = g.short_term_max;
}

// The launch of mgx_loudness on the CPU: x[n][2] float32 -> e[nsub][2], peaks[workgroups][2], *error = the input word.
// `e` must hold exactly nsub rows and `peaks` exactly `workgroups`.  Returns the number of workgroups.
extern "C" long long emu_loudness(const float* x, long long n, int rate, double* e, double* peaks, int* error) {
    const LoudnessPlan plan = loudness_design(rate);
    const LoudnessGeometry g = loudness_geometry(plan, n);
    LoudnessArgs a;
    loudness_launch(a, plan, g, n);
    a.x = x;
    a.table = plan.table.data();
    a.e = e;
    a.peaks = peaks;
    a.error = error;
    a.error_slot = 0;
    std::vector<char> smem(LOUD_LDS_BYTES);
    std::vector<LoudThread> th(LOUD_THREADS);
    const LoudLds l = loud_lds(smem.data());
    for (long long wg = 0; wg < g.workgroups; ++wg) {
        std::fill(smem.begin(), smem.end(), (char)0x7f);            // (what a previous workgroup left behind must not matter)
        const LoudRange r = loud_range(a, wg, g.workgroups);
        for (int t = 0; t < LOUD_THREADS; ++t) loud_init(l, t, th[t]);
        for (int tile = 0; tile < r.tiles; ++tile) {
            for (int t = 0; t < LOUD_THREADS; ++t) loud_stage(a, r.start + (long long)tile * LOUD_TILE, l, t);
            // -- barrier --
            for (int t = 0; t < LOUD_THREADS; ++t) loud_run(a, tile, l, t, th[t]);
            // -- barrier --
            for (int k = 0; k < LOUD_SCAN_STEPS; ++k)
                for (int t = 0; t < LOUD_THREADS; ++t) loud_scan_step(a, k, l, t, th[t]);       // -- barrier behind each --
            for (int t = 0; t < LOUD_THREADS; ++t) loud_energy(a, r, tile, l, t, th[t]);
            // -- barrier --
            for (int t = 0; t < LOUD_THREADS; ++t) loud_reduce_groups(a, r, tile, l, t);
            // -- barrier --
            for (int t = 0; t < LOUD_THREADS; ++t) loud_reduce_tile(a, r, tile, l, t);
        }
        // -- barrier --
        for (int t = 0; t < LOUD_THREADS; ++t) loud_finish_put(a, r, l, t, th[t]);
        // -- barrier --
        for (int t = 0; t < LOUD_THREADS; ++t) loud_finish_groups(l, t);
        // -- barrier --
        for (int t = 0; t < LOUD_THREADS; ++t) loud_finish(a, wg, l, t);
    }
    return g.workgroups;
}
