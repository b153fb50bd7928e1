// The clip repair's phase functions (csrc/declip_kernel.h: declip_window, declip_scan, declip_step, declip_fold_slot)
// driven segment by segment and thread by thread on the host, as k_declip and k_declip_fold drive them, behind a C
// interface for tests/test_declip_emu.py.  Each segment's window is a buffer of exactly its size, so that an index off
// by one is AddressSanitizer's to find in the stand-alone program below.  Test infrastructure.
#include <vector>

#include "../../matchering_amd/csrc/declip_kernel.h"

using namespace mgx;

extern "C" {

void emu_declip_constants(long long* out) {
    out[0] = DECLIP_SEGMENT, out[1] = DECLIP_HALO, out[2] = DECLIP_STRETCH, out[3] = DECLIP_THREADS, out[4] = DECLIP_MAX_RUN;
    out[5] = DECLIP_SLOTS, out[6] = DECLIP_WINDOW;
}

// x, out: [n][2]; totals: [2][DECLIP_SLOTS], the words k_declip_fold leaves.  segment, halo and stretch are the
// kernel's constants or smaller ones (all even, halo >= max_run + 2).  Returns 0, or -1 for a geometry it refuses.
int emu_declip(const float* x, long long n, double level, double max_rise, int min_run, int max_run, int segment, int halo,
               int stretch, float* out, long long* totals) {
    if (segment < 2 || (segment & 1) || (halo & 1) || (stretch & 1) || stretch < 2 || halo < max_run + 2) return -1;
    DeclipArgs a;
    a.n = n, a.segments = (n + segment - 1) / segment;
    a.p.level = level, a.p.cap = max_rise * level, a.p.min_run = min_run, a.p.max_run = max_run;
    const DeclipParams P = a.p;
    const int threads = (segment + 2 * halo + stretch - 1) / stretch;
    std::vector<int> seg((size_t)a.segments * 2 * DECLIP_SLOTS);
    for (long long s = 0; s < a.segments; ++s) {
        DeclipWindow W = declip_window(nullptr, s, n, segment, halo);
        const std::vector<float> win(x + W.lo * 2, x + (W.lo + W.wn) * 2);     // stage
        W.w = win.data();
        int cnt[2][DECLIP_SLOTS];
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < DECLIP_SLOTS; ++k) cnt[c][k] = declip_slot_identity(k);
        int rail = 0;
        for (float v : win) rail |= declip_class(v, P.level);
        float* o = out + W.lo * 2;
        if (!rail) {
            for (int f = W.core0; f < W.core1; ++f)
                for (int c = 0; c < 2; ++c) {
                    o[2 * f + c] = win[2 * f + c];
                    declip_copied(win[2 * f + c], cnt[c]);
                }
            for (int c = 0; c < 2; ++c) cnt[c][DECLIP_PEAK_AFTER] = cnt[c][DECLIP_PEAK_BEFORE];
        } else {
            // scan, then the exclusive prefix maximum and suffix minimum over the threads
            std::vector<int> begin[2], end[2], begin_in[2], end_in[2];
            for (int c = 0; c < 2; ++c) {
                begin[c].resize(threads), end[c].resize(threads), begin_in[c].resize(threads), end_in[c].resize(threads);
                for (int t = 0; t < threads; ++t) {
                    const int s0 = t * stretch < W.wn ? t * stretch : W.wn, s1 = s0 + stretch < W.wn ? s0 + stretch : W.wn;
                    declip_scan(W, P.level, s0, s1, c, begin[c][t], end[c][t]);
                }
                int m = -1;
                for (int t = 0; t < threads; ++t) begin_in[c][t] = m, m = begin[c][t] > m ? begin[c][t] : m;
                m = DECLIP_NO_END;
                for (int t = threads - 1; t >= 0; --t) end_in[c][t] = m, m = end[c][t] < m ? end[c][t] : m;
            }
            // walk: every thread its own counters, folded by the slots' rules as the lanes and waves are
            for (int t = 0; t < threads; ++t) {
                const int s0 = t * stretch < W.wn ? t * stretch : W.wn, s1 = s0 + stretch < W.wn ? s0 + stretch : W.wn;
                if (!(s0 < W.core1 && s1 > W.core0)) continue;
                int mine[2][DECLIP_SLOTS];
                for (int c = 0; c < 2; ++c)
                    for (int k = 0; k < DECLIP_SLOTS; ++k) mine[c][k] = declip_slot_identity(k);
                DeclipRun run[2];
                declip_run_start(run[0], s0), declip_run_start(run[1], s0);
                for (int f = s0; f < s1; ++f)
                    for (int c = 0; c < 2; ++c) {
                        const float y = declip_step(W, P, s0, s1, begin_in[c][t], end_in[c][t], c, f, run[c], mine[c]);
                        if (f >= W.core0 && f < W.core1) o[2 * f + c] = y;
                    }
                for (int c = 0; c < 2; ++c)
                    for (int k = 0; k < DECLIP_SLOTS; ++k) cnt[c][k] = declip_fold_slot<int>(k, cnt[c][k], mine[c][k]);
            }
        }
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < DECLIP_SLOTS; ++k) seg[((size_t)s * 2 + c) * DECLIP_SLOTS + k] = cnt[c][k];
    }
    for (int j = 0; j < 2 * DECLIP_SLOTS; ++j) totals[j] = declip_slot_identity(j % DECLIP_SLOTS);
    for (long long s = 0; s < a.segments; ++s)
        for (int j = 0; j < 2 * DECLIP_SLOTS; ++j)
            totals[j] = declip_fold_slot<long long>(j % DECLIP_SLOTS, totals[j], (long long)seg[(size_t)s * 2 * DECLIP_SLOTS + j]);
    return 0;
}

}  // extern "C"

#ifdef EMU_DECLIP_MAIN
// Stand-alone: tracks of the lengths around a segment and a halo, runs of every length up to max_run + 1 at every
// offset against a border, at two geometries; the segmented evaluation against one segment that holds the whole track.
#include <cstdio>
#include <cstring>
int main() {
    unsigned state = 2463534242u;
    auto next = [&]() { return state = state * 1664525u + 1013904223u; };
    int tracks = 0;
    const int geometry[2][4] = {{16, 8, 2, 6}, {64, 20, 6, 18}};          // segment, halo, stretch, max_run
    for (const auto& g : geometry) {
        const int S = g[0], H = g[1], L = g[2], max_run = g[3];
        for (int n : {0, 1, 2, 3, 4, 5, S - 1, S, S + 1, 2 * S + H + 1, 4 * S + 1, 5 * S}) {
            for (int round = 0; round < 40; ++round) {
                std::vector<float> x((size_t)n * 2), got((size_t)n * 2, -5.f), want((size_t)n * 2, -7.f);
                for (auto& v : x) v = (float)((int)(next() >> 16) % 1000) * 0.0007f - 0.35f;
                for (int c = 0; c < 2 && n > 0; ++c)
                    for (int k = 0; k < 2 + n / 12; ++k) {
                        const int at = (int)(next() >> 8) % n, r = 1 + (int)(next() >> 8) % (max_run + 2);
                        const float v = (next() >> 31) ? 0.8f : -0.8f;
                        for (int i = at; i < at + r && i < n; ++i) x[2 * i + c] = v;
                    }
                if (n > 0 && round % 5 == 0) x[(next() >> 8) % (2 * n)] = NAN;
                long long t0[2 * DECLIP_SLOTS], t1[2 * DECLIP_SLOTS];
                // the whole track as one segment: no border inside it
                const int whole = 2 * ((n + 2) / 2);
                if (emu_declip(x.data(), n, 0.8, 2.0, 1 + round % 3, max_run, whole, H, 2 * whole + 2 * H, want.data(), t1) != 0 ||
                    emu_declip(x.data(), n, 0.8, 2.0, 1 + round % 3, max_run, S, H, L, got.data(), t0) != 0) {
                    std::printf("refused geometry\n");
                    return 1;
                }
                if ((n > 0 && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) != 0) ||
                    std::memcmp(t0, t1, sizeof(t0)) != 0) {
                    std::printf("mismatch at segment %d n %d round %d\n", S, n, round);
                    return 1;
                }
                ++tracks;
            }
        }
    }
    std::printf(tracks == 960 ? "ok\n" : "too few tracks\n");
    return 0;
}
#endif
