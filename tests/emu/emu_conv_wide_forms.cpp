// CPU emulation of k_conv_wide with a choice of phase forms -- TEST INFRASTRUCTURE (tests/test_conv_wide_exchange_emu.py
// registers the unit with tests/emu/build.py and loads it; emu.cpp's emu_convolve_wide stays what it was).
//
// F taps on N = 4F blocks (conv_wide_kernel.h): the phase sequence of k_conv_wide in mgx_kernels.h, as emu.cpp drives it,
// where `forms` chooses, bit by bit, between the form of a phase the kernel runs and the earlier one that is its
// reference:
//   WIDE_KEEP    the *_keep phases; otherwise the whole row through the LDS
//   WIDE_PEAK    the block peak as one maximum per wave, combined by thread 0; otherwise one maximum over the workgroup
//   WIDE_END     the end-of-track mask of phase_store behind a last-block branch; otherwise on every frame
#include <cmath>
#include <functional>
#include <vector>

#include "../../matchering_amd/csrc/conv_wide_kernel.h"
#include "../../matchering_amd/csrc/host_params.h"

using namespace mgx;

static std::vector<float2> twiddles(int n) {
    std::vector<float2> tw(n);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < n; ++k)
        tw[k] = make_float2((float)std::cos(2.0 * pi * k / n), (float)-std::sin(2.0 * pi * k / n));
    return tw;
}

#define FOR_THREADS(T_) for (int tid = 0; tid < (T_); ++tid)

// As in emu.cpp: phases between pass 0 and its inverse run WAVE BY WAVE where the plan is wave-local (no workgroup
// barrier separates them in the kernel), phase by phase otherwise.
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
template <class F>
static std::vector<Phase> mid_phases(bool inverse, float2* lds, const float2* table) {
    std::vector<Phase> out;
    if (F::P < 3) return out;
    if (inverse) {
        if (F::P == 4) out.push_back([=](int tid) { F::inv_mid2(tid, lds, table); });
        out.push_back([=](int tid) { F::inv_mid(tid, lds, table); });
    } else {
        out.push_back([=](int tid) { F::fwd_mid(tid, lds, table); });
        if (F::P == 4) out.push_back([=](int tid) { F::fwd_mid2(tid, lds, table); });
    }
    return out;
}
static std::vector<Phase> operator+(std::vector<Phase> a, const std::vector<Phase>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

enum { WIDE_KEEP = 1, WIDE_PEAK = 2, WIDE_END = 4, WIDE_ALL = 7 };
template <int LOG2N>
static int conv_wide_impl(const float* x, long long n, const double* fir_mid, const double* fir_side, int taps,
                          double gain, float* y, float* ymid, float* block_peak, int forms) {
    using CW = ConvWide<LOG2N>;
    using CB = Conv2Block<LOG2N>;
    using F = typename CB::F;
    if (taps != CW::TAPS) return -1;
    const bool KEEP = forms & WIDE_KEEP;
    const std::vector<float2> tw = twiddles(F::N);
    std::vector<float2> lds(F::LDS_ELEMS), mid_table(F::MID_TABLE + 1), tables((size_t)2 * F::N);
    std::vector<float> h(2 * taps);
    for (int i = 0; i < taps; ++i) { h[i] = (float)fir_mid[i]; h[taps + i] = (float)fir_side[i]; }
    std::vector<typename CB::Persist> ps(F::T);
    FOR_THREADS(F::T) CB::load_persist(tid, tw.data(), mid_table.data(), ps[tid]);
    for (int ch = 0; ch < 2; ++ch) {
        FOR_THREADS(F::T) CW::phase_load_taps(tid, h.data() + (size_t)ch * taps, ps[tid], lds.data());
        float2* table = tables.data() + (size_t)ch * F::N;
        local_phases<F>(mid_phases<F>(false, lds.data(), mid_table.data()) + std::vector<Phase>{[&](int tid) {
                            CB::phase_write_filter(tid, lds.data(), (float)(gain / F::N), table);
                        }});
    }
    Conv2Args a;
    a.x = reinterpret_cast<const float2*>(x);
    a.n = n;
    a.y = reinterpret_cast<float2*>(y);
    a.ymid = ymid;
    a.h_mid = tables.data();
    a.h_side = tables.data() + F::N;
    a.tw = tw.data();
    a.parts = 1;
    a.npairs = (n + CW::HOP - 1) / CW::HOP;              // blocks
    a.pair_peak = nullptr;
    for (long long b = 0; b < a.npairs; ++b) {
        FOR_THREADS(F::T) {
            typename CW::Frames fr;
            CW::fetch(tid, b, a, fr);
            CW::phase_pass0(tid, ps[tid], fr, lds.data());
        }
        std::vector<typename CW::Filters> filt(F::T);
        std::vector<typename CW::Kept> kept(F::T);           // the own half of each thread's row, in its registers
        local_phases<F>(mid_phases<F>(false, lds.data(), mid_table.data()) + std::vector<Phase>{[&](int tid) {
                            CW::fetch_filters(tid, a, filt[tid]);
                            if (KEEP) CW::phase_row_keep(tid, kept[tid], lds.data());
                            else CW::phase_row(tid, lds.data());
                        }});
        FOR_THREADS(F::T) {                                 // (mirror rows: a barrier either side)
            if (KEEP) CW::phase_multiply_keep(tid, filt[tid], kept[tid], lds.data());
            else CW::phase_multiply(tid, filt[tid], lds.data());
        }
        local_phases<F>(std::vector<Phase>{[&](int tid) {
                            if (KEEP) CW::phase_row_back_keep(tid, kept[tid], lds.data());
                            else CW::phase_row_back(tid, lds.data());
                        }} +
                        mid_phases<F>(true, lds.data(), mid_table.data()));
        std::vector<float> thread_peak(F::T);
        FOR_THREADS(F::T) {
            thread_peak[tid] = forms & WIDE_END ? CW::template phase_store<true>(tid, b, a, ps[tid], lds.data())
                                                : CW::template phase_store<false>(tid, b, a, ps[tid], lds.data());
        }
        float pk = 0.f;
        if (forms & WIDE_PEAK) {                             // per wave, no LDS; thread 0 combines the waves' words
            std::vector<float> scratch(F::T / 64, 0.f);
            FOR_THREADS(F::T) scratch[tid >> 6] = std::fmax(scratch[tid >> 6], thread_peak[tid]);
            for (float w : scratch) pk = std::fmax(pk, w);
        } else {
            FOR_THREADS(F::T) pk = std::fmax(pk, thread_peak[tid]);
        }
        if (block_peak) block_peak[b] = pk;
    }
    return 0;
}
// forms: a sum of WIDE_* (0 = every phase in its earlier form)
extern "C" int emu_convolve_wide_forms(const float* x, long long n, const double* fir_mid, const double* fir_side, int taps,
                                       double gain, float* y, float* ymid, float* block_peak, int forms) {
    if (forms < 0 || forms > WIDE_ALL) return -1;
    switch (ilog2_exact(taps)) {
#define CASE(L) case L - 2: return conv_wide_impl<L>(x, n, fir_mid, fir_side, taps, gain, y, ymid, block_peak, forms);
        CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
        default: return -4;
    }
}
