// The host side of the visuals (visuals_kernel.h) that is no entry point: the window table a handle builds once per
// transform length, and the spectrogram's launch.
#pragma once

#include <cmath>

#include "handle.h"

// the periodic Hann window of 2^log2n points on the device, float32 of the float64 values, and the sum of the float32s
static int spectro_window(mgx_handle* h, int log2n, mgx_handle::SpectroWindow** out) {
    mgx_handle::SpectroWindow& w = h->spectro_windows[log2n];
    if (!w.table.p) {
        const int N = 1 << log2n;
        std::vector<float> host(N);
        const double pi = 3.14159265358979323846;
        double sum = 0.0;
        for (int i = 0; i < N; ++i) {
            host[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)N));
            sum += (double)host[i];
        }
        MGX_TRY(ensure(h, w.table, (size_t)N * sizeof(float)));
        HIP_TRY(hipMemcpy(w.table.p, host.data(), (size_t)N * sizeof(float), hipMemcpyHostToDevice));
        w.sum = sum;
    }
    *out = &w;
    return 0;
}

template <int LOG2N>
static int launch_spectrogram(mgx_handle* h, const SpectroArgs& a) {
    const size_t lds = analysis_lds_bytes<LOG2N>();
    MGX_TRY(allow_lds(k_spectrogram<LOG2N>, lds));
    hipLaunchKernelGGL(k_spectrogram<LOG2N>, dim3((unsigned)((long long)a.columns * a.parts)), dim3(Fft2<LOG2N>::T), lds,
                       h->stream, a);
    return 0;
}
