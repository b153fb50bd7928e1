// Matching EQ tone controls on the device (include/mgx.h, mgx_eq_tone): the matching range, the side amount, mono bass
// and the manual trims, as one stage in place on the two smooth planes.  k_eq_tone runs INSTEAD of k_eq_shape
// (eq_shape_kernels.h) where a call carries a tone that is not neutral: behind every curve route, in front of every tap
// synthesis (run_fir.h), one launch either way.  A bin is a handful of float64 log2 / cos / pow calls and there are
// F/2 + 1 of them per channel: plain code, one thread per bin, nothing shared, no scratch.
//
// The per-thread phase function is eq_tone.h's.
#pragma once

#include "eq_shape_kernels.h"
#include "eq_tone.h"

#if defined(__HIPCC__) && !defined(MGX_HOST_EMU)

namespace mgx {

// the tone stage, in place on the two smooth planes; grid (ceil(bins / 256), 2)
__global__ __launch_bounds__(256) void k_eq_tone(FirPlanView pl, double* scratch, EqToneArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y;
    if (k >= pl.bins) return;
    eq_tone_phase(k, plane, fir_scratch(scratch, pl, plane).smooth, a);
}

}  // namespace mgx
#endif
