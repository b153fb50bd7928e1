// csrc/call_pipeline.cpp behind a C interface (tests/test_call_pipeline_host.py), and -- built with
// -DEMU_CALL_PIPELINE_MAIN -- a stand-alone driver of the same unit for sanitizer builds: it runs a generated
// sequence of calls through the planner and prints one line per plan.
#include <cstdint>
#include <cstdio>

#include "../../matchering_amd/csrc/call_pipeline.h"

using namespace mgx;

extern "C" {

void* emu_pipeline_create(void) { return new CallPipeline(); }
void emu_pipeline_destroy(void* p) { delete (CallPipeline*)p; }
void emu_pipeline_other_work(void* p) { ((CallPipeline*)p)->other_work(); }
void emu_pipeline_drained(void* p) { ((CallPipeline*)p)->drained(); }
int emu_pipeline_current(void* p) { return ((CallPipeline*)p)->current(); }

static void fill(const MasterPlan& plan, int* out) {
    out[0] = plan.context;
    out[1] = plan.pipelined;
    out[2] = plan.wait_context;
    out[3] = plan.wait_main;
    out[4] = plan.record_back;
}

// ranges: [7][2] = {lo, hi} of target, reference, profile, fir_given, then the three outputs; plan: [5]
void emu_pipeline_master(void* p, const uint64_t* ranges, int reads_context_taps, int serial, int* plan) {
    MasterRanges r;
    for (int i = 0; i < 4; ++i) r.in[i] = byte_range((const void*)(uintptr_t)ranges[2 * i], ranges[2 * i + 1] - ranges[2 * i]);
    for (int i = 0; i < 3; ++i)
        r.out[i] = byte_range((const void*)(uintptr_t)ranges[8 + 2 * i], ranges[8 + 2 * i + 1] - ranges[8 + 2 * i]);
    r.reads_context_taps = reads_context_taps != 0;
    fill(((CallPipeline*)p)->master(r, serial != 0), plan);
}
void emu_pipeline_replay(void* p, int* plan) { fill(((CallPipeline*)p)->replay(), plan); }

}  // extern "C"

#ifdef EMU_CALL_PIPELINE_MAIN
int main() {
    uint64_t state = 12345;
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)(state >> 33);
    };
    for (int round = 0; round < 2; ++round) {
        void* p = emu_pipeline_create();
        int pipelined = 0, waits = 0;
        for (int step = 0; step < 4000; ++step) {
            const unsigned what = next() % 8;
            if (what == 0) emu_pipeline_other_work(p);
            if (what == 1) emu_pipeline_drained(p);
            int plan[5];
            if (what == 2 && step > 0) {
                emu_pipeline_replay(p, plan);
                continue;
            }
            uint64_t ranges[14];
            for (int i = 0; i < 7; ++i) {
                const uint64_t lo = 4096 + 1024 * (next() % 12);
                ranges[2 * i] = (next() % 4 == 0) ? 0 : lo;
                ranges[2 * i + 1] = ranges[2 * i] ? lo + 1024 : 0;
            }
            emu_pipeline_master(p, ranges, next() % 16 == 0, next() % 8 == 0, plan);
            if (plan[0] < 0 || plan[0] >= CALL_CONTEXTS || plan[0] != emu_pipeline_current(p)) return 1;
            pipelined += plan[1];
            waits += plan[2] + plan[3];
        }
        std::printf("round %d: %d pipelined plans, %d waits\n", round, pipelined, waits);
        emu_pipeline_destroy(p);
    }
    return 0;
}
#endif
