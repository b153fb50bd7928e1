// Which per-call context an mgx_master call uses and which event waits order it against its neighbours.
// Pure host code, no HIP: master_call.h only executes what master() returns, and tests/test_call_pipeline_host.py drives
// this unit with generated call sequences on a machine without a GPU.
//
// A master call has a FRONT half (analysis, FIR design, filter spectra: reads the call's inputs, writes its context)
// and a BACK half (convolution, level correction, scale, limiter: reads the context and the target, writes the
// outputs).  Back halves stay on the handle's main stream, one behind the other.  The front half of call k may run on
// a second stream, under the back half of call k - 1, because it depends on nothing that call computes -- unless the
// handle is "dirty" for this call, in which case it first waits for everything queued on main so far.
//
// The back half itself lets go of the context early: behind round 0 of its level correction nothing of the call touches
// the context any more (handle.h, CallContext; correction_kernels.h, BackState).  The event of wait (a) is recorded there, so the front half
// of call k may also run beside the tail, the scale kernel and the limiter of call k - 2.  The planner does not care
// where in the back half the event lies: `record_back` says that it is recorded, `wait_context` that it is waited for.
#pragma once
#include <cstdint>

namespace mgx {

constexpr int CALL_CONTEXTS = 2;

struct ByteRange {              // [lo, hi) of device addresses; lo == hi: nothing
    uintptr_t lo = 0, hi = 0;
};
inline ByteRange byte_range(const void* p, uint64_t bytes) {
    ByteRange r;
    if (p && bytes) {
        r.lo = (uintptr_t)p;
        r.hi = r.lo + bytes;
    }
    return r;
}
inline bool overlap(const ByteRange& a, const ByteRange& b) { return a.lo < b.hi && b.lo < a.hi; }

struct MasterRanges {
    ByteRange in[4];            // target, reference, profile, fir_given: what the front half reads
    ByteRange out[3];           // result, result_no_limiter, result_no_limiter_normalized
    bool reads_context_taps = false;        // fir_given lies in a context's own taps buffer
};

struct MasterPlan {
    int context = 0;            // the CallContext of this call: the other one for a pipelined call, the current one else
    bool pipelined = false;     // front half on the front stream, (c) and (d); else the whole call on main as ever
    bool wait_context = false;  // (a) front waits for ctx_released[context]: call k - 2 has let go of the context
    bool wait_main = false;     // (b) front waits for an event recorded on main now: the call is dirty
    bool record_back = false;   // ctx_released[context] is recorded in the back half, behind its last launch that touches the context
};

class CallPipeline {
public:
    // `serial`: the call must run on main alone (stage timing brackets one stream's work; a report waits for its
    // scalars anyway; the handle has siblings on its device)
    MasterPlan master(const MasterRanges& r, bool serial);
    // the last call again, on main alone, after the caller has drained both streams (check_device_error)
    MasterPlan replay();
    // an entry point other than a master call has queued work on main that may write device memory
    void other_work() { dirty_ = true; }
    // the caller has synchronised main with no front half left without its back half: nothing is in flight
    void drained();
    int current() const { return current_; }        // the most recent call's context

private:
    int current_ = 0;
    bool dirty_ = false;                            // other_work() since the previous master call
    bool busy_[CALL_CONTEXTS] = {};                 // ctx_released[c] recorded and not known to have passed
    // The outputs of the previous two master calls.  Two are enough although the front half of call k + 2 may run while
    // the limiter of call k still writes its result: when call k + 2 is planned these are the outputs of calls k + 1 and
    // k, exactly the back halves that may still be running.  Every older one has finished before that front half starts:
    // it waits for call k's round 0 (wait (a)), which lies on main behind the whole back half of call k - 1.
    ByteRange recent_out_[2][3];
};

}  // namespace mgx
