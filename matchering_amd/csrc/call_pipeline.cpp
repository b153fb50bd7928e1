#include "call_pipeline.h"

namespace mgx {

MasterPlan CallPipeline::master(const MasterRanges& r, bool serial) {
    MasterPlan p;
    p.record_back = true;
    if (!serial) {
        p.context = (current_ + 1) % CALL_CONTEXTS;
        bool dirty = dirty_ || r.reads_context_taps;
        for (const auto& call : recent_out_)
            for (const ByteRange& out : call)
                for (const ByteRange& in : r.in) dirty = dirty || overlap(in, out);
        p.pipelined = true;
        p.wait_context = busy_[p.context];
        p.wait_main = dirty;
        dirty_ = false;         // (the front stream is now behind everything main held)
    } else {
        // A call on main alone stays in the current context -- a handle that never pipelines (a lane of a batch) works in
        // one set of buffers, as it always did -- and needs no wait: the context's previous user put its back half on
        // main, where this call follows it.  The front stream has not moved past it, though: the next pipelined call
        // waits for main, whatever this call and the serial calls behind it write (only two calls' outputs are
        // remembered) or read (the other context's taps as fir_given).
        p.context = current_;
        dirty_ = true;
    }
    current_ = p.context;
    busy_[p.context] = true;
    for (int i = 0; i < 3; ++i) {
        recent_out_[1][i] = recent_out_[0][i];
        recent_out_[0][i] = r.out[i];
    }
    return p;
}

MasterPlan CallPipeline::replay() {
    MasterPlan p;
    p.context = current_;
    p.record_back = true;
    busy_[p.context] = true;
    return p;
}

void CallPipeline::drained() {
    dirty_ = false;
    for (bool& b : busy_) b = false;
    for (auto& call : recent_out_)
        for (ByteRange& out : call) out = ByteRange();
}

}  // namespace mgx
