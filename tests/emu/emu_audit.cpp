// The audit's run monoid (csrc/audit_kernel.h: audit_push, audit_combine, audit_finish) behind a C interface, so that
// tests/test_audit_host.py can fold a predicate sequence in any association on the host.  Test infrastructure.
#include "../../matchering_amd/csrc/audit_kernel.h"

using namespace mgx;

extern "C" {

// nine ints: start, len, prefix, suffix, best, best_at, events, samples, first
int emu_audit_run_ints() { return (int)(sizeof(AuditRun) / sizeof(int)); }

// the record of predicate[0 .. len), which lies at frames [start, start + len), element by element
void emu_audit_leaf(const unsigned char* predicate, int start, int len, int min_run, int* out) {
    AuditRun r = audit_empty(start);
    for (int i = 0; i < len; ++i) audit_push(r, predicate[i] != 0, min_run);
    *reinterpret_cast<AuditRun*>(out) = r;
}

void emu_audit_combine(const int* a, const int* b, int min_run, int* out) {
    *reinterpret_cast<AuditRun*>(out) =
        audit_combine(*reinterpret_cast<const AuditRun*>(a), *reinterpret_cast<const AuditRun*>(b), min_run);
}

void emu_audit_finish(const int* total, int min_run, int* out) {
    *reinterpret_cast<AuditRun*>(out) = audit_finish(*reinterpret_cast<const AuditRun*>(total), min_run);
}

void emu_audit_constants(long long* out) {
    out[0] = AUDIT_SEGMENT, out[1] = AUDIT_THREADS, out[2] = AUDIT_RUN, out[3] = AUDIT_SUBS_MAX, out[4] = AUDIT_MERGE_THREADS;
}

}  // extern "C"

#ifdef EMU_AUDIT_MAIN
// Stand-alone: the same fold over every split of a few sequences, for a run under the host sanitizers.
#include <cstdio>
#include <vector>
int main() {
    unsigned state = 12345u;
    int checked = 0;
    for (int round = 0; round < 200; ++round) {
        std::vector<unsigned char> p(round % 65);
        for (auto& v : p) v = ((state = state * 1664525u + 1013904223u) >> 24) < 150;
        const int n = (int)p.size(), min_run = 1 + round % 3;
        AuditRun whole = audit_empty(0);
        for (int i = 0; i < n; ++i) audit_push(whole, p[i] != 0, min_run);
        for (int cut = 0; cut <= n; ++cut) {
            AuditRun a = audit_empty(0), b = audit_empty(cut);
            for (int i = 0; i < cut; ++i) audit_push(a, p[i] != 0, min_run);
            for (int i = cut; i < n; ++i) audit_push(b, p[i] != 0, min_run);
            const AuditRun c = audit_combine(a, b, min_run);
            const AuditRun f = audit_finish(c, min_run), g = audit_finish(whole, min_run);
            if (f.best != g.best || f.best_at != g.best_at || f.events != g.events || f.samples != g.samples ||
                f.first != g.first || c.prefix != whole.prefix || c.suffix != whole.suffix) {
                std::printf("mismatch at round %d cut %d\n", round, cut);
                return 1;
            }
            ++checked;
        }
    }
    std::printf(checked > 6000 ? "ok\n" : "too few splits\n");
    return 0;
}
#endif
