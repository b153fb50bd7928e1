"""The early release of a call's context on the model of tests/test_call_pipeline_host.py, without a GPU.

The back half of a master call is two operations here, as master_call.h queues it:

  A = convolution + round 0 of the level correction: reads the context and the target, writes the handle's back buffers
      (y, mid, the band lists, the back state);
  B = tail / later rounds / scale / limiter: reads and writes only the handle's back buffers, writes the outputs.

The event that wait (a) of the context's next user waits for is recorded BETWEEN them.  The planner
(csrc/call_pipeline.cpp) is the one the library links, driven through the same C wrapper, and the invariant is the same:
any two operations that touch the same context, the back buffers or overlapping user ranges, one of them writing, are
ordered by a chain of same-stream and event edges or by a host synchronisation.  ``ReleaseModel(wrong=True)`` is the
library as it must NOT be -- B still reads the context -- and the invariant has to catch it.
"""

import numpy as np
import pytest

from test_call_pipeline_host import BACK, Model, buffers, lib  # noqa: F401  (lib: the fixture)


class ReleaseModel(Model):
    def __init__(self, lib, wrong=False):
        super().__init__(lib)
        self.wrong = wrong
        self.parts = []                             # per executed plan: (front, A, B) operation numbers

    def execute(self, plan):
        reads, target, outs = self.last_call
        c = plan.context
        k = len(self.plans) - 1
        if plan.pipelined:
            if plan.wait_context:
                self.wait("front", self.back_done[c])                      # (a): the context was released
            if plan.wait_main:
                self.wait("front", self.record("main"))                    # (b)
            front = self.op(f"front {k}", "front", reads, [("ctx", c)])        # (c)
            self.front_done[c] = self.record("front")
            self.wait("main", self.front_done[c])                          # (d)
        else:
            front = self.op(f"front {k}", "main", reads, [("ctx", c)])
        a = self.op(f"back A {k}", "main", [("ctx", c), target], [BACK])
        if plan.record_back:
            self.back_done[c] = self.record("main")                        # behind round 0, not behind the limiter
        b = self.op(f"back B {k}", "main", [BACK] + ([("ctx", c)] if self.wrong else []), list(outs) + [BACK])
        self.parts.append((front, a, b))
        return front, b

    def limit(self, x, out):
        """mgx_limit works in the handle's back state and buffers, in no context; it waits for its result."""
        self.lib.emu_pipeline_other_work(self.pipe)
        self.op("limit", "main", [x], [out, BACK])
        self.sync_main()


def drive(m, rng):
    """A generated sequence of entry points: masters on all three routes (outputs of the previous calls as inputs more
    often than chance would have it), runs of serial calls, uploads, downloads, mgx_limit, synchronisations, replays."""
    pool = buffers(rng, count=24)       # (many buffers, so that most calls are clean and their front halves run ahead)
    pick = lambda: pool[int(rng.randint(len(pool)))]         # noqa: E731
    stage_timing = siblings = False
    serial_run = 0
    written = []                                            # the outputs of the masters so far, latest last
    for _ in range(int(rng.randint(4, 28))):
        what = rng.choice(["master"] * 24 + ["upload", "upload", "download", "download_wait", "download_taps", "limit",
                                            "timing", "siblings", "serial_run", "serial_run", "sync", "replay"])
        if serial_run:
            what = "master"
        if what == "serial_run":
            serial_run = int(rng.randint(2, 5))
        elif what == "master":
            def recent():                                   # an output of one, two or three calls back, or any buffer
                if written and rng.rand() < 0.1:
                    outs = written[-int(rng.randint(1, min(3, len(written)) + 1))]
                    return outs[int(rng.randint(len(outs)))]
                return pick()
            route = rng.choice(["pair", "pair", "profile", "fir", "last_fir"])
            outs = [pick() for _ in range(int(rng.randint(1, 4)))]
            report = rng.rand() < 0.15 and not serial_run
            kwargs = dict(outs=outs, serial=stage_timing or siblings or serial_run > 0 or report)
            serial_run = max(0, serial_run - 1)
            if route == "profile":
                kwargs["profile"] = recent()
            else:
                kwargs["reference"] = recent()
            if route == "fir":
                kwargs["fir"] = recent()
            if route == "last_fir" and m.plans:
                c = m.plans[-1].context
                kwargs["fir_context"] = c
                kwargs["fir"] = (0x7000000 + 0x10000 * c, 0x7000000 + 0x10000 * c + 0x8000)
            m.master(recent(), **kwargs)
            written.append(outs)
            if report:
                m.sync_main()                               # the call waits for its scalars
        elif what == "upload":
            m.upload(pick())
        elif what == "download":
            m.download(pick(), wait=False)
        elif what == "download_wait":
            m.download(pick(), wait=True)
        elif what == "limit":
            m.limit(pick(), pick())
        elif what == "download_taps" and m.plans:
            m.download_taps(m.plans[-1].context)
        elif what == "timing":
            stage_timing = not stage_timing
        elif what == "siblings":
            siblings = not siblings
        elif what == "sync":
            m.sync_main()
        elif what == "replay" and m.plans:
            m.replay()


@pytest.mark.parametrize("seed", range(40))
def test_generated_sequences_keep_every_conflict_ordered(lib, seed):
    rng = np.random.RandomState(1000 + seed)
    for _ in range(10):
        m = ReleaseModel(lib)
        drive(m, rng)
        m.check()
        m.close()


def plain_masters(m, calls=6):
    pool = buffers(np.random.RandomState(0), count=12, aliased=False)
    for k in range(calls):
        plan = m.master(pool[2 * (k % 3)], reference=pool[2 * (k % 3) + 1], outs=[pool[6 + k]])
        assert plan.pipelined and not plan.wait_main and plan.wait_context == (k >= 2) and plan.record_back
    return pool


def test_the_front_half_runs_beside_the_rest_of_the_back_half_two_calls_before(lib):
    """What the release is for: front half k + 2 follows round 0 of call k (A) and nothing later of main."""
    m = ReleaseModel(lib)
    plain_masters(m)
    for k in range(2, 6):
        before = m.ops[m.parts[k][0]][4]
        assert m.parts[k - 2][1] in before, f"front half {k} does not wait for round 0 of call {k - 2}"
        assert m.parts[k - 2][2] not in before, f"front half {k} waits for the limiter of call {k - 2}"
        assert m.parts[k - 1][1] not in before and m.parts[k - 1][2] not in before
    m.check()
    m.sync_main()
    m.close()


def test_the_model_sees_a_back_half_that_still_reads_its_context(lib):
    """The deliberately wrong library: B reads the context that front half k + 2 is already writing."""
    m = ReleaseModel(lib, wrong=True)
    plain_masters(m, calls=4)
    with pytest.raises(AssertionError, match="unordered"):
        m.check()
    m.close()
    failed = 0
    rng = np.random.RandomState(7)
    for _ in range(50):                                     # ... and generated sequences run into it too
        m = ReleaseModel(lib, wrong=True)
        drive(m, rng)
        try:
            m.check()
        except AssertionError:
            failed += 1
        m.close()
    assert failed > 0


def test_output_of_call_k_as_input_of_call_k_plus_2(lib):
    """Front half k + 2 may now run while the limiter of call k writes: as its target or its reference that output
    makes the call dirty (the planner remembers two calls' outputs), and it waits for main."""
    for as_reference in (False, True):
        m = ReleaseModel(lib)
        pool = plain_masters(m, calls=3)
        out_k = m.last_call[2][0]                           # call 2's output
        m.master(pool[0], reference=pool[1], outs=[pool[10]])                   # call 3
        if as_reference:
            plan = m.master(pool[0], reference=out_k, outs=[pool[11]])          # call 4 reads call 2's output
        else:
            plan = m.master(out_k, reference=pool[1], outs=[pool[11]])
        assert plan.pipelined and plan.wait_main
        assert m.parts[2][2] in m.ops[m.parts[4][0]][4]
        m.check()
        m.close()


def test_replay_and_serial_calls_keep_the_order(lib):
    m = ReleaseModel(lib)
    pool = plain_masters(m, calls=3)
    m.replay()                                              # both streams drained, the last call again on main
    m.master(pool[0], reference=pool[1], outs=[pool[9]], serial=True)
    m.limit(pool[9], pool[10])
    assert m.master(pool[10], reference=pool[1], outs=[pool[11]]).pipelined
    m.master(pool[0], reference=pool[1], outs=[pool[9]])
    m.master(pool[0], reference=pool[1], outs=[pool[9]])
    m.check()
    m.close()
