"""The call pipeline's planner (csrc/call_pipeline.cpp) without a GPU.

The planner says, for every ``mgx_master`` call, which per-call context it uses and which event waits order its front
half (analysis, FIR design, filter spectra -- possibly on the front stream) against the rest.  The tests execute its
plans on a model of two in-order streams with events, exactly as ``queue_master`` in master_call.h does, and check the
invariant rather than the implementation: any two operations that touch the same context, the same back-half buffers
or overlapping user ranges, where at least one of them writes, are ordered by a chain of "same stream" and "event
wait" edges (or by a host synchronisation in between).
"""

import ctypes
import subprocess

import numpy as np
import pytest

import emu_build


@pytest.fixture(scope="module")
def lib():
    lib = emu_build.load("call_pipeline")
    lib.emu_pipeline_create.restype = ctypes.c_void_p
    lib.emu_pipeline_create.argtypes = []
    for name in ("destroy", "other_work", "drained"):
        getattr(lib, "emu_pipeline_" + name).restype = None
        getattr(lib, "emu_pipeline_" + name).argtypes = [ctypes.c_void_p]
    lib.emu_pipeline_current.restype = ctypes.c_int
    lib.emu_pipeline_current.argtypes = [ctypes.c_void_p]
    lib.emu_pipeline_master.restype = None
    lib.emu_pipeline_master.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int)]
    lib.emu_pipeline_replay.restype = None
    lib.emu_pipeline_replay.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    return lib


class Plan:
    def __init__(self, words):
        self.context, self.pipelined, self.wait_context, self.wait_main, self.record_back = (
            words[0], bool(words[1]), bool(words[2]), bool(words[3]), bool(words[4]))


BACK = ("back",)                # y, mid, band, block_peak, the limiter's words: what only back halves touch


class Model:
    """Two in-order streams, events, host synchronisations; the planner drives it as master_call.h executes its plans."""

    def __init__(self, lib):
        self.lib = lib
        self.pipe = lib.emu_pipeline_create()
        self.ops = []                               # (name, stream, reads, writes, ancestors)
        self.tail = {"main": frozenset(), "front": frozenset()}      # what the next operation of a stream follows
        self.base = frozenset()                     # what the host has waited for: everything later follows it
        self.front_done, self.back_done = {}, {}
        self.last_call = None
        self.plans = []
        self.taps_of = {}                           # context -> the pretend address range of its taps buffer

    def close(self):
        self.lib.emu_pipeline_destroy(self.pipe)

    # ---- the streams -------------------------------------------------------------
    def op(self, name, stream, reads=(), writes=()):
        ancestors = self.tail[stream] | self.base
        self.ops.append((name, stream, tuple(reads), tuple(writes), ancestors))
        self.tail[stream] = ancestors | {len(self.ops) - 1}
        return len(self.ops) - 1

    def record(self, stream):
        return self.tail[stream]

    def wait(self, stream, event):
        self.tail[stream] = self.tail[stream] | event

    def sync_main(self):
        """hipStreamSynchronize(main) from an entry point, then CallPipeline::drained -- which claims that the front
        stream is idle too: checked here."""
        self.base = self.base | self.tail["main"]
        assert self.tail["front"] <= self.base, "a front half was still in flight behind a synchronised main stream"
        self.lib.emu_pipeline_drained(self.pipe)

    # ---- entry points --------------------------------------------------------------
    def master(self, target, reference=None, profile=None, fir=None, outs=(), serial=False, fir_context=None):
        """``fir_context``: fir_given is the taps buffer of that context (mgx_last_fir's pointer)."""
        words = (ctypes.c_uint64 * 14)()
        for i, r in enumerate([target, reference, profile, fir]):
            if r is not None:
                words[2 * i], words[2 * i + 1] = r
        for i, r in enumerate(outs):
            words[8 + 2 * i], words[8 + 2 * i + 1] = r
        got = (ctypes.c_int * 5)()
        self.lib.emu_pipeline_master(self.pipe, words, int(fir_context is not None), int(serial), got)
        plan = Plan(got)
        assert self.lib.emu_pipeline_current(self.pipe) == plan.context
        reads = [r for r in (target, reference, profile, fir) if r is not None]
        if fir_context is not None and fir_context != plan.context:
            reads.append(("ctx", fir_context))
        self.last_call = (reads, target, tuple(outs))
        self.plans.append(plan)
        self.execute(plan)
        return plan

    def execute(self, plan):
        reads, target, outs = self.last_call
        c = plan.context
        k = len(self.plans) - 1
        if plan.pipelined:
            if plan.wait_context:
                self.wait("front", self.back_done[c])                      # (a)
            if plan.wait_main:
                self.wait("front", self.record("main"))                    # (b)
            front = self.op(f"front {k}", "front", reads, [("ctx", c)])        # (c)
            self.front_done[c] = self.record("front")
            self.wait("main", self.front_done[c])                          # (d)
        else:
            front = self.op(f"front {k}", "main", reads, [("ctx", c)])
        back = self.op(f"back {k}", "main", [("ctx", c), target], list(outs) + [BACK])
        if plan.record_back:
            self.back_done[c] = self.record("main")
        return front, back

    def replay(self):
        """check_device_error queues the last call again: both streams drained, then main alone."""
        self.base = self.base | self.tail["main"] | self.tail["front"]
        got = (ctypes.c_int * 5)()
        self.lib.emu_pipeline_replay(self.pipe, got)
        plan = Plan(got)
        assert not plan.pipelined and plan.context == self.plans[-1].context
        self.plans.append(plan)
        self.execute(plan)
        self.sync_main()

    def upload(self, r):
        self.lib.emu_pipeline_other_work(self.pipe)
        self.op("upload", "main", [], [r])

    def download(self, r, wait):
        self.op("download", "main", [r], [])                # (writes no device memory: the planner is not told)
        if wait:
            self.sync_main()

    def download_taps(self, context):
        """A download of mgx_last_fir's table, a context's own taps: mgx_memcpy_d2h_async tells the planner of this one."""
        self.lib.emu_pipeline_other_work(self.pipe)
        self.op("download taps", "main", [("ctx", context)], [])

    def limit(self, x, out):
        """mgx_limit: the most recent context's scalars, the limiter's buffers; it waits for its result."""
        self.lib.emu_pipeline_other_work(self.pipe)
        current = self.lib.emu_pipeline_current(self.pipe)
        self.op("limit", "main", [x], [out, ("ctx", current), BACK])
        self.sync_main()

    # ---- the invariant ---------------------------------------------------------------
    @staticmethod
    def _clash(a, b):
        if isinstance(a[0], str) or isinstance(b[0], str):
            return a == b
        return a[0] < b[1] and b[0] < a[1]

    def check(self):
        for j, (name_j, _, reads_j, writes_j, before_j) in enumerate(self.ops):
            for i in range(j):
                if i in before_j:
                    continue
                name_i, _, reads_i, writes_i, _ = self.ops[i]
                for w in writes_i:
                    for x in reads_j + writes_j:
                        assert not self._clash(w, x), f"{name_i} writes {w}, {name_j} touches {x}: unordered"
                for w in writes_j:
                    for x in reads_i:
                        assert not self._clash(w, x), f"{name_i} reads {x}, {name_j} writes {w}: unordered"


def buffers(rng, count=7, aliased=True):
    """Disjoint user ranges, and (``aliased``) a few more that straddle two of them."""
    out = [(0x10000 * (i + 1), 0x10000 * (i + 1) + 0x8000) for i in range(count)]
    if aliased:
        for _ in range(3):
            i = int(rng.randint(count))
            out.append((out[i][0] + 0x4000, out[i][0] + 0xc000))
    return out


@pytest.mark.parametrize("seed", range(40))
def test_generated_sequences_keep_every_conflict_ordered(lib, seed):
    rng = np.random.RandomState(seed)
    for _ in range(10):
        m = Model(lib)
        pool = buffers(rng)
        pick = lambda: pool[int(rng.randint(len(pool)))]         # noqa: E731
        stage_timing = siblings = False             # either keeps calls on main alone, and neither synchronises
        serial_run = 0                              # masters still to come of a run of unsynchronised serial calls
        for _ in range(int(rng.randint(4, 28))):
            what = rng.choice(["master"] * 8 + ["upload", "upload", "download", "download_wait", "download_taps", "limit",
                                                "timing", "siblings", "serial_run", "serial_run", "sync", "replay"])
            if serial_run:
                what = "master"
            if what == "serial_run":
                serial_run = int(rng.randint(2, 5))
            elif what == "master":
                route = rng.choice(["pair", "pair", "profile", "fir", "last_fir"])
                outs = [pick() for _ in range(int(rng.randint(1, 4)))]
                report = rng.rand() < 0.15 and not serial_run
                kwargs = dict(outs=outs, serial=stage_timing or siblings or serial_run > 0 or report)
                serial_run = max(0, serial_run - 1)
                if route == "profile":
                    kwargs["profile"] = pick()
                else:
                    kwargs["reference"] = pick()
                if route == "fir":
                    kwargs["fir"] = pick()
                if route == "last_fir" and m.plans:
                    kwargs["fir_context"] = m.plans[-1].context
                    kwargs["fir"] = (0x7000000 + 0x10000 * m.plans[-1].context, 0x7000000 + 0x10000 * m.plans[-1].context + 0x8000)
                serial = kwargs["serial"]
                m.master(pick(), **kwargs)
                if report:
                    m.sync_main()                                   # the call waits for its scalars
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
        m.check()
        m.close()


@pytest.mark.parametrize("one_output", [False, True])
def test_plain_masters_run_ahead(lib, one_output):
    """Back-to-back masters on disjoint buffers (and, as bench.py, all into one output): every front half is on the
    front stream and waits for nothing but back_done of call k - 2, so it is NOT ordered behind call k - 1's back half."""
    m = Model(lib)
    pool = buffers(np.random.RandomState(0), count=12, aliased=False)
    pairs = [(pool[0], pool[1]), (pool[2], pool[3]), (pool[4], pool[5])]
    fronts, backs = [], []
    for k in range(6):
        target, reference = pairs[k % 3]
        plan = m.master(target, reference=reference, outs=[pool[6] if one_output else pool[6 + k]])
        assert plan.pipelined and not plan.wait_main
        assert plan.context == (k + 1) % 2 and plan.wait_context == (k >= 2) and plan.record_back
        fronts.append(len(m.ops) - 2)
        backs.append(len(m.ops) - 1)
    for k in range(1, 6):
        before = m.ops[fronts[k]][4]
        assert backs[k - 1] not in before, f"front half {k} waits for back half {k - 1}"
        assert (backs[k - 2] in before) == (k >= 2)
    m.check()
    m.sync_main()
    plan = m.master(pool[0], reference=pool[1], outs=[pool[6]])
    assert plan.pipelined and not plan.wait_context and not plan.wait_main      # nothing in flight after a synchronisation
    m.close()


@pytest.mark.parametrize("why", ["stage timing", "siblings"])
@pytest.mark.parametrize("serial_calls", [1, 2, 3])
@pytest.mark.parametrize("back", [3, 4])
def test_serial_calls_between_pipelined_ones(lib, why, serial_calls, back):
    """Pipelined calls, then calls on main alone with no synchronisation (stage timing switched on, or a sibling handle
    created, for their length: the planner sees `serial` either way), then a pipelined call that reads the output of call
    k - 3 or k - 4: older than the two calls whose outputs the planner remembers, and written on main, which the front
    stream has not waited for since.  It must wait for main."""
    m = Model(lib)
    pool = buffers(np.random.RandomState(0), count=14, aliased=False)
    outs = []
    for k in range(3):
        outs.append(pool[4 + k])
        assert m.master(pool[0], reference=pool[1], outs=[outs[-1]]).pipelined
    for k in range(serial_calls):
        outs.append(pool[8 + k])
        assert not m.master(pool[0], reference=pool[1], outs=[outs[-1]], serial=True).pipelined
    plan = m.master(outs[-back], reference=pool[1], outs=[pool[12]])
    assert plan.pipelined and plan.wait_main
    plan = m.master(pool[0], reference=outs[-back + 1], outs=[pool[13]])
    assert plan.pipelined
    m.check()
    m.close()


def test_a_download_of_the_taps_holds_the_next_front_half_back(lib):
    m = Model(lib)
    pool = buffers(np.random.RandomState(0), count=8, aliased=False)
    for k in range(3):
        m.master(pool[0], reference=pool[1], outs=[pool[2 + k]])
    m.download_taps(m.plans[-1].context)
    assert m.master(pool[0], reference=pool[1], outs=[pool[5]]).wait_main
    m.master(pool[0], reference=pool[1], outs=[pool[6]])                 # ... which writes the taps the copy reads
    m.check()
    m.close()


def test_dirty_calls_wait_for_main(lib):
    m = Model(lib)
    pool = buffers(np.random.RandomState(0), count=10, aliased=False)
    a = m.master(pool[0], reference=pool[1], outs=[pool[2]])
    assert not a.wait_main
    assert m.master(pool[2], reference=pool[1], outs=[pool[3]]).wait_main           # call k's result is call k + 1's target
    assert not m.master(pool[0], reference=pool[1], outs=[pool[4]]).wait_main
    assert m.master(pool[0], reference=pool[3], outs=[pool[5]]).wait_main           # ... the output of two calls ago
    m.upload(pool[0])
    assert m.master(pool[0], reference=pool[1], outs=[pool[6]]).wait_main           # other work on main since
    assert not m.master(pool[0], reference=pool[1], outs=[pool[6]]).wait_main
    m.download(pool[6], wait=False)
    assert not m.master(pool[0], reference=pool[1], outs=[pool[7]]).wait_main       # a download writes nothing on the device
    last = m.master(pool[0], reference=pool[1], outs=[pool[7]], fir=(0x7000000, 0x7008000), fir_context=m.plans[-1].context)
    assert last.wait_main                                                           # fir_given in a context's own taps
    serial = m.master(pool[0], reference=pool[1], outs=[pool[8]], serial=True)
    assert not serial.pipelined and not serial.wait_main and not serial.wait_context
    m.upload(pool[1])
    serial = m.master(pool[0], reference=pool[1], outs=[pool[8]], serial=True)
    assert m.master(pool[0], reference=pool[1], outs=[pool[9]]).wait_main           # the upload is still ahead of the front stream
    m.check()
    m.close()


def test_a_handle_that_never_pipelines_stays_in_one_context(lib):
    """Every call serial (a lane of a batch, whose device has several handles): one context, main alone, no waits."""
    m = Model(lib)
    pool = buffers(np.random.RandomState(0), count=6, aliased=False)
    for k in range(5):
        if k == 2:
            m.upload(pool[0])
        plan = m.master(pool[0], reference=pool[1], outs=[pool[2 + k % 3]], serial=True)
        assert (plan.context, plan.pipelined, plan.wait_context, plan.wait_main) == (0, False, False, False)
    m.replay()
    assert all(stream == "main" for _, stream, _, _, _ in m.ops)
    m.check()
    m.close()


def test_standalone_driver_under_sanitizers(tmp_path):
    """The same unit in a program of its own, built with AddressSanitizer and UBSan, run once (nothing loaded into
    Python runs under a sanitizer)."""
    out = str(tmp_path / "driver")
    emu_build.build_driver("call_pipeline", out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    done = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "round 1:" in done.stdout
