"""Batch front end: many independent target/reference pairs on one or several MI355X.

The reference has no batch API (``core.process`` masters exactly one pair, core.py:32-121; batches
are left to the external matchering-cli, README.md:146-147).  Pairs share nothing, so the batch
axis shards without any data-path collective:

* across GPUs: pair ``i`` belongs to rank ``i mod world_size``, one process per GPU.  Ranks are read
  from the environment ``torch.distributed.run`` (or any launcher) sets -- RANK, WORLD_SIZE,
  LOCAL_RANK -- and no rank ever talks to another one here;
* inside a rank: ``lanes`` device handles (each its own HIP stream and workspace) are fed by one
  thread each.  A pair's kernels form a dependent chain with short single-workgroup links (FIR
  design, level-correction decisions, the limiter's look-back waits) and its PCIe copies run in one
  direction at a time; the other lanes fill those holes with other pairs' work (three by default: eight
  resident 4-minute pairs take 2.6 / 2.1 / 1.85 ms with one / two / three; ``MAX_LANES`` says why not many);
* around the GPU: reading and writing audio files is host work, so ``process_batch`` keeps ``io_threads``
  loaders ahead of the lanes (``intake``'s host step there, its device step on the lane) and writes results
  behind them (``delivery.write_results``).

``master_many`` works on arrays in memory, ``process_batch`` on files with the reference's
``Result`` objects.  Command line (one rank)::

    python -m matchering_amd.batch jobs.json

and on a node with 8 GPUs::

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m matchering_amd.batch jobs.json

``jobs.json`` is a list of ``{"target": path, "reference": path, "results": [{"file": path,
"subtype": "PCM_16", "use_limiter": true, "normalize": true, "delivery": {"loudness": -14, "true_peak": -1,
"dither": "tpdf_hp", "seed": 0, "limiter": true, "sample_rate": 48000}}, ...]}`` (``"delivery"`` and each of its keys
optional: ``delivery.Delivery``; ``"dither"``: a name -- "lipshitz5" and "wannamaker9" are noise shapers -- or
``{"coefficients": [...]}`` for a ``delivery.NoiseShaper`` of one's own; ``"limiter"``: ``true`` or the fields of
``delivery.TruePeakLimiter``; ``"sample_rate"``: the rate of that file in Hz, converted on the device, default the Config's internal rate); in place of ``"reference"`` a job may name a
``"reference_profile"``, the path of a profile saved by ``ReferenceProfile.save`` (profile.py), or ``"references"``, a
list of audio files and saved profiles that are merged into one profile (``ReferenceProfile.merge``).  A job may carry
``"eq": {"amount": 0.5, "max_boost_db": 6, "max_cut_db": 6, "phase": "minimum"}`` (every key optional:
``eq.MatchingEq``), the controls of its matching EQ, and ``"audit": true``: its tracks, renderings and deliveries are
audited (``qc.audit``) and the job carries the audits as plain dicts under ``"audit"`` afterwards; and
``"visuals": true`` or ``{"columns": 512, "bands": 64, ...}`` (``visuals.VisualsRequest``): the waveform overview and the
spectrogram of its tracks and renderings are made in HBM and the job carries them as plain dicts under ``"visuals"``.
"""

import json
import os
import queue
import sys
import threading

import numpy as np
from concurrent.futures import ThreadPoolExecutor

from .config import Config
from .log import Code, ModuleError, debug
from .results import Result


def rank_and_world(rank=None, world_size=None):
    """(rank, world_size, local_rank) from the arguments or the launcher's environment."""
    r = int(os.environ.get("RANK", "0")) if rank is None else int(rank)
    w = int(os.environ.get("WORLD_SIZE", "1")) if world_size is None else int(world_size)
    local = int(os.environ.get("LOCAL_RANK", str(r)))
    if not 0 <= r < w:
        raise ValueError(f"rank {r} outside world of {w}")
    return r, w, local


def shard(items, rank, world_size):
    """Indices of the items rank ``rank`` owns: ``i mod world_size == rank``."""
    return list(range(rank, len(items), world_size))


class _Lanes:
    """``lanes`` worker threads, each bound to its own device handle, draining one job queue."""

    def __init__(self, make_worker, lanes):
        # bounded: ``submit`` blocks while every lane is busy and one job per lane is waiting, so whoever
        # feeds the lanes (the file loaders of process_batch) runs only that far ahead of the GPU
        self.jobs = queue.Queue(maxsize=max(1, lanes))
        self.failure = None
        self.threads = [threading.Thread(target=self._run, args=(make_worker, lane), daemon=True)
                        for lane in range(lanes)]
        for t in self.threads:
            t.start()

    def _run(self, make_worker, lane):
        worker = None
        while True:
            item = self.jobs.get()
            if item is None:
                return
            index, payload, done = item
            try:
                if self.failure is not None:
                    raise RuntimeError("batch aborted")
                if worker is None:
                    worker = make_worker(lane)
                done(index, worker(payload), None)
            except BaseException as exc:           # recorded and re-raised by close()
                if self.failure is None:
                    self.failure = exc
                done(index, None, exc)

    def submit(self, index, payload, done):
        self.jobs.put((index, payload, done))

    def close(self):
        for _ in self.threads:
            self.jobs.put(None)
        for t in self.threads:
            t.join()
        if self.failure is not None:
            raise self.failure


_lane_devices = {}
_lane_devices_lock = threading.Lock()


# More lanes than this are not used: k_correction_tail keeps its <= 128 workgroups resident together (48 KB of
# LDS each: 768 fit the chip), and the tails of seven pairs dispatched side by side could each hold part of
# the slots and wait for the rest.
MAX_LANES = 6


_lane_choice = {}


def lanes_allowed(world_size=1):
    """MAX_LANES is a budget per GPU, not per process: ranks that share one GPU split it."""
    from .device import device_count

    sharing = max(1, -(-int(world_size) // max(1, device_count())))
    if sharing > 1:
        ranks_share_a_gpu()
    return max(1, MAX_LANES // sharing)


def ranks_share_a_gpu():
    """More rank PROCESSES than GPUs: their limiter launches can be resident on one chip together, where chunks dealt by
    workgroup number may wait for each other for ever (handle.h, LimiterChain -- handles of one process are chained,
    processes cannot see each other).  The library then deals chunks by an atomic ticket: slower by a fifth, safe with
    any neighbour.  Read by the library at every limiter launch."""
    os.environ.setdefault("MGX_LIMIT_TICKETS", "1")


_measuring = threading.Lock()


def choose_lanes(device_index=0, candidates=(2, 3), seconds=120.0, pairs=6, master=None, world_size=1):
    """How many device handles a batch should run on THIS GPU: measured, once per process and GPU.

    Boxes of the pool disagree: on some, three handles beat two by 10 % (1.87 vs 2.11 ms for eight resident
    4-minute pairs), on others three LOSE to two by 13 % (2.93 vs 2.60 ms; profiles/r02_lanes.txt,
    profiles/r02_g_bench_slow_box.json, BENCH_r02.json) -- so the number is not a constant of the code.  A
    short synthetic batch (``pairs`` resident pairs of ``seconds`` each -- six: a multiple of both candidate
    counts, so neither is handed an uneven share --, full pipeline) is timed through
    each candidate count and the fastest wins; the decision and both timings are kept in
    ``lane_choice_report(device_index)``.  Costs ~1 s of host time for the synthetic material and a few
    milliseconds of GPU time.  ``MGX_LANES=n`` skips the measurement; candidates above the per-GPU budget of
    ``lanes_allowed(world_size)`` are not tried (ranks that share a GPU would otherwise measure with more handles
    than they may use); one measurement at a time per process, each lane's device locked while it runs, and the
    blocks it recycled are given back afterwards."""
    if master is not None:                       # a stand-in for the GPU (CPU tests): nothing to measure
        return min(candidates[-1], MAX_LANES)
    forced = os.environ.get("MGX_LANES", "")
    if forced.isdigit() and int(forced) > 0:
        return min(int(forced), lanes_allowed(world_size))
    budget = lanes_allowed(world_size)
    candidates = tuple(c for c in candidates if c <= budget) or (budget,)
    if len(candidates) == 1:
        return candidates[0]
    with _measuring:
        with _lane_devices_lock:
            if device_index in _lane_choice:
                return min(_lane_choice[device_index]["lanes"], budget)
        import time
        from contextlib import ExitStack

        from .synth import make_pair

        native = Config().to_native()
        host = [make_pair(seconds, 44100, pair=300 + k) for k in range(pairs)]
        timings = {}
        for count in candidates:
            devs = [lane_device(device_index, lane) for lane in range(count)]
            with ExitStack() as held:
                for d in devs:
                    held.enter_context(d.lock)
                jobs = []
                for k, (t, r) in enumerate(host):
                    d = devs[k % count]
                    jobs.append((d, d.upload(t), t.shape[0], d.upload(r), r.shape[0], d.alloc(t.shape[0] * 8)))

                def step():
                    for d, t, n, r, nr, out in jobs:
                        d.master(t, n, r, nr, native, result=out, want_report=False)

                def sync():
                    for d in devs:
                        d.synchronize()

                def settled():
                    # the one-time switch of a handle to its safe mode (a GPU shared with somebody else's kernels,
                    # MGX_ERR_RETRY) belongs in front of the measurement, once per handle and kind of wait
                    from ._native import MgxError

                    for _ in range(2 * len(devs) + 1):
                        step()
                        try:
                            sync()
                            return
                        except MgxError as exc:
                            if not exc.retry:
                                raise
                    raise RuntimeError("the lanes' handles keep losing their launches")

                settled()
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    step()
                    step()
                    try:
                        sync()
                    except Exception as exc:             # (a switch in mid-measurement: this sample does not count)
                        if not getattr(exc, "retry", False):
                            raise
                        settled()
                        continue
                    took = (time.perf_counter() - t0) / 2
                    best = took if best is None else min(best, took)
                if best is None:
                    best = float("inf")
                timings[count] = best
                for d, t, n, r, nr, out in jobs:
                    for b in (t, r, out):
                        b.release()
                for d in devs:
                    d.trim()
        chosen = min(timings, key=timings.get)
        with _lane_devices_lock:
            _lane_choice[device_index] = {"lanes": chosen, "ms_per_batch": {str(k): round(v * 1e3, 3) for k, v in timings.items()},
                                          "batch": f"{pairs} resident pairs of {seconds:.0f} s"}
        return chosen


def lane_choice_report(device_index=0):
    return dict(_lane_choice.get(device_index, {}))


def lane_device(device_index, lane):
    """The device handle of lane ``lane`` on GPU ``device_index``: created once per process and kept --
    with it its FIR plans, workspaces and recycled HBM blocks, which a batch should not pay for twice."""
    from .device import Device

    with _lane_devices_lock:
        key = (device_index, lane)
        if key not in _lane_devices:
            _lane_devices[key] = Device(device_index)
        return _lane_devices[key]


def _device_worker(device_index, lane, config, needs, master, encodings=None):
    """A callable mastering one (target, reference) array pair on the lane's own device handle.
    ``encodings``: stages.main's (integer PCM renderings straight from the GPU).  ``deliveries`` (per call): a job's
    ``delivery.DeliveryRequest``, handed to ``main`` where the job has one; ``eq`` (per call): the job's
    ``eq.MatchingEq``, likewise; ``audit`` (per call): ``stages.main``'s handler, where the job asks for audits;
    ``visuals`` (per call): the same for its pictures; ``repair`` (per call): ``stages.main``'s, where the job asks for
    its target's clipping to be repaired."""
    def extra(deliveries, eq, audit, visuals=None, repair=None):
        given = {"deliveries": deliveries} if deliveries else {}
        if eq is not None:
            given["eq"] = eq
        if audit is not None:
            given["audit"] = audit
        if visuals is not None:
            given["visuals"] = visuals
        if repair is not None:
            given["repair"] = repair
        return given

    if master is not None:                         # tests inject a stand-in for the GPU
        if encodings is None or not any(encodings):
            return lambda pair, deliveries=None, eq=None, audit=None, visuals=None, repair=None: master(
                pair[0], pair[1], config, *needs, **extra(deliveries, eq, audit, visuals, repair))
        return lambda pair, deliveries=None, eq=None, audit=None, visuals=None, repair=None: master(
            pair[0], pair[1], config, *needs, encodings=encodings, **extra(deliveries, eq, audit, visuals, repair))
    from .stages import main

    dev = lane_device(device_index, lane)
    return lambda pair, deliveries=None, eq=None, audit=None, visuals=None, repair=None: main(
        pair[0], pair[1], config, *needs, device=dev, encodings=encodings, **extra(deliveries, eq, audit, visuals, repair))


def master_many(pairs, config=None, need_default=True, need_no_limiter=False,
                need_no_limiter_normalized=False, device_index=0, lanes=None, master=None, on_result=None, repair=None):
    """``stages.main`` over a list of (target, reference) arrays on ONE GPU, ``lanes`` pairs in flight
    (``None``: as many as ``choose_lanes`` measures to be best on this GPU).

    A pair's reference may be a ``profile.ReferenceProfile`` (uploaded once per lane device).  Returns the list of
    result triples in the order of ``pairs``.  Results are bit-identical to
    calling ``stages.main`` pair by pair: lanes only change when work is submitted, never what is
    computed.  With ``on_result(index, triple)`` every triple is handed over as it completes (from a lane
    thread) and NOT kept: the pinned host blocks the results live in are recycled as soon as the
    consumer lets go of them, and the returned list holds ``None``.  ``repair``: ``stages.main``'s, for every pair (a
    handler in it is called from the lane threads)."""
    from .repair import as_repair

    as_repair(repair)                                  # (ValueError before a device is touched)
    config = config if config is not None else Config()
    needs = (need_default, need_no_limiter, need_no_limiter_normalized)
    out = [None] * len(pairs)

    def done(index, value, exc):
        if on_result is not None and exc is None:
            on_result(index, value)
        else:
            out[index] = value

    if lanes is None:
        lanes = choose_lanes(device_index, master=master) if len(pairs) > 2 else 2
    def worker_for(lane):
        worker = _device_worker(device_index, lane, config, needs, master)
        return worker if repair is None else (lambda pair: worker(pair, repair=repair))

    pool = _Lanes(worker_for, max(1, min(lanes, MAX_LANES, len(pairs) or 1)))
    for i, pair in enumerate(pairs):
        pool.submit(i, pair, done)
    pool.close()
    return out


def master_album(targets, reference, config=None, rank=None, world_size=None, device_index=None, root=0,
                 exchange=None, need_default=True, need_no_limiter=False, need_no_limiter_normalized=False, eq=None,
                 repair=None):
    """Album mode across the ranks of one node: ONE matching FIR for every track.

    Rank ``root`` masters ``targets[0]`` against ``reference`` the ordinary way; the FIR pair it designed
    (2 x fft_size float32, 32 KiB at the default size) is the only thing that crosses xGMI -- one
    ``ncclBroadcast`` over RCCL -- and every rank then masters its share of the targets (track i -> rank
    i mod world) with that FIR given (``mgx_master_with_fir``), levels still matched per track.  Returns
    ``{index: triple}`` for this rank's tracks.  ``reference`` may be a ``profile.ReferenceProfile``: the reference
    is then never uploaded or analysed here (``mgx_master_with_profile``).  ``exchange(payload, size)`` must hand rank 0's 128-byte
    RCCL id to all ranks (bench.Ranks.broadcast_bytes); not needed with one rank.  ``eq`` (an ``eq.MatchingEq``) shapes
    the album's one FIR: it applies on the rank that designs it, every other call is given the shaped taps.  ``repair``:
    ``stages.main``'s, for every track -- the design pass hears the repaired first track too."""
    from .eq import as_eq
    from .repair import as_repair
    from .stages import main

    as_repair(repair)
    mended = {} if repair is None else {"repair": repair}

    config = config if config is not None else Config()
    eq = as_eq(eq)
    if eq is not None:
        eq.check(config)
    r, w, local = rank_and_world(rank, world_size)
    dev = lane_device(local if device_index is None else device_index, 0)
    needs = (need_default, need_no_limiter, need_no_limiter_normalized)
    count = 2 * config.fft_size
    mine = shard(targets, r, w)
    results = {}
    with dev.lock:
        fir = dev.alloc(count * 4)
        if r == root:                                           # the design pass; its result is track 0's
            first = main(targets[0], reference, config, *needs, device=dev, eq=eq, **mended)
            taps_ptr, taps = dev.last_fir()
            assert taps == config.fft_size
            designed = dev.download(taps_ptr, (count,))
            fir.release()
            fir = dev.upload(designed)
            if 0 in mine:
                results[0] = first
        dev.comm_init(r, w, exchange)
        try:
            dev.comm_broadcast(fir, count, root)
            dev.synchronize()
        finally:
            dev.comm_destroy()
        for i in mine:
            if i not in results:
                results[i] = main(targets[i], reference, config, *needs, device=dev, fir=fir, **mended)
        fir.release()
    return results


class _SharedReference:
    """``process_batch(share_references=True)``: the reference FILE of a job, left to the lane that masters the job --
    which analyses it once (``ReferenceProfile.analyze``) and masters every job that names the same file against
    that profile."""

    def __init__(self, path):
        self.path = path

    @property
    def key(self):
        try:
            st = os.stat(self.path)
            return (st.st_dev, st.st_ino)              # (what os.path.samefile compares)
        except OSError:
            return os.path.abspath(self.path)


class _ReferenceSet:
    """A job's "references": left to the lane that masters the job, which makes a profile of every element
    (``_analyze_reference`` for an audio file) and merges them (``ReferenceProfile.merge``)."""

    def __init__(self, items):
        self.items = list(items)

    @property
    def key(self):
        """What tells two sets apart: the elements in order (the order of a merge's float64 sums)."""
        return tuple(("object", id(item)) if _is_profile_object(item) else ("file", _SharedReference(item).key)
                     for item in self.items)


def _is_profile_object(item):
    from .profile import ReferenceProfile

    return isinstance(item, ReferenceProfile)


def _audio_files(job):
    """The audio files a job names as its reference, alone or in a set (saved profiles are not among them)."""
    from .profile import is_profile_file

    if job.get("references") is not None:
        return [item for item in job["references"] if not _is_profile_object(item) and not is_profile_file(item)]
    if job.get("reference") is not None and job.get("reference_profile") is None:
        return [job["reference"]]
    return []


def _analyze_reference(path, config, device):
    from .profile import ReferenceProfile

    return ReferenceProfile.analyze(path, config, device=device)


def _job_profile(job):
    """The ``ReferenceProfile`` of a job that names one ("reference_profile": the object or a saved file), else None."""
    from .profile import ReferenceProfile

    _job_reference_keys(job)
    given = job.get("reference_profile")
    if given is None:
        return None
    return given if isinstance(given, ReferenceProfile) else ReferenceProfile.load(given)


def _load_job(job, config, gpu=False, shared=False):
    """``intake``'s host step for both files of a job, on a loader thread.  Returns (target, reference, guard): the
    ``intake.Track``s, and whether the equality guard is left to the lane because it needs the frames the device converts
    (one that does not has run here, and fails the job before it takes a lane).  A job with a "reference_profile" or
    "references", or whose reference file is ``shared`` with other jobs (``process_batch``'s ``share_references``), loads
    its target only: ``reference`` is then the ``ReferenceProfile`` / a ``_ReferenceSet`` / a ``_SharedReference``."""
    from . import intake
    from .utils import get_temp_folder

    temp_folder = config.temp_folder if config.temp_folder else get_temp_folder(job["results"])
    target = intake.read(job["target"], "target", config, temp_folder, gpu, host_peaks=True)
    profile = _job_profile(job)
    several = _ReferenceSet(job["references"]) if job.get("references") is not None else None
    if profile is not None or several is not None or shared:
        if profile is not None:
            profile.matches(config)
        intake.validate(config, target)
        intake.no_equality_check(config)
        stand_in = profile if profile is not None else (several if several is not None else _SharedReference(job["reference"]))
        return target, stand_in, False
    reference = intake.read(job["reference"], "reference", config, temp_folder, gpu)
    guard = intake.guard_needs_frames(target, reference, config)
    if not guard:
        intake.equality_guard(target, reference, config)
    intake.validate(config, target, reference)
    return target, reference, guard


def _finish_tracks(target, reference, guard, dev, config):
    """``intake``'s device step for a job's tracks on the lane's device (``dev``: None with a stand-in for the GPU), then
    the equality guard ``_load_job`` left: what ``stages.main`` receives."""
    from . import intake

    with intake.released_on_error(target, reference):
        target.to_device(dev, config)
        if isinstance(reference, intake.Track):
            reference.to_device(dev, config)
            if guard:
                intake.equality_guard(target, reference, config)
            reference = reference.for_main
    return target.for_main, reference


class _WithDeliveries(tuple):
    """A job's triple of renderings with the ``DeliveryRequest`` that ``stages.main`` filled beside it."""

    def __new__(cls, triple, deliveries):
        self = super().__new__(cls, triple)
        self.deliveries = deliveries
        return self


def process_batch(jobs, config=None, rank=None, world_size=None, device_index=None, lanes=None, io_threads=4,
                  master=None, share_references=False, eq=None, repair=None):
    """``process`` for a list of jobs, this rank's share only.

    ``jobs``: dicts with "target", "reference" (paths) and "results" (list of ``Result``); in place of "reference" a
    job may name a "reference_profile" (a ``ReferenceProfile`` or the path of a saved one) or "references" (a list of
    audio files, saved profiles and ``ReferenceProfile``s, merged into one profile on the lane that masters the job).
    With ``share_references=True`` the jobs of this rank that name the same reference FILE (``os.path.samefile``), alone
    or in a set, have it loaded and analysed once per lane device and are mastered against that profile, and every
    distinct set is merged once per lane.  Off by default: the profile
    route agrees with the pair route to the project's tolerances, not bit for bit.  Returns
    the indices of the jobs this rank mastered.  The first failing job aborts the rank's batch and
    its exception is re-raised (after the jobs already in flight have finished).  ``eq``: the ``eq.MatchingEq`` of every
    job that has no "eq" of its own (an ``eq.MatchingEq`` or the JSON object of one); what the library refuses is a
    ValueError before a file is read.  A job with ``"audit": True`` has every track, rendering and delivery audited
    (``qc.audit``; the deliveries as the integer samples their files hold) and carries the audits afterwards as plain
    dicts under ``"audit"``, keyed "target", "reference", the renderings' names and "delivered:" + file.  ``repair``: the
    ``repair.ClipRepair`` (or its JSON: True, an object) of every job that has no "repair" of its own (``"repair": False`` on a job: none,
    whatever the batch's); a job that is
    repaired carries the ``Repaired`` of its target afterwards as a plain dict under ``"repaired"``."""
    from .delivery import DeliveryRequest, renderings_wanted, write_results
    from .eq import as_eq
    from .repair import as_repair

    config = config if config is not None else Config()
    r, w, local = rank_and_world(rank, world_size)
    mine = shard(jobs, r, w)
    eq = as_eq(eq)
    eqs, repairs = {}, {}
    for i in mine:
        if not jobs[i].get("results"):
            raise RuntimeError("The result list is empty")
        eqs[i] = as_eq(jobs[i]["eq"]) if jobs[i].get("eq") is not None else eq
        if eqs[i] is not None:
            eqs[i].check(config)
        repairs[i] = as_repair(jobs[i]["repair"] if jobs[i].get("repair") is not None else repair)
        # (a delivery rate the device converter refuses is a ValueError here, before a file is read)
        DeliveryRequest.for_results(jobs[i]["results"]).check_rates(config.internal_sample_rate)
    device_index = local if device_index is None else device_index
    savers = []
    shared_keys = set()
    if share_references:
        seen = {}
        for i in mine:
            for key in {_SharedReference(path).key for path in _audio_files(jobs[i])}:
                seen[key] = seen.get(key, 0) + 1
        shared_keys = {key for key, count in seen.items() if count > 1}

    def is_shared(job):
        return bool(shared_keys) and job.get("reference") is not None and job.get("reference_profile") is None \
            and _SharedReference(job["reference"]).key in shared_keys

    with ThreadPoolExecutor(max_workers=max(1, io_threads)) as io:
        def worker_for(lane):
            workers = {}
            profiles = {}                              # share_references: reference file -> its profile on this lane
            merged = {}                                # ... and set of references -> its merged profile

            def analysed(path, kept):
                key = _SharedReference(path).key
                if key not in kept:
                    kept[key] = _analyze_reference(
                        path, config, None if master is not None else lane_device(device_index, lane))
                return kept[key]

            def merged_set(several):
                """One profile per element -- with share_references the lane's own of a file it has analysed before --
                and their merge."""
                from .profile import ReferenceProfile, is_profile_file

                kept = profiles if share_references else {}
                sources = []
                for element in several.items:
                    if _is_profile_object(element) or is_profile_file(element):
                        profile = element if _is_profile_object(element) else ReferenceProfile.load(element)
                        profile.matches(config)
                        sources.append(profile)
                    else:
                        sources.append(analysed(element, kept))
                return ReferenceProfile.merge(sources, device=None if master is not None else lane_device(device_index, lane))

            def run(item):
                index, (target, reference, guard) = item
                if isinstance(reference, _SharedReference):
                    reference = analysed(reference.path, profiles)
                elif isinstance(reference, _ReferenceSet):
                    if not share_references:
                        reference = merged_set(reference)
                    else:
                        if reference.key not in merged:
                            merged[reference.key] = merged_set(reference)
                        reference = merged[reference.key]
                deliveries = DeliveryRequest.for_results(jobs[index]["results"])
                key = renderings_wanted(jobs[index]["results"])
                if key not in workers:
                    workers[key] = _device_worker(device_index, lane, config, key[0], master, key[1])
                target, reference = _finish_tracks(target, reference, guard,
                                                 None if master is not None else lane_device(device_index, lane), config)
                shaped = {} if eqs[index] is None else {"eq": eqs[index]}
                if jobs[index].get("audit"):
                    # "audit": true -> the job's audits as plain dicts, by the names stages.main's handler receives
                    audits = jobs[index]["audit"] = {}
                    shaped["audit"] = lambda name, value, kept=audits: kept.__setitem__(name, value.as_dict())
                if jobs[index].get("visuals"):
                    # "visuals": true or the sizes -> the job's pictures as plain dicts, by the same names
                    from .visuals import VisualsRequest

                    pictures, sizes = {}, VisualsRequest.from_json(jobs[index]["visuals"])
                    jobs[index]["visuals"] = pictures
                    shaped["visuals"] = (lambda name, value, kept=pictures: kept.__setitem__(name, value.as_dict()), sizes)
                handler, mend = repairs[index]
                if mend is not None:
                    def mended(name, value, job=jobs[index], also=handler):
                        job["repaired"] = value.as_dict()
                        if also is not None:
                            also(name, value)
                    shaped["repair"] = (mended, mend)
                if not deliveries:
                    return workers[key]((target, reference), **shaped)
                return _WithDeliveries(workers[key]((target, reference), deliveries, **shaped), deliveries)
            return run

        if lanes is None:
            lanes = choose_lanes(device_index, master=master, world_size=w) if len(mine) > 2 else 2
        lanes = min(max(1, lanes), MAX_LANES if master is not None else lanes_allowed(w))
        pool = _Lanes(worker_for, lanes)
        # Host memory stays bounded whatever the batch size: at most `io_threads` decoded pairs wait for
        # the lanes (the loaders are started one by one as their predecessors are consumed, and the lane
        # queue is bounded), and at most `lanes + io_threads` mastered triples wait for their writers.
        unsaved = threading.Semaphore(max(1, lanes) + max(1, io_threads))

        def done(index, triple, exc):
            if exc is None:
                unsaved.acquire()
                future = io.submit(write_results, jobs[index]["results"], tuple(triple), config.internal_sample_rate,
                                   getattr(triple, "deliveries", None))
                future.add_done_callback(lambda _f: unsaved.release())
                savers.append(future)

        ahead = {k: io.submit(_load_job, jobs[i], config, master is None, is_shared(jobs[i]))
                 for k, i in enumerate(mine[:io_threads])}
        nxt = len(ahead)
        try:
            for k, i in enumerate(mine):
                arrays = ahead.pop(k).result()            # (popped: the decoded arrays live on only in the job)
                if nxt < len(mine):
                    ahead[nxt] = io.submit(_load_job, jobs[mine[nxt]], config, master is None, is_shared(jobs[mine[nxt]]))
                    nxt += 1
                pool.submit(i, (i, arrays), done)
                del arrays
        finally:
            pool.close()
        for s in savers:
            s.result()
    if master is None:                       # a batch of varied track lengths leaves many size classes behind
        from .device import pinned

        for lane in range(lanes):
            lane_device(device_index, lane).trim()
        pinned.trim()
    return mine


def jobs_from_json(path):
    with open(path) as fh:
        raw = json.load(fh)
    jobs = []
    for item in raw:
        from .delivery import Delivery

        results = [Result(r["file"], subtype=r.get("subtype", "PCM_16"), use_limiter=r.get("use_limiter", True),
                          normalize=r.get("normalize", True),
                          delivery=None if r.get("delivery") is None else Delivery.from_json(r["delivery"]))
                   for r in item["results"]]
        job = {"target": item["target"], "results": results}
        if item.get("audit"):
            job["audit"] = True
        if item.get("visuals"):
            job["visuals"] = item["visuals"]
        if item.get("repair") is False:
            job["repair"] = False                  # (the job opts out of a batch-wide ``repair=``)
        elif item.get("repair") is not None:
            from .repair import ClipRepair

            job["repair"] = ClipRepair.from_json(item["repair"]).check()
        if item.get("eq") is not None:
            from .eq import MatchingEq

            job["eq"] = MatchingEq.from_json(item["eq"])
        for key in REFERENCE_KEYS:
            if item.get(key) is not None:
                job[key] = item[key]
        _job_reference_keys(job)
        jobs.append(job)
    return jobs


REFERENCE_KEYS = ("reference", "reference_profile", "references")


def _job_reference_keys(job):
    """A job names its reference exactly once: "reference" (an audio file), "reference_profile" (a saved profile) or
    "references" (a list of audio files and saved profiles, merged into one profile)."""
    named = [key for key in REFERENCE_KEYS if job.get(key) is not None]
    if len(named) != 1:
        raise ValueError(f'job for {job.get("target")!r}: exactly one of "reference", "reference_profile" and "references" '
                         f'is needed, got {named or "none of them"}')
    several = job.get("references")
    if several is not None and (not isinstance(several, (list, tuple)) or not several):
        raise ValueError(f'job for {job.get("target")!r}: "references" is a list of at least one file, got {several!r}')


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit(__doc__)
    jobs = jobs_from_json(argv[0])
    r, w, _ = rank_and_world()
    done = process_batch(jobs)
    print(f"rank {r}/{w}: mastered {len(done)} of {len(jobs)} pairs")


if __name__ == "__main__":
    main()
