"""GPU tier: the device-pointer entries under callers that do not synchronise (include/sbv.h: "asynchronous on `hip_stream`").

Every other file of the tier drains the device before a `_dev` call and synchronises right behind it, so nothing there can see a side stream
of a grouped step that starts reading the caller's tuples too early, one that is never joined back before the caller's next operation
overwrites them, a tail of one batch that the next scheme's grouping overruns, or a buffer that grows while a call is queued (DESIGN.md,
"Stream contract", lists every such edge).  The symptom of a missing edge is a wrong verdict that depends on timing.  Here every call goes
through the C-ABI on a stream whose head holds a device-side DELAY, everything is enqueued without a host wait and the first synchronisation
comes at the very end; the inputs are the complementary pairs of tests/stream_cases.py (X accepts the even tuples, Y the odd ones: a read
of the wrong generation flips verdicts, a mixed one gives a bitmap equal to neither), and every bitmap is compared bit for bit.

The delay is sized at run time: ten times one warm call of the same entry, size and cache mode, timed with events in this process (at
least DELAY_MIN_MS, which covers the host's enqueue time of the few hundred API calls of the longest schedule; at most DELAY_MAX_MS), from a
calibration of torch.cuda._sleep (a chain of large element-wise ops where a torch build lacks it).  Where a schedule holds no host wait of
the library's own, an event behind the delay must still be pending after the last enqueue: the GPU had the whole sequence queued before it
ran any of it.

Control.  A process has a handful of hardware queues and the library owns three or four streams, so some streams share a queue with a
library stream: work of that library stream then serialises behind the delay and a missing edge could not show.  Per candidate stream the
late-producer schedule runs once with the delay and the producer on the candidate and the call on ANOTHER stream, with no event between
them: the library must see the stale generation — the bitmap must be X's.  Only candidates for which it is are used; the schedules
across streams ask for two or three DIFFERENT ones and fail, saying so, where the control found fewer (four candidates, then more,
until three are accepted or twelve were tried).

The legacy NULL stream is what torch's current stream is on this platform unless a test makes another one current, and the rest of the tier
calls the entries on it: it has no schedule of its own.  Stream capture is out of scope (the entries allocate and, for `_dev_part`,
synchronise inside the call): nothing here captures a graph or touches queue settings."""
import collections
import itertools
import threading

import numpy as np
import pytest

import consensus_amd as sbv
import group_model as gm
import stream_cases as sc

pytestmark = pytest.mark.gpu

SCHEDULES = ("late_producer", "early_overwriter", "back_to_back", "across_schemes", "growth", "host_call", "setters", "threads", "parts")
Entry = collections.namedtuple("Entry", "scheme kind call schedules")
_GENERIC = ("late_producer", "early_overwriter", "back_to_back", "across_schemes", "growth", "host_call", "setters", "threads")
_KEYED = ("late_producer", "early_overwriter", "back_to_back", "growth", "host_call", "setters")
# every `_dev` / `_dev_part` entry of include/sbv.h (tests/test_stream_cases_cpu.py compares this table with the header) -> the wrapper
# that calls it and the schedules below that run it.  The signer reads nothing of the library's that a call or a setter can free or
# rewrite (the comb of G alone; no scratch, no busy event) and enqueues on the caller's stream only: growth, setters and threads have
# nothing of it to order, the host-pointer schedule runs it once.  The part entry synchronises its stream inside the call, so it cannot be
# queued behind anything: its own schedule puts the delay in front of the whole sequence.
ENTRIES = {
    "sbv_p256_verify_batch_dev": Entry("p256", "generic", "verify_batch_dev", _GENERIC),
    "sbv_secp256k1_verify_batch_dev": Entry("k256", "generic", "secp256k1_verify_batch_dev", _GENERIC),
    "sbv_ed25519_verify_batch_dev": Entry("ed25519", "generic", "ed25519_verify_batch_dev", _GENERIC),
    "sbv_p256_verify_batch_keyed_dev": Entry("p256", "keyed", "verify_batch_keyed_dev", _KEYED + ("across_schemes",)),
    "sbv_secp256k1_verify_batch_keyed_dev": Entry("k256", "keyed", "secp256k1_verify_batch_keyed_dev", _KEYED),
    "sbv_ed25519_verify_batch_keyed_dev": Entry("ed25519", "keyed", "ed25519_verify_batch_keyed_dev", _KEYED),
    "sbv_p256_sign_batch_dev": Entry("p256", "sign", "sign_batch_dev", ("late_producer", "early_overwriter", "back_to_back", "host_call")),
    "sbv_p256_verify_batch_dev_part": Entry("p256", "part", "verify_batch_dev_part", ("parts",)),
}
GENERIC = [name for name, e in ENTRIES.items() if e.kind == "generic"]
KEYED = [name for name, e in ENTRIES.items() if e.kind == "keyed"]
GENERIC_OF = {ENTRIES[name].scheme: name for name in GENERIC}
KEYED_OF = {ENTRIES[name].scheme: name for name in KEYED}
SCHEME_ID = {"p256": sbv.SCHEME_P256, "k256": sbv.SCHEME_SECP256K1, "ed25519": sbv.SCHEME_ED25519}
HOST_CALL = {"p256": "verify_batch", "k256": "secp256k1_verify_batch", "ed25519": "ed25519_verify_batch"}
REGISTER = {"p256": "register_keys", "k256": "secp256k1_register_keys", "ed25519": "ed25519_register_keys"}
WIDEN = {"p256": "widen_keys", "k256": "secp256k1_widen_keys", "ed25519": "ed25519_widen_keys"}
CLEAR = {"p256": "clear_keys", "k256": "secp256k1_clear_keys", "ed25519": "ed25519_clear_keys"}
HOT = {"p256": "hot_keys", "k256": "k256_hot_keys", "ed25519": "ed_hot_keys"}
HOT_STATS = {"p256": "hot_key_stats", "k256": "k256_hot_key_stats", "ed25519": "ed_hot_key_stats"}
DELAY_MIN_MS, DELAY_MAX_MS, DELAY_FACTOR = 30.0, 300.0, 10.0
PARTS = 3
MAX_CANDIDATES = 12
PATTERN = 0xA5
TIMES = {}                                                   # (entry, n, mode) -> ms of one warm call: what the delays were sized from


class Delay:
    """A device-side delay on the current stream, calibrated once with events."""

    def __init__(self, torch):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:                                # a chain of large element-wise ops instead
            self.big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
        self.unit = 1_000_000 if self.sleep else 4            # cycles / ops
        self._run(self.unit)
        torch.cuda.synchronize()
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self._run(self.unit)
            b.record()
            torch.cuda.synchronize()
            self.unit_ms = a.elapsed_time(b)
            if self.unit_ms >= 5.0 or self.unit >= 1 << 40:
                break
            self.unit *= 4
        self.per_ms = self.unit / self.unit_ms

    def _run(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.big.mul_(1.0)

    def __call__(self, ms):
        self._run(max(1, round(ms * self.per_ms)))


class Job:
    """One entry on one pair: device-resident sources of both generations, the input buffers the library reads, outputs of twice the size
    the library writes (the second half belongs to the caller) and pinned host memory for the results.  Everything stays alive with the
    job: keep it until the final synchronisation."""

    def __init__(self, ctx, name, data, parts=PARTS):
        torch = ctx.torch
        self.ctx, self.name, self.entry, self.data = ctx, name, ENTRIES[name], data
        e = self.entry
        self.fn = getattr(sbv, e.call)
        self.parts = parts
        if e.kind == "sign":
            keys, index, dx, dy = data
            self.n = dx.shape[0]
            self.fixed = [torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda(), torch.from_numpy(index.view(np.int32).copy()).cuda()]
            self.nkeys = len(keys) // 32
            src = {"x": [dx], "y": [dy]}
            self.out_bytes = 65 * self.n
        else:
            self.n = data.n
            if e.kind == "keyed":
                reg = np.array(getattr(sbv, REGISTER[e.scheme])(data.keys), dtype=np.uint32)       # equal keys share a slot: registering again is a lookup
                src = {g: [data.keyed(g)[0], reg[data.keyed(g)[1]].view(np.int32)] for g in "xy"}
            else:
                src = {g: [data.rows(g)] for g in "xy"}
            self.out_bytes = 4 * ((self.n + 31) // 32) if e.kind == "part" else (self.n + 7) // 8
        self.src = {g: [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs] for g, arrs in src.items()}
        self.bufs = [torch.empty_like(t) for t in self.src["x"]]
        self.half = (self.out_bytes + 15) & ~15
        self.outs, self.hosts, self.used = [], [], 0
        for _ in range(4):
            self.new_out()
        self.used = 0
        if e.kind == "part":
            self.rows = torch.zeros((parts, self.out_bytes // 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def want(self, g):
        if self.entry.kind == "sign":
            return self.ctx.signatures(self.data, g)
        w = self.data.want(g)
        return w + bytes(self.out_bytes - len(w))

    def fill(self, g):
        """generation g into the input buffers, finished when it returns"""
        self.produce(g)
        self.ctx.torch.cuda.synchronize()

    def produce(self, g):
        """device-to-device copies of generation g into the input buffers, on the current stream"""
        for dst, s in zip(self.bufs, self.src[g]):
            dst.copy_(s, non_blocking=True)

    def new_out(self):
        """index of an unused output; the first few exist from the start, so that nothing is allocated while a delay runs"""
        torch = self.ctx.torch
        if self.used == len(self.outs):
            self.outs.append(torch.full((2 * self.half,), 0x3C, dtype=torch.uint8, device="cuda"))
            self.hosts.append(torch.zeros(2 * self.half, dtype=torch.uint8).pin_memory())
        self.used += 1
        return self.used - 1

    def call(self, stream, k=None, read=True):
        """the entry on `stream` (which must be torch's current stream) into output k (a new one by default), then the copy of the output into pinned memory"""
        if k is None:
            k = self.new_out()
        out, sp, e = self.outs[k], stream.cuda_stream, self.entry
        if e.kind == "generic":
            self.fn(self.bufs[0].data_ptr(), self.n, out.data_ptr(), sp)
        elif e.kind == "keyed":
            self.fn(self.bufs[0].data_ptr(), self.bufs[1].data_ptr(), self.n, out.data_ptr(), sp)
        elif e.kind == "sign":
            self.fn(self.fixed[0].data_ptr(), self.nkeys, self.fixed[1].data_ptr(), self.bufs[0].data_ptr(), self.n, out.data_ptr(), out.data_ptr() + 64 * self.n, sp)
        else:
            self.call_parts([stream] * self.parts, k)
        if read:
            self.read(k)
        return k

    def call_parts(self, streams, k):
        """part p on streams[p] into row p of one word array; the caller joins the streams before assemble()"""
        total = 0
        for p, st in enumerate(streams):
            total += self.fn(self.bufs[0].data_ptr(), self.n, p, self.parts, self.rows[p].data_ptr(), st.cuda_stream)
        assert total == self.n, (total, self.n)
        if len(set(streams)) == 1:
            self.assemble(k)

    def assemble(self, k):
        acc = self.rows[0]
        for p in range(1, self.parts):
            acc = acc | self.rows[p]
        self.outs[k][:self.out_bytes].view(self.ctx.torch.int32).copy_(acc)

    def read(self, k):
        self.hosts[k].copy_(self.outs[k], non_blocking=True)

    def overwrite(self, g):
        """what a caller may do right behind the call: reuse the inputs, and write into its own half of the output allocations"""
        self.produce(g)
        for out in self.outs:
            out[self.half:].fill_(PATTERN)

    def got(self, k):
        return self.hosts[k][:self.out_bytes].numpy().tobytes()

    def check(self, k, g, what=""):
        got, want = self.got(k), self.want(g)
        if got != want:
            other = self.want("x" if g == "y" else "y")
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            kind = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s n=%d %s: output %d is not generation %s's but %s" % (self.name, self.n, what, k, g.upper(), kind))


class Ctx:
    def __init__(self, torch, oracle):
        self.torch, self.oracle = torch, sc.prepare(oracle)
        self.delay = Delay(torch)
        self.probe = torch.cuda.Stream()
        self.candidates = [torch.cuda.Stream() for _ in range(4)]
        self.streams, self.verdicts = [], []
        self.mode = None
        self._sigs = {}

    def pair(self, scheme, n, tail=True):
        return sc.pair(self.oracle, scheme, n, sc.SINGLES if tail and n == sc.MAIN else 0)

    def job(self, name, n=sc.MAIN, tail=True):
        if ENTRIES[name].kind == "sign":
            return Job(self, name, sc.digest_pair(n))
        return Job(self, name, self.pair(ENTRIES[name].scheme, n, tail))

    def signatures(self, data, g):
        """The blocking host-pointer entry on a drained device is the reference of the signer's device-pointer entry: no independent one,
        which the ordering does not need (RFC 6979 signatures are deterministic, and every signature of X differs from its twin of Y).  The
        signer's arithmetic is held to the host signer, the RFC's known answers and the oracle in tests/test_gpu_sign.py."""
        keys, index, dx, dy = data
        key = (dx.shape[0], g)
        if key not in self._sigs:
            self.torch.cuda.synchronize()
            sigs, ok = sbv.sign_batch(keys, (dx if g == "x" else dy).tobytes(), [int(i) for i in index])
            assert ok == b"\x01" * dx.shape[0]
            self._sigs[key] = sigs + ok
        return self._sigs[key]

    def stream(self):
        """the first stream the control accepted"""
        assert self.streams, "the delay holds nothing back on any candidate stream (%s)" % ", ".join(self.verdicts)
        return self.streams[0]

    def distinct(self, k):
        """k different streams the control accepted: a schedule across streams run on fewer proves nothing about them"""
        assert len(self.streams) >= k, ("this schedule needs %d distinct streams on which the delay holds nothing of the library back; the control accepted %d of %d candidates (%s)"
                                        % (k, len(self.streams), len(self.verdicts), ", ".join(self.verdicts)))
        return self.streams[:k]

    def set_mode(self, mode):
        """cold: every key-table cache off; warm: on; hot: on, emptied, and every scheme's hot-key pool on with 64 combs from 64 hits on —
        a signer of the main pairs (85 uses or more per batch) is promoted behind the first batch that meets it.  Grouped from 64 tuples."""
        self.torch.cuda.synchronize()
        sbv.set_grouping(True, 64, 0, 0)
        for s in SCHEME_ID.values():
            sbv.key_cache(mode != "cold", 0, s)
        if mode == "hot":
            for s in SCHEME_ID.values():
                sbv.key_cache(False, 0, s)
                sbv.key_cache(True, 0, s)
            for scheme in HOT:
                getattr(sbv, HOT[scheme])(64, 64)
        elif self.mode == "hot":
            restore_hot_pools()
        self.mode = mode

    def call_ms(self, job):
        """One blocking call of the job's entry at its size in the current mode — whatever the library allocates or builds lazily exists
        afterwards, so that no schedule pays for it while its delay runs — and, once per (entry, size, mode), a second one timed with events."""
        torch = self.torch
        key = (job.name, job.n, self.mode)
        job.fill("y")
        used = job.used
        with torch.cuda.stream(self.probe):
            k = job.call(self.probe, read=False)
            self.probe.synchronize()
            if key not in TIMES:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(self.probe)
                job.call(self.probe, k, read=False)
                b.record(self.probe)
                torch.cuda.synchronize()
                TIMES[key] = a.elapsed_time(b)
        torch.cuda.synchronize()
        job.used = used
        return TIMES[key]

    def delay_ms(self, *jobs):
        ms = DELAY_FACTOR * sum(self.call_ms(j) for j in jobs)
        assert ms <= DELAY_MAX_MS, "ten warm calls take %.0f ms: the delay would pass its cap of %.0f ms" % (ms, DELAY_MAX_MS)
        return max(ms, DELAY_MIN_MS)

    def held_back(self, stream, ms):
        """the delay at the head of `stream` (torch's current one) and an event behind it: pending for as long as the delay runs"""
        self.delay(ms)
        gate = self.torch.cuda.Event()
        gate.record(stream)
        return gate

    def finish(self, gates, host_waits=False):
        """the first synchronisation of a schedule.  Without host waits inside the library the delays must still be running here."""
        pending = [not g.query() for g in gates]
        self.torch.cuda.synchronize()
        if not host_waits:
            assert all(pending), "a delay ran out before the schedule was enqueued: it proves nothing"


def restore_hot_pools():
    sbv.hot_keys(1024, 4096)
    sbv.ed_hot_keys(1024, 4096)
    sbv.k256_hot_keys(0, 4096)


def run_control(ctx, n, want=1):
    """Which candidate streams hold nothing of the library back (module docstring).  A grouped cold batch: every stream of the step has work.
    The calling stream must not share a queue with the candidate either: the probe stream first, then the other candidates, until one
    shows the stale generation.  Four candidates; while fewer than `want` are accepted (the schedules across streams need three different
    ones, and the streams of a process share a handful of hardware queues with the library's), further ones up to MAX_CANDIDATES."""
    torch = ctx.torch
    ctx.set_mode("cold")
    job = ctx.job("sbv_p256_verify_batch_dev", n)
    ms = ctx.delay_ms(job)
    ctx.streams, ctx.verdicts = [], []
    at = 0
    while at < 4 or (len(ctx.streams) < want and at < MAX_CANDIDATES):
        if at == len(ctx.candidates):
            ctx.candidates.append(torch.cuda.Stream())
        s = ctx.candidates[at]
        at += 1
        seen = []
        for caller in [ctx.probe] + [c for c in ctx.candidates if c is not s]:
            job.fill("x")
            with torch.cuda.stream(s):
                gate = ctx.held_back(s, ms)
                job.produce("y")
            with torch.cuda.stream(caller):
                k = job.call(caller)
            pending = not gate.query()
            torch.cuda.synchronize()
            job.used = 0
            got = job.got(k)
            seen.append(("stale" if got == job.want("x") else "serialised" if got == job.want("y") else "mixed") + ("" if pending else " (delay too short)"))
            if seen[-1] == "stale":
                break
        ctx.verdicts.append(seen[-1] if seen[-1] == "stale" else "/".join(sorted(set(seen))))
        if seen[-1] == "stale":
            ctx.streams.append(s)
    return job


@pytest.fixture(scope="module")
def ctx(oracle):
    import torch
    sbv.init(0)
    c = Ctx(torch, oracle)
    job = run_control(c, sc.MAIN, want=3)
    print("\n[stream order] delay: %d units of %s = %.2f ms; one warm cold call of sbv_p256_verify_batch_dev at n = %d: %.3f ms; control per candidate stream: %s (%d accepted)"
          % (c.delay.unit, "torch.cuda._sleep" if c.delay.sleep else "a 2^26-element op", c.delay.unit_ms, job.n, TIMES[(job.name, job.n, "cold")], ", ".join(c.verdicts), len(c.streams)))
    yield c
    torch.cuda.synchronize()
    print("\n[stream order] warm calls the delays were sized from (ms): " + ", ".join("%s/%d/%s %.3f" % (k[0][4:], k[1], k[2], v) for k, v in sorted(TIMES.items())))
    sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
    for s in SCHEME_ID.values():
        sbv.key_cache(True, 0, s)
    restore_hot_pools()


def test_control_the_delay_opens_a_window(ctx):
    """With the producer held behind the delay on one stream and the call on another, with no event between them, the library reads the
    stale generation: the delay really holds work back while the library's streams run.  At least one candidate stream must show it."""
    assert ctx.streams, "the delay holds nothing back on any candidate stream (%s): no schedule of this file could fail" % ", ".join(ctx.verdicts)


def _sizes(name):
    return (sc.MAIN, sc.ABOVE_THRESHOLD, sc.ONE_LANE) if ENTRIES[name].kind in ("generic", "keyed") else (sc.MAIN, sc.ONE_LANE)


def _entries(schedule, kinds=("generic", "keyed", "sign", "part")):
    return [name for name, e in ENTRIES.items() if schedule in e.schedules and e.kind in kinds]


def _with_modes(names, modes):
    """the key-table caches (cold / warm / hot) belong to the generic entries' grouped steps: the other entries run once, warm"""
    return [(name, mode) for mode in modes for name in names if ENTRIES[name].kind == "generic" or mode == "warm"]      # mode by mode: a change of the hot-key pools rebuilds them


@pytest.mark.parametrize("name,mode", _with_modes(_entries("late_producer"), ("cold", "warm")))
def test_late_producer_and_early_overwriter(ctx, name, mode):
    """Schedules 1 and 2 per entry and size.  The buffers hold X; on one stream: the delay, device-to-device copies of Y into every input
    (keyed entries: records and slots; the signer: digests), the call, the copy of the output into pinned memory — Y's output.  Then the
    same with, right behind the call, X written back over the inputs and a pattern into the caller's half of the output allocation: still
    Y's output, the pattern untouched.  A reader on a side stream that was not forked behind the caller's stream fails the first, one that
    was never joined back the second."""
    torch = ctx.torch
    ctx.set_mode(mode)
    s = ctx.stream()
    for n in _sizes(name):
        job = ctx.job(name, n)
        ms = ctx.delay_ms(job)
        for overwrite in (False, True):
            job.fill("x")
            with torch.cuda.stream(s):
                gate = ctx.held_back(s, ms)
                job.produce("y")
                k = job.call(s)
                if overwrite:
                    job.overwrite("x")
                    job.read(k)                                # once more, behind the overwriter: the library half as it is at the end
            ctx.finish([gate])
            job.check(k, "y", "%s, %s" % (mode, "early overwriter" if overwrite else "late producer"))
            if overwrite:
                assert (job.hosts[k][job.half:].numpy() == PATTERN).all(), (name, n, "the caller's half of the output allocation was written")
                for dst, src in zip(job.bufs, job.src["x"]):
                    assert torch.equal(dst, src), (name, n, "the overwritten inputs do not hold X")


@pytest.mark.parametrize("name,mode", _with_modes(_entries("back_to_back"), ("cold", "warm", "hot")))
def test_back_to_back_on_one_stream(ctx, name, mode):
    """Schedule 3: Y, then X, then Y through the same input buffers into three outputs, with no synchronisation between — cold, warm, and
    with the hot-key pool promoting behind the first call, so that the tail of one batch (table marks, promotion select, the comb builders on
    the library's second side stream) runs beside the grouping of the next."""
    torch = ctx.torch
    ctx.set_mode(mode)
    s = ctx.stream()
    job = ctx.job(name)
    ms = ctx.delay_ms(job)
    if mode == "hot":
        ctx.set_mode("hot")                                    # the timed calls filled the cache and promoted: from empty again
    job.fill("x")
    ks = []
    with torch.cuda.stream(s):
        gate = ctx.held_back(s, ms)
        for g in "yxy":
            job.produce(g)
            ks.append(job.call(s))
    ctx.finish([gate])
    for k, g in zip(ks, "yxy"):
        job.check(k, g, mode + ", back to back")
    if mode == "hot":
        promoted, cap, wide, min_hits = getattr(sbv, HOT_STATS[job.entry.scheme])()
        assert cap == 64 and min_hits == 64 and promoted > 0, (name, promoted, cap, wide, min_hits)
        if job.entry.scheme != "p256":                         # (a P-256 batch of this size takes the one cooperative launch, which has no wide pass)
            assert wide > 0, (name, promoted, cap, wide, min_hits)


@pytest.mark.parametrize("order", list(itertools.permutations(("p256", "ed25519", "k256"))), ids="-".join)
def test_across_streams_and_schemes(ctx, order):
    """Schedule 4: P-256 on one stream, Ed25519 on a second, secp256k1 on a third, called in every order, then the registered-key P-256
    entry on the second stream — each behind a late producer of its own, every hot-key pool on, and no event of the caller's between the
    streams: the library's own ordering (its busy event, the fork event, the event behind a batch's tail) is all there is.  Four bitmaps, and
    the grouping lists the last grouped batch left behind satisfy tests/group_model.py for THAT batch: they are no mixture."""
    torch = ctx.torch
    if ctx.mode != "hot":
        ctx.set_mode("hot")
    streams = dict(zip(("p256", "ed25519", "k256"), ctx.distinct(3)))
    jobs = {scheme: ctx.job(GENERIC_OF[scheme]) for scheme in order}
    keyed = ctx.job(KEYED_OF["p256"])
    ms = ctx.delay_ms(keyed, *jobs.values())
    last = jobs[order[-1]]
    # the last scheme's key-table cache as its batch will find it: only that scheme's batches change it
    torch.cuda.synchronize()
    getattr(sbv, HOST_CALL[order[-1]])(last.data.rows("x").tobytes(), last.n)
    before = sbv.debug_group_readout()
    assert before["scheme"] == SCHEME_ID[order[-1]]
    for j in list(jobs.values()) + [keyed]:
        j.fill("x")
    gates, ks = [], {}
    for scheme in order:
        s = streams[scheme]
        with torch.cuda.stream(s):
            gates.append(ctx.held_back(s, ms))
            jobs[scheme].produce("y")
            ks[scheme] = jobs[scheme].call(s)
    s = streams["ed25519"]
    with torch.cuda.stream(s):
        keyed.produce("y")
        kk = keyed.call(s)
    ctx.finish(gates)
    for scheme in order:
        jobs[scheme].check(ks[scheme], "y", "across schemes " + "-".join(order))
    keyed.check(kk, "y", "across schemes " + "-".join(order))
    ro = sbv.debug_group_readout()
    assert ro["scheme"] == SCHEME_ID[order[-1]] and ro["n"] == last.n and ro["serial"] == before["serial"] + 3, (ro["scheme"], ro["n"], ro["serial"], before["serial"])
    violations = gm.check(last.data.rows("y"), gm.KEYLOC[ro["scheme"]], ro, cache_before={"keys": before["cache_keys"], "count": before["cache_count"]},
                          bitmap=last.data.want("y"))
    assert violations == [], violations[:6]


@pytest.mark.parametrize("name", _entries("host_call"))
def test_host_pointer_call_against_a_queued_device_call(ctx, name):
    """Schedule 6: with the entry's call held behind the delay, the same host thread calls a blocking host-pointer entry — of the same
    scheme, then of another.  It returns X's bitmap (its own input), and the held call Y's: the busy event orders the two across entries
    and streams, also where the library lends its own stream to the held call's table kernels."""
    torch = ctx.torch
    ctx.set_mode("warm")
    s = ctx.stream()
    job = ctx.job(name)
    ms = ctx.delay_ms(job)
    schemes = list(SCHEME_ID)
    for other in (job.entry.scheme, schemes[(schemes.index(job.entry.scheme) + 1) % 3]):
        theirs = ctx.pair(other, sc.MAIN, tail=False)
        job.fill("x")
        with torch.cuda.stream(s):
            gate = ctx.held_back(s, ms)
            job.produce("y")
            k = job.call(s)
        got = getattr(sbv, HOST_CALL[other])(theirs.rows("x").tobytes(), theirs.n)
        ctx.finish([gate], host_waits=True)
        assert got == theirs.want("x"), (name, other, "the blocking entry's bitmap")
        job.check(k, "y", "held while %s's host-pointer entry ran" % other)


@pytest.mark.parametrize("name", _entries("setters"))
def test_setters_against_a_queued_call(ctx, name):
    """Schedule 7: with a call held behind the delay, a setter that frees or rewrites what the call reads — the scheme's key-table cache off
    and on, clear_keys, a hot-key pool of another size (generic entries); widen_keys and register_keys of 124 further keys
    (registered-key entries).  The held call's output and the next call's are both right.  (clear_keys keeps a registry's allocation, so
    by now these 148 slots fit: the registration that has to double the capacity runs on a fresh context, in the growth test below.)"""
    torch = ctx.torch
    ctx.set_mode("warm")
    s = ctx.stream()
    e = ENTRIES[name]
    sid = SCHEME_ID[e.scheme]
    if e.kind == "keyed":
        torch.cuda.synchronize()
        getattr(sbv, CLEAR[e.scheme])()
    job = ctx.job(name, tail=False)                            # keyed: registers the 24 signers
    ms = ctx.delay_ms(job)
    nxt = job
    if e.kind == "generic":
        def cache_off_on():
            sbv.key_cache(False, 0, sid)
            sbv.key_cache(True, 0, sid)
        setters = [("key_cache", cache_off_on), ("clear_keys", getattr(sbv, CLEAR[e.scheme])), ("hot_keys", lambda: getattr(sbv, HOT[e.scheme])(32, 64))]
    else:
        more = ctx.pair(e.scheme, sc.MAIN, tail=True)           # 124 further keys: 148 slots
        setters = [("widen_keys", lambda: getattr(sbv, WIDEN[e.scheme])(sorted(set(job.src["y"][1].cpu().numpy().view(np.uint32).tolist()))[:2])),
                   ("register_keys", lambda: getattr(sbv, REGISTER[e.scheme])(more.keys))]
    try:
        for what, setter in setters:
            job.fill("x")
            with torch.cuda.stream(s):
                gate = ctx.held_back(s, ms)
                job.produce("y")
                k = job.call(s)
            setter()
            if what == "register_keys":
                nxt = ctx.job(name, tail=True)                 # the registration is a lookup now
            nxt.fill("x")
            with torch.cuda.stream(s):
                k2 = nxt.call(s)
            ctx.finish([gate], host_waits=True)
            job.check(k, "y", "held while %s ran" % what)
            nxt.check(k2, "x", "the call after " + what)
    finally:
        torch.cuda.synchronize()
        if e.kind == "keyed":
            getattr(sbv, CLEAR[e.scheme])()
        else:
            restore_hot_pools()


@pytest.mark.parametrize("schemes", [("p256", "p256"), ("ed25519", "k256")], ids="-".join)
def test_two_host_threads_two_streams(ctx, schemes):
    """Schedule 8: two host threads, each with a stream and a pair of its own, each running the late-producer schedule eight times in a row
    without a synchronisation; the first one comes when both threads are done."""
    torch = ctx.torch
    ctx.set_mode("warm")
    jobs = [ctx.job(GENERIC_OF[schemes[0]], tail=True), ctx.job(GENERIC_OF[schemes[1]], tail=False)]
    ms = ctx.delay_ms(*jobs)
    rounds = 8
    for j in jobs:
        for _ in range(rounds):
            j.new_out()                                        # outputs 0 .. 7, allocated before anything is queued
        j.fill("x")
    gates, errors = [[], []], []

    def worker(j, s, mine):
        try:
            with torch.cuda.stream(s):
                for it in range(rounds):
                    j.produce("x")
                    mine.append(ctx.held_back(s, ms))
                    j.produce("y")
                    j.call(s, it)
        except BaseException as exc:                            # noqa: BLE001 — reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(j, s, mine)) for j, s, mine in zip(jobs, ctx.distinct(2), gates)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and all(len(mine) == rounds for mine in gates), errors
    ctx.finish([mine[-1] for mine in gates])                   # the last delay of EITHER thread is still pending
    for j in jobs:
        for it in range(rounds):
            j.check(it, "y", "thread round %d" % it)


def test_parts_on_one_stream_and_on_two(ctx):
    """Schedule 9: every part of a key-affine split of Y behind a late producer into one word array (a row per part: the entry zeroes
    what it is given), the rows OR-ed on the device — Y's bitmap.  The entry holds a host round trip, so the delay sits in front of the whole
    sequence.  Then four parts alternating between two streams that the caller joined with events of its own at both ends: the parts share
    the library's staging (member list, dense tuples, dense verdicts), which the library orders itself."""
    torch = ctx.torch
    ctx.set_mode("warm")
    name = "sbv_p256_verify_batch_dev_part"
    s1, s2 = ctx.distinct(2)
    job = ctx.job(name)
    ms = ctx.delay_ms(job)
    job.fill("x")
    with torch.cuda.stream(s1):
        gate = ctx.held_back(s1, ms)
        job.produce("y")
        k = job.call(s1)
    ctx.finish([gate], host_waits=True)
    job.check(k, "y", "%d parts on one stream" % job.parts)
    for rnd in range(3):
        job = Job(ctx, name, ctx.pair("p256", sc.MAIN), parts=4)
        job.fill("x")
        k = job.new_out()
        with torch.cuda.stream(s1):
            gate = ctx.held_back(s1, ms)
            job.produce("y")
            produced = torch.cuda.Event()
            produced.record(s1)
        s2.wait_event(produced)
        job.call_parts([s1, s2, s1, s2], k)
        done = torch.cuda.Event()
        done.record(s2)
        s1.wait_event(done)
        with torch.cuda.stream(s1):
            job.assemble(k)
            job.read(k)
        ctx.finish([gate], host_waits=True)
        job.check(k, "y", "4 parts on two streams, round %d" % rnd)


def _free_bytes(torch):
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("scheme", list(SCHEME_ID))
def test_growth_in_flight(ctx, scheme):
    """Schedule 5 and the growing setter of schedule 7, on a context that has seen nothing larger than 70 tuples and has an empty registry: the
    library is shut down and initialised again, and the control runs again at n = 70 (its streams are new ones; that call sizes the
    scratch and the grouping buffers for 1 024 tuples).
    First register_keys past a doubling: with the registered-key call of the 24 signers at n = 70 held behind the delay, 124 further keys
    are registered.  24 slots took a capacity of 32 (P-256: doubling from 16) or 64; 148 need 256, so the registry's arrays are allocated
    anew, copied and freed while the call is queued — the device's free memory drops by the 192 combs or more that come on top (33 x 128
    entries of 64 bytes = 264 KiB each at least, 49.5 MiB), less what the allocator's granularity of a few MiB per array rounds away; a
    registration that fits allocates nothing.  The bound between the two is half of it: 96 combs.  The held call and the next one, on the new keys, are right.
    Then the growth: the generic and the registered-key call at n = 70 queued behind the delay, then both at n = 8229 — the scratch, the
    grouping buffers and the staging of the slots grow (9 216 tuples) while the first calls have not run.  Then the four calls big first:
    nothing grows any more there, the small calls only run through the grown buffers.  (The last tests of the file: they leave a fresh
    context behind.)"""
    torch = ctx.torch
    names = (GENERIC_OF[scheme], KEYED_OF[scheme])
    ctx.set_mode("warm")
    ms = ctx.delay_ms(*[ctx.job(name, n) for name in names for n in (sc.ABOVE_THRESHOLD, sc.MAIN)])      # timed BEFORE the context is renewed
    torch.cuda.synchronize()
    sbv.shutdown()
    sbv.init(0)
    run_control(ctx, sc.ABOVE_THRESHOLD)
    ctx.set_mode("warm")
    s = ctx.stream()
    # (no warm call from here on: it would grow the buffers before the schedule does)
    small = [ctx.job(name, sc.ABOVE_THRESHOLD) for name in names]             # registers the 24 signers
    more = ctx.pair(scheme, sc.MAIN)
    held = small[1]
    held.fill("x")
    with torch.cuda.stream(s):
        gate = ctx.held_back(s, ms)
        held.produce("y")
        k = held.call(s)
    free_before = _free_bytes(torch)
    slots = getattr(sbv, REGISTER[scheme])(more.keys)
    grown = free_before - _free_bytes(torch)
    assert len(set(slots)) == len(more.keys) and max(slots) == len(small[1].data.keys) + len(more.keys) - 1, (min(slots), max(slots))
    assert grown >= 96 * 33 * 128 * 64, "registering %d keys on top of %d allocated %d bytes: the registry did not grow while the call was held" % (len(more.keys), len(held.data.keys), grown)
    big = [ctx.job(name, sc.MAIN) for name in names]                          # the registration is a lookup now
    big[1].fill("x")
    with torch.cuda.stream(s):
        k2 = big[1].call(s)
    ctx.finish([gate], host_waits=True)
    held.check(k, "y", "held while register_keys doubled the registry")
    big[1].check(k2, "x", "the call after register_keys")
    for first, then in ((small, big), (big, small)):
        for j in small + big:
            j.fill("x")
        ks = []
        with torch.cuda.stream(s):
            gate = ctx.held_back(s, ms)
            for j in first + then:
                j.produce("y")
                ks.append((j, j.call(s)))
        ctx.finish([gate], host_waits=True)
        for j, k in ks:
            j.check(k, "y", "growth in flight, %s first" % ("n = 70" if first is small else "n = 8229"))
