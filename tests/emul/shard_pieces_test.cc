// shard_pieces_test.cc — consensus_amd/csrc/shard_pieces.h as a program of its own (tests/test_shard_pieces_cpu.py builds it with
// AddressSanitizer and UBSan and wants exit status 0).
//
// Part 1, the piece plan: the sizes the GPU tests' docstrings quote, as literal cases, and a sweep for the properties every plan has.
//
// Part 2, the pipeline against a fake HIP runtime.  Streams and events are small integers; the seven runtime functions the header calls,
// hipMemcpyAsync for the uploads and a stand-in for a kernel launch are defined here and log every call with its stream and event; the
// fake fails the k-th call on request and gives a fixed duration per pair of event ids.  A scripted share runs in both lane
// configurations (kernels on one stream; kernels alternating between two) with 1 to 4 pieces, the busy flag set and clear: the clean run
// is checked against the ordering rules in the header's comment, then once per runtime call of the clean run with that call failing.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../../consensus_amd/csrc/shard_pieces.h"

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_what.c_str()); std::exit(1); } \
    } while (0)

namespace {

std::string g_what;                     // the scenario, for a failing CHECK

enum Kind { CREATE, DESTROY, RECORD, WAIT, COPY, LAUNCH, SYNC, ELAPSED, KINDS };
const char* const kKindText[KINDS] = {"fake: create", "fake: destroy", "fake: record", "fake: wait", "fake: copy", "fake: launch", "fake: synchronise", "fake: elapsed"};
const hipError_t kKindError[KINDS] = {hipErrorOutOfMemory, hipErrorInvalidHandle, hipErrorUnknown, hipErrorNotReady,
                                      hipErrorInvalidValue, hipErrorLaunchFailure, hipErrorIllegalAddress, hipErrorInvalidDevice};

struct Call { Kind kind; int stream; int event; int event2; };

struct Fake {
    std::vector<Call> log;              // every runtime call, in order
    long fail_at = -1;                  // index into log of the call that fails
    int events = 0;                     // ids handed out so far: 1, 2, ...
    bool step(Kind k, int stream, int event, int event2 = 0) {          // true: this call fails
        const long i = (long)log.size();
        log.push_back({k, stream, event, event2});
        return i == fail_at;
    }
};
Fake g_fake;

constexpr int kMain = 0x11, kCopy = 0x22, kSide = 0x33, kBusy = 1000;
hipStream_t stream_of(int id) { return reinterpret_cast<hipStream_t>(uintptr_t(id)); }
hipEvent_t event_of(int id) { return reinterpret_cast<hipEvent_t>(uintptr_t(id)); }
int id_of(const void* p) { return (int)reinterpret_cast<uintptr_t>(p); }
float fake_ms(int a, int b) { return 0.25f * (float)a + 0.5f * (float)b; }     // exact in float, so the sums are exact

}  // namespace

extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) {
    if (g_fake.step(CREATE, 0, g_fake.events + 1)) { *e = nullptr; return kKindError[CREATE]; }
    *e = event_of(++g_fake.events);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { return g_fake.step(DESTROY, 0, id_of(e)) ? kKindError[DESTROY] : hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return g_fake.step(RECORD, id_of(s), id_of(e)) ? kKindError[RECORD] : hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) {
    CHECK(flags == 0);
    return g_fake.step(WAIT, id_of(s), id_of(e)) ? kKindError[WAIT] : hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { return g_fake.step(SYNC, id_of(s), 0) ? kKindError[SYNC] : hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    if (g_fake.step(ELAPSED, 0, id_of(a), id_of(b))) return kKindError[ELAPSED];
    *ms = fake_ms(id_of(a), id_of(b));
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind kind, hipStream_t s) {
    CHECK(kind == hipMemcpyHostToDevice);
    return g_fake.step(COPY, id_of(s), 0) ? kKindError[COPY] : hipSuccess;
}
const char* hipGetErrorString(hipError_t e) {
    for (int k = 0; k < KINDS; ++k)
        if (kKindError[k] == e) return kKindText[k];
    return "fake: unknown";
}
}  // extern "C"

namespace {

constexpr size_t kMaxChunk = (size_t)1 << 21;           // as in sbv_api.hip

// ---- part 1: the plan -------------------------------------------------------------------------------------------------------

sbv::PiecePlan tuple_plan(size_t m, size_t gran, bool cache_on, size_t piece) {
    sbv::PiecePlan p;
    std::string err;
    CHECK(sbv::plan_tuple_pieces(m, gran, cache_on, piece, kMaxChunk, &p, &err) == SBV_OK && err.empty());
    return p;
}
sbv::PiecePlan keyed_plan(size_t m, size_t gran, size_t piece) {
    sbv::PiecePlan p;
    std::string err;
    CHECK(sbv::plan_keyed_pieces(m, gran, piece, kMaxChunk, &p, &err) == SBV_OK && err.empty());
    return p;
}
size_t last_piece(size_t m, const sbv::PiecePlan& p) { return m - (p.pieces - 1) * p.chunk; }
bool is(const sbv::PiecePlan& p, size_t chunk, size_t pieces) { return p.chunk == chunk && p.pieces == pieces; }

void plan_cases() {
    g_what = "plan: literal cases";
    CHECK(sbv::shard_granule(0) == 512 && sbv::shard_granule(1) == 512 && sbv::shard_granule(4) == 512 && sbv::shard_granule(64) == 512);
    CHECK(sbv::shard_granule(3) == 1536 && sbv::shard_granule(7) == 3584 && sbv::shard_granule(11) == 5632);
    // the tuple form
    CHECK(is(tuple_plan(550000, 512, true, (size_t)1 << 18), 183808, 3));               // configs[3] on one device: 3 equal pieces
    CHECK(is(tuple_plan(330000, 5632, true, 16384), 11264, 30));                        // test_sharded_entry_uploads_in_pieces_beside_the_kernels
    CHECK(is(tuple_plan(1541, 512, true, 512), 512, 4) && last_piece(1541, tuple_plan(1541, 512, true, 512)) == 5);
    CHECK(is(tuple_plan(3077, 1536, true, 512), kMaxChunk / 1536 * 1536, 1));           // the piece is below the granule: whole launches
    CHECK(is(tuple_plan(550000, 512, false, (size_t)1 << 18), kMaxChunk, 1));           // cache off: whole launches
    CHECK(is(tuple_plan(3 * kMaxChunk, 512, false, 512), kMaxChunk, 3));
    CHECK(is(tuple_plan(100003, 512, true, 16384), 14336, 7));                          // even(ceil(100003 / 7)) = 14 336 <= 16 384
    // the registered-key form
    CHECK(is(keyed_plan(14341, 512, 7168), 5120, 3));                                   // test_sharded_message_frontend_in_pieces
    CHECK(is(keyed_plan(1536, 512, 512), 512, 3));
    CHECK(is(keyed_plan(1541, 512, 512), 512, 4) && last_piece(1541, keyed_plan(1541, 512, 512)) == 5);
    CHECK(is(keyed_plan(3077, 1536, 512), 1536, 3) && last_piece(3077, keyed_plan(3077, 1536, 512)) == 5);
    CHECK(is(keyed_plan(550000, 512, (size_t)1 << 17), 110080, 5));
    CHECK(is(keyed_plan(4 * kMaxChunk, 512, kMaxChunk), kMaxChunk / 2, 8));             // never above half of a launch
    sbv::PiecePlan p;
    std::string err;
    CHECK(sbv::plan_keyed_pieces(1000, kMaxChunk / 2 + 512, 512, kMaxChunk, &p, &err) == SBV_EINVAL && err == "group too large");
    CHECK(sbv::plan_keyed_pieces(1000, kMaxChunk / 2, 512, kMaxChunk, &p, &err) == SBV_OK && is(p, kMaxChunk / 2, 1));
    err.clear();
    CHECK(sbv::plan_tuple_pieces(1000, kMaxChunk + 512, true, 512, kMaxChunk, &p, &err) == SBV_EINVAL && err == "group too large");
}

void plan_sweep() {
    const size_t groups[] = {0, 1, 3, 4, 7, 11, 64}, sizes[] = {512, 7168, (size_t)1 << 17, (size_t)1 << 18};
    for (size_t group : groups)
        for (size_t piece : sizes)
            for (size_t m = 1; m <= 40000; m += 37)                      // 37 is coprime to 512
                for (int form = 0; form < 3; ++form) {
                    g_what = "plan sweep: group " + std::to_string(group) + ", piece " + std::to_string(piece) + ", m " + std::to_string(m) + ", form " + std::to_string(form);
                    const size_t gran = sbv::shard_granule(group);
                    const sbv::PiecePlan p = form == 2 ? keyed_plan(m, gran, piece) : tuple_plan(m, gran, form == 1, piece);
                    CHECK(p.chunk > 0 && p.chunk % gran == 0);
                    CHECK(p.chunk <= (form == 2 ? kMaxChunk / 2 : kMaxChunk));
                    CHECK(p.pieces >= 1 && (p.pieces - 1) * p.chunk < m && m <= p.pieces * p.chunk);   // pieces - 1 of chunk and a non-empty last one cover m
                    if (form == 0) CHECK(p.pieces == 1);                                               // cache off and m below a launch
                    if (p.pieces > 1) CHECK(p.chunk <= (piece > gran ? piece : (form == 2 ? gran : kMaxChunk)));
                }
}

// ---- part 2: the pipeline ---------------------------------------------------------------------------------------------------

constexpr size_t kChunk = 512;
constexpr int kStepRefuses = SBV_ENOMEM;                 // what the scripted step makes of a failing launch: a code of its own

struct Outcome {
    int rc = 0;
    std::string err;
    bool busy_valid = false;
    double h2d_us = 0, kern_us = 0;
    std::vector<Call> log;
    std::vector<int> copy_piece, launch_piece;          // log index -> piece, for the copies and launches
};

// a share of `m` tuples: upload = two copies, step = one launch; step_refuses_at: the piece whose step returns SBV_EINVAL without a call
Outcome scripted_share(bool side, size_t m, bool busy, long fail_at, long step_refuses_at = -1) {
    g_fake = Fake();
    g_fake.fail_at = fail_at;
    Outcome o;
    o.busy_valid = busy;
    o.h2d_us = 1.0;                                       // the sums are added to what is there
    o.kern_us = 2.0;
    size_t seen = 0;
    const sbv::PieceLanes lanes = {stream_of(kMain), stream_of(kCopy), side ? stream_of(kSide) : nullptr};
    char host[4] = {0}, dev[4];
    o.rc = sbv::run_pieces(lanes, event_of(kBusy), &o.busy_valid, m, kChunk, "share", &o.h2d_us, &o.kern_us, &o.err,
        [&](size_t i, size_t off, size_t k, int w, hipStream_t up) {
            CHECK(i == seen && off == i * kChunk && k == (m - off < kChunk ? m - off : kChunk) && w == (int)(i & 1));
            const hipError_t e = hipMemcpyAsync(dev, host, 4, hipMemcpyHostToDevice, up);
            return e != hipSuccess ? e : hipMemcpyAsync(dev, host, 4, hipMemcpyHostToDevice, up);
        },
        [&](size_t i, size_t off, size_t k, int w, hipStream_t stream) {
            CHECK(i == seen && off == i * kChunk && k == (m - off < kChunk ? m - off : kChunk) && w == (int)(i & 1));
            ++seen;
            if ((long)i == step_refuses_at) { o.err = "step: refused"; return (int)SBV_EINVAL; }
            if (g_fake.step(LAUNCH, id_of(stream), (int)i)) { o.err = "step: launch"; return kStepRefuses; }
            return (int)SBV_OK;
        });
    o.log = g_fake.log;
    return o;
}

long find(const std::vector<Call>& log, Kind kind, int stream, int event, long from = 0) {
    for (long j = from; j < (long)log.size(); ++j)
        if (log[j].kind == kind && (stream < 0 || log[j].stream == stream) && (event < 0 || log[j].event == event)) return j;
    return -1;
}
long count(const std::vector<Call>& log, Kind kind, int stream = -1, int event = -1) {
    long n = 0;
    for (const Call& c : log) n += c.kind == kind && (stream < 0 || c.stream == stream) && (event < 0 || c.event == event);
    return n;
}
// events are numbered in the order of their creation: piece i has copy start 3 i + 1, copy end 3 i + 2, kernels end 3 i + 3
int cstart(size_t i) { return (int)(3 * i + 1); }
int cend(size_t i) { return (int)(3 * i + 2); }
int kend(size_t i) { return (int)(3 * i + 3); }

// what holds when the call is over, however it went: the streams that were handed anything are drained before the first event goes, and
// every event that was created goes exactly once
void check_release(const Outcome& o, size_t created) {
    const long first_destroy = find(o.log, DESTROY, -1, -1);
    std::set<int> used, synced;
    for (long j = 0; j < (long)o.log.size(); ++j) {
        const Call& c = o.log[j];
        if (c.kind == RECORD || c.kind == WAIT || c.kind == COPY || c.kind == LAUNCH) { used.insert(c.stream); CHECK(first_destroy < 0 || j < first_destroy); }
        if (c.kind == SYNC) { synced.insert(c.stream); CHECK(first_destroy < 0 || j < first_destroy); }
    }
    for (int s : used) CHECK(synced.count(s) == 1);
    for (size_t e = 1; e <= created; ++e) CHECK(count(o.log, DESTROY, -1, (int)e) == 1);
    CHECK(count(o.log, DESTROY) == (long)created);
}

void check_clean(const Outcome& o, bool side, size_t pieces, bool busy) {
    const bool two = pieces > 1;
    const int up = two ? kCopy : kMain;
    auto ks = [&](size_t i) { return two && side && (i & 1) ? kSide : kMain; };
    CHECK(o.rc == SBV_OK && o.err.empty() && !o.busy_valid);
    CHECK(count(o.log, CREATE) == (long)(3 * pieces));
    for (long j = 0; j < (long)(3 * pieces); ++j) CHECK(o.log[j].kind == CREATE);          // all of them before anything is enqueued
    // the busy waits: exactly the streams this call uses, before anything else is enqueued
    std::set<int> streams = {kMain};
    if (two) streams.insert(kCopy);
    if (two && side) streams.insert(kSide);
    CHECK(count(o.log, WAIT, -1, kBusy) == (busy ? (long)streams.size() : 0));
    if (busy) {
        long j = (long)(3 * pieces);
        std::set<int> waited;
        for (; j < (long)o.log.size() && o.log[j].kind == WAIT && o.log[j].event == kBusy; ++j) waited.insert(o.log[j].stream);
        CHECK(waited == streams);
    }
    std::set<int> used;
    for (const Call& c : o.log)
        if (c.kind == RECORD || c.kind == WAIT || c.kind == COPY || c.kind == LAUNCH) used.insert(c.stream);
    CHECK(used == streams);
    long prev_launch = -1;
    for (size_t i = 0; i < pieces; ++i) {
        const long r0 = find(o.log, RECORD, -1, cstart(i)), r1 = find(o.log, RECORD, -1, cend(i)), r2 = find(o.log, RECORD, -1, kend(i));
        const long launch = find(o.log, LAUNCH, -1, (int)i);
        CHECK(r0 >= 0 && r1 > r0 && launch > r1 && r2 > launch && launch > prev_launch);
        prev_launch = launch;
        CHECK(o.log[r0].stream == up && o.log[r1].stream == up);
        CHECK(count(o.log, RECORD, -1, cstart(i)) == 1 && count(o.log, RECORD, -1, cend(i)) == 1 && count(o.log, RECORD, -1, kend(i)) == 1);
        // the piece's two copies: on `up`, between copy start and copy end
        long copies = 0;
        for (long j = r0 + 1; j < r1; ++j) { CHECK(o.log[j].kind == COPY && o.log[j].stream == up); ++copies; }
        CHECK(copies == 2);
        // its kernels and their end on its kernel stream: main throughout, or alternating with the side stream
        CHECK(o.log[launch].stream == ks(i) && o.log[r2].stream == ks(i));
        // a staging set is overwritten only behind the kernels that read it: `up` waits for kernels end of piece i - 2, recorded by then
        const long reuse = i >= 2 ? find(o.log, WAIT, up, kend(i - 2)) : -1;
        if (i >= 2) CHECK(reuse > find(o.log, RECORD, -1, kend(i - 2)) && reuse < r0);
        // the kernels start behind the piece's copies: their stream waits for copy end, recorded by then; one piece needs no wait at all
        const long ready = find(o.log, WAIT, ks(i), cend(i));
        if (two) CHECK(ready > r1 && ready < launch);
        else CHECK(ready < 0);
    }
    CHECK(count(o.log, COPY) == (long)(2 * pieces) && count(o.log, LAUNCH) == (long)pieces);
    CHECK(count(o.log, WAIT) == (busy ? (long)streams.size() : 0) + (two ? (long)pieces : 0) + (pieces > 2 ? (long)(pieces - 2) : 0));
    // the drain: each stream once, behind everything enqueued
    long last_work = -1;
    for (long j = 0; j < (long)o.log.size(); ++j)
        if (o.log[j].kind == RECORD || o.log[j].kind == WAIT || o.log[j].kind == COPY || o.log[j].kind == LAUNCH) last_work = j;
    for (int s : streams) CHECK(count(o.log, SYNC, s) == 1 && find(o.log, SYNC, s, -1) > last_work);
    CHECK(count(o.log, SYNC) == (long)streams.size());
    check_release(o, 3 * pieces);
    // the timing sums, over the right pairs of events
    double h2d = 1.0;
    for (size_t i = 0; i < pieces; ++i) h2d += 1e3 * fake_ms(cstart(i), cend(i));
    CHECK(o.h2d_us == h2d);
    CHECK(o.kern_us == 2.0 + 1e3 * fake_ms(cend(0), kend(pieces - 1)));
    CHECK(count(o.log, ELAPSED) == (long)pieces + 1);
}

void run(bool side, size_t pieces, bool busy) {
    const size_t m = (pieces - 1) * kChunk + 5;          // a ragged last piece
    const std::string what = std::string(side ? "two kernel streams, " : "one kernel stream, ") + std::to_string(pieces) + " pieces, busy " + (busy ? "set" : "clear");
    g_what = what + ", clean";
    const Outcome clean = scripted_share(side, m, busy, -1);
    check_clean(clean, side, pieces, busy);
    const std::vector<Call>& script = clean.log;

    for (size_t k = 0; k < script.size(); ++k) {
        g_what = what + ", failing call " + std::to_string(k) + " (" + kKindText[script[k].kind] + ")";
        const Outcome o = scripted_share(side, m, busy, (long)k);
        CHECK(o.log.size() > k);
        for (size_t j = 0; j <= k; ++j)                    // the same call failed as was meant to
            CHECK(o.log[j].kind == script[j].kind && o.log[j].stream == script[j].stream && o.log[j].event == script[j].event);
        const Kind kind = script[k].kind;
        if (kind == CREATE) {
            // nothing was enqueued: the events made so far go, and the busy flag stays as it was
            CHECK(o.rc == SBV_EDEVICE && o.err == "hipEventCreate failed" && o.busy_valid == busy);
            CHECK(o.log.size() == 2 * k + 1 && o.h2d_us == 1.0 && o.kern_us == 2.0);
            check_release(o, k);
            continue;
        }
        CHECK(!o.busy_valid);
        check_release(o, 3 * pieces);
        if (kind == ELAPSED || kind == DESTROY) {
            // the share was through and drained when this failed: a duration that cannot be read counts as none
            CHECK(o.rc == SBV_OK && o.err.empty() && o.log.size() == script.size());
            if (kind == DESTROY) CHECK(o.h2d_us == clean.h2d_us && o.kern_us == clean.kern_us);
            else CHECK(o.h2d_us + o.kern_us == clean.h2d_us + clean.kern_us - 1e3 * fake_ms(script[k].event, script[k].event2));
            continue;
        }
        if (kind == LAUNCH) CHECK(o.rc == kStepRefuses && o.err == "step: launch");            // the step's own code and text, unchanged
        else CHECK(o.rc == SBV_EDEVICE && o.err == std::string("share: ") + kKindText[kind]);
        CHECK(o.h2d_us == 1.0 && o.kern_us == 2.0 && count(o.log, ELAPSED) == 0);
        // after the failure: draining and releasing only.  A failing synchronise of the drain does not stop the others.
        for (size_t j = k + 1; j < o.log.size(); ++j) CHECK(o.log[j].kind == SYNC || o.log[j].kind == DESTROY);
        CHECK(count(o.log, SYNC) == count(script, SYNC));
        for (const Call& c : script)
            if (c.kind == SYNC) CHECK(count(o.log, SYNC, c.stream) == 1);
    }

    // a step that refuses its piece without any runtime call failing
    for (size_t at = 0; at < pieces; ++at) {
        g_what = what + ", step refuses piece " + std::to_string(at);
        const Outcome o = scripted_share(side, m, busy, -1, (long)at);
        CHECK(o.rc == SBV_EINVAL && o.err == "step: refused" && !o.busy_valid && o.h2d_us == 1.0 && o.kern_us == 2.0);
        CHECK(count(o.log, LAUNCH) == (long)at && count(o.log, COPY) == (long)(2 * (at + 1)) && count(o.log, RECORD, -1, kend(at)) == 0);
        CHECK(count(o.log, SYNC) == count(script, SYNC));
        check_release(o, 3 * pieces);
    }
}

}  // namespace

int main() {
    plan_cases();
    plan_sweep();
    for (int side = 0; side < 2; ++side)
        for (size_t pieces = 1; pieces <= 4; ++pieces)
            for (int busy = 0; busy < 2; ++busy) run(side != 0, pieces, busy != 0);
    std::puts("shard_pieces: ok");
    return 0;
}
