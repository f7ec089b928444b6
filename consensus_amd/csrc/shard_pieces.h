// shard_pieces.h — one device's share of a sharded call, cut into pieces and pipelined (sbv_api.hip: verify_shard, verify_shard_keyed,
// verify_shard_msgs).
//
// A share of m tuples goes up in pieces of `chunk` (plan_tuple_pieces / plan_keyed_pieces) through two staging sets: while the kernels of
// piece i run, piece i + 1 is on its way over PCIe on the copy stream.  run_pieces owns that protocol — the events, the order of the
// waits, the first failure, the drain, the timing sums — and its caller brings what differs between the three forms:
//
//     sbv::PiecePlan p;
//     int rc = sbv::plan_keyed_pieces(m, sbv::shard_granule(group), g_shard_piece_keyed, kMaxChunk, &p, &g_err);
//     ...                                                            // capacity, second staging set, copy stream
//     return sbv::run_pieces({c.stream, c.copy_stream, c.gsync.side_a}, c.busy, &c.busy_valid, m, p.chunk, "verify_shard_keyed", h2d_us, kern_us, &g_err,
//         [&](size_t, size_t off, size_t k, int w, hipStream_t up) { return hipMemcpyAsync(stage[w], h + off * 96, k * 96, hipMemcpyHostToDevice, up); },
//         [&](size_t, size_t off, size_t k, int w, hipStream_t s) { return enqueue_keyed(c, stage[w], ..., k, d_bits + off / 8, s, nullptr, w ? p.chunk : 0); });
//
// Host code only, and nothing of the library's context: g++ compiles this header against any definition of the seven runtime functions
// it calls (tests/emul/shard_pieces_test.cc brings a fake one that logs every call with its stream and fails the k-th).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <string>
#include <vector>

#include "../../include/sbv.h"

namespace sbv {

inline size_t gcd_sz(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }
// shards and pieces are whole bitmap words of whole proposals
inline size_t shard_granule(size_t group) {
    const size_t g8 = 8 * (group ? group : 1);
    return 512 / gcd_sz(512, g8) * g8;            // lcm(512, 8 * group)
}

// m tuples in `pieces` pieces of `chunk` (a multiple of the granule), the last one m - (pieces - 1) * chunk
struct PiecePlan { size_t chunk = 0, pieces = 0; };

// EQUAL pieces (round 6): 550 000 signatures in pieces of 2^18 used to end with a piece of 32 000 that paid the step's fixed chain
// (grouping, sort, classes: ~0.4 ms) for a tenth of the work, behind the last upload; a short last piece of a registered-key share
// would fall into the 8-lanes-per-signature latency kernel
inline void even_pieces(size_t m, size_t gran, PiecePlan* p) {
    const size_t even = ((m + p->pieces - 1) / p->pieces + gran - 1) / gran * gran;
    if (even && even <= p->chunk) { p->chunk = even; p->pieces = (m + even - 1) / even; }
}

// Tuple form (verify_shard).  Pieces of `piece` tuples when the key-table cache is on — the first piece builds the signers' combs, the
// others find them — and whole launches of up to max_chunk when it is off (every cold piece would rebuild every table).
inline int plan_tuple_pieces(size_t m, size_t gran, bool cache_on, size_t piece, size_t max_chunk, PiecePlan* p, std::string* err) {
    const size_t want = cache_on ? piece : max_chunk;
    p->chunk = (want < max_chunk ? want : max_chunk) / gran * gran;
    if (p->chunk == 0) p->chunk = max_chunk / gran * gran;
    if (p->chunk == 0) { *err = "group too large"; return SBV_EINVAL; }
    p->pieces = (m + p->chunk - 1) / p->chunk;
    if (p->pieces > 1) even_pieces(m, gran, p);
    return SBV_OK;
}

// Registered-key form (verify_shard_keyed, verify_shard_msgs).  No table is built per batch, so a piece only has to fill the device; two
// pieces are in flight, each in its half of the scratch planes: half of max_chunk at the most.
inline int plan_keyed_pieces(size_t m, size_t gran, size_t piece, size_t max_chunk, PiecePlan* p, std::string* err) {
    const size_t cap = max_chunk / 2;
    if (gran > cap) { *err = "group too large"; return SBV_EINVAL; }
    p->chunk = (piece < cap ? piece : cap) / gran * gran;
    if (p->chunk == 0) p->chunk = gran;
    p->pieces = (m + p->chunk - 1) / p->chunk;
    if (p->pieces) even_pieces(m, gran, p);
    return SBV_OK;
}

// The streams of a share.  With one piece everything runs on `main`.  With more, the uploads go through `copy`, and the kernels of piece i
// run on main (side == nullptr) or alternate between main and `side` (two pieces in flight: the front of piece i + 1 beside the bulk of
// piece i, each in its own half of the scratch).
struct PieceLanes { hipStream_t main, copy, side; };

// The m tuples of a share in pieces of `chunk`, P = ceil(m / chunk) of them; piece i = tuples [off, off + k) uses staging set w = i & 1.
//   upload(i, off, k, w, up)    enqueues the piece's host-to-device copies on `up`; returns the first hipError_t
//   step(i, off, k, w, stream)  enqueues the piece's kernels on `stream`; returns an SBV_* code, its text in *err
// In this order: 3 P events (per piece copy start, copy end, kernels end); if *busy_valid, every stream of this call waits for `busy`
// (kernels of an earlier call may still be using the scratch and group buffers); then per piece
//     i >= 2: `up` waits for the kernels of piece i - 2, which read the staging set this upload overwrites
//     copy start, upload, copy end on `up`
//     P > 1: the piece's kernel stream waits for copy end
//     step, kernels end on the piece's kernel stream.
// The first failure ends the enqueueing; a code from `step` is returned as it is, a HIP error as SBV_EDEVICE "<name>: <its text>".
// In every case every stream used is drained before an event is destroyed and before this returns: the staging sets and the caller's
// host buffers are free then, and *busy_valid is cleared.  On success *h2d_us grows by the copies' own durations, summed, and *kern_us
// by the time from the end of the first copy to the end of the last kernel (waits for later copies included).
template <class Upload, class Step>
int run_pieces(const PieceLanes& ln, hipEvent_t busy, bool* busy_valid, size_t m, size_t chunk, const char* name, double* h2d_us,
               double* kern_us, std::string* err, Upload&& upload, Step&& step) {
    const size_t pieces = (m + chunk - 1) / chunk;
    const bool two = pieces > 1, side = two && ln.side;
    const hipStream_t up = two ? ln.copy : ln.main;
    const hipStream_t ks[2] = {ln.main, side ? ln.side : ln.main};
    std::vector<hipEvent_t> ev(3 * pieces, nullptr);
    auto drop_events = [&] { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); };
    for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) { drop_events(); *err = "hipEventCreate failed"; return SBV_EDEVICE; }
    hipError_t he = hipSuccess;                    // the first HIP error
    auto ok = [&](hipError_t r) { if (he == hipSuccess) he = r; return he == hipSuccess; };
    int rc = SBV_OK;
    bool go = true;
    if (*busy_valid)
        go = ok(hipStreamWaitEvent(ln.main, busy, 0)) && (!side || ok(hipStreamWaitEvent(ks[1], busy, 0))) && (!two || ok(hipStreamWaitEvent(up, busy, 0)));
    for (size_t i = 0, off = 0; go && off < m; off += chunk, ++i) {
        const size_t k = m - off < chunk ? m - off : chunk;
        const int w = (int)(i & 1);
        hipEvent_t* e = &ev[3 * i];
        go = (i < 2 || ok(hipStreamWaitEvent(up, ev[3 * (i - 2) + 2], 0))) &&
             ok(hipEventRecord(e[0], up)) && ok(upload(i, off, k, w, up)) && ok(hipEventRecord(e[1], up)) &&
             (!two || ok(hipStreamWaitEvent(ks[w], e[1], 0))) &&
             (rc = step(i, off, k, w, ks[w])) == SBV_OK &&
             ok(hipEventRecord(e[2], ks[w]));
    }
    if (two) ok(hipStreamSynchronize(up));
    if (side) ok(hipStreamSynchronize(ks[1]));
    ok(hipStreamSynchronize(ln.main));
    if (rc == SBV_OK && he != hipSuccess) { *err = std::string(name) + ": " + hipGetErrorString(he); rc = SBV_EDEVICE; }
    if (rc == SBV_OK && pieces) {
        auto us_between = [](hipEvent_t a, hipEvent_t b) { float ms = 0.f; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? 1e3 * ms : 0.0; };
        if (h2d_us) for (size_t j = 0; j < pieces; ++j) *h2d_us += us_between(ev[3 * j], ev[3 * j + 1]);
        if (kern_us) *kern_us += us_between(ev[1], ev[3 * (pieces - 1) + 2]);
    }
    drop_events();
    *busy_valid = false;
    return rc;
}

}  // namespace sbv
