// call_buffers_test.cc — consensus_amd/csrc/call_buffers.h against a fake HIP runtime, as a program of its own (tests/test_call_buffers_cpu.py
// builds it with AddressSanitizer and UBSan and wants exit status 0).
//
// The six runtime functions the helper calls are defined here over malloc / memcpy.  The fake counts every call, fails the k-th one on
// request, and keeps a "work pending" flag that any asynchronous operation sets and a synchronise clears.  At hipFree it notes whether work
// was pending and whether the block was all zero.  One scripted call shaped like the signers (a secret upload, a plain upload, an optional
// upload, two allocations, a launch, two downloads of which one goes nowhere, finish) runs clean and then once per runtime call of the
// clean run with that call failing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../consensus_amd/csrc/call_buffers.h"

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_what.c_str()); std::exit(1); } \
    } while (0)

namespace {

enum Kind { MALLOC, FREE, H2D, D2H, MEMSET, SYNC, LAUNCH };
const char* const kKindText[] = {"fake: out of memory", "fake: free", "fake: upload", "fake: download", "fake: memset", "fake: synchronise", "fake: launch"};
const hipError_t kKindError[] = {hipErrorOutOfMemory,  hipErrorInvalidDevicePointer, hipErrorInvalidValue, hipErrorInvalidMemcpyDirection,
                                 hipErrorInvalidDevice, hipErrorIllegalAddress,       hipErrorLaunchFailure};

struct Block { void* p; size_t bytes; int frees; bool zero_at_free; bool pending_at_free; };

struct Fake {
    std::vector<Kind> log;              // every runtime call, in order
    long fail_at = -1;                  // index into log of the call that fails
    bool fail_all_after = false;        // ... and every later one too
    bool pending = false;
    int syncs = 0;
    std::vector<Block> blocks;
    // true: this call fails
    bool step(Kind k) {
        const long i = (long)log.size();
        log.push_back(k);
        return i == fail_at || (fail_all_after && fail_at >= 0 && i > fail_at);
    }
};
Fake g_fake;
std::string g_what;                     // the scenario, for a failing CHECK
const hipStream_t kStream = reinterpret_cast<hipStream_t>(uintptr_t(0x51));

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fake.step(MALLOC)) { *p = nullptr; return kKindError[MALLOC]; }
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xA5, bytes);
    g_fake.blocks.push_back({*p, bytes, 0, false, false});
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    const bool fails = g_fake.step(FREE);
    for (Block& b : g_fake.blocks)
        if (b.p == p) {
            if (++b.frees == 1) {
                b.pending_at_free = g_fake.pending;
                b.zero_at_free = true;
                for (size_t i = 0; i < b.bytes; ++i) b.zero_at_free &= static_cast<const unsigned char*>(p)[i] == 0;
                std::free(p);
            }
            return fails ? kKindError[FREE] : hipSuccess;
        }
    CHECK(!"hipFree of a pointer that hipMalloc never returned");
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    CHECK(stream == kStream && dst && src && (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToHost));
    const Kind k = kind == hipMemcpyHostToDevice ? H2D : D2H;
    if (g_fake.step(k)) return kKindError[k];
    g_fake.pending = true;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream) {
    CHECK(stream == kStream && dst);
    if (g_fake.step(MEMSET)) return kKindError[MEMSET];
    g_fake.pending = true;
    std::memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    CHECK(stream == kStream);
    ++g_fake.syncs;
    if (g_fake.step(SYNC)) return kKindError[SYNC];
    g_fake.pending = false;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) {
    for (int k = MALLOC; k <= LAUNCH; ++k)
        if (kKindError[k] == e) return kKindText[k];
    return "fake: unknown";
}
}  // extern "C"

namespace {

constexpr size_t N = 37;

// the kernel's stand-in: sig[i] = key[i] ^ msg[i] ^ idx[i] (idx absent: 0), skipped[i] = i.  Counts as a runtime call.
hipError_t fake_launch(const uint8_t* key, const uint8_t* msg, const uint32_t* idx, uint8_t* sig, uint8_t* skipped) {
    CHECK(key && msg && sig && skipped);                    // a launch after a failure would come with null pointers
    if (g_fake.step(LAUNCH)) return kKindError[LAUNCH];
    g_fake.pending = true;
    for (size_t i = 0; i < N; ++i) { sig[i] = uint8_t(key[i] ^ msg[i] ^ (idx ? idx[i] : 0)); skipped[i] = uint8_t(i); }
    return hipSuccess;
}

struct Outcome {
    int rc = 0;
    std::string err;
    uint8_t sig[N];
    std::vector<const void*> secrets;   // device pointers of the buffers marked secret
    Fake fake;                          // the runtime's record of the call
};

Outcome scripted_call(bool secret, bool with_idx, long fail_at, bool fail_all_after = false) {
    g_what = std::string(secret ? "secret" : "plain") + (with_idx ? ", idx" : ", no idx") + ", failing call " + std::to_string(fail_at) +
             (fail_all_after ? " and all after" : "");
    g_fake = Fake();
    g_fake.fail_at = fail_at;
    g_fake.fail_all_after = fail_all_after;
    uint8_t key[N], msg[N];
    uint32_t idx[N];
    for (size_t i = 0; i < N; ++i) { key[i] = uint8_t(3 * i + 1); msg[i] = uint8_t(7 * i + 2); idx[i] = uint32_t(i % 5); }
    Outcome o;
    std::memset(o.sig, 0xEE, N);
    {
        sbv::CallBuffers cb(kStream, &o.err);
        const uint8_t* d_key = cb.upload(key, N, secret);
        const uint8_t* d_msg = cb.upload(msg, N);
        const uint32_t* d_idx = cb.upload(with_idx ? idx : nullptr, N * sizeof(uint32_t));
        uint8_t* d_sig = cb.alloc(N);
        uint8_t* d_skipped = cb.alloc(N);
        CHECK(with_idx || !d_idx);
        if (cb.good()) cb.launch(fake_launch(d_key, d_msg, d_idx, d_sig, d_skipped));
        cb.download(o.sig, d_sig, N);
        cb.download(nullptr, d_skipped, N);
        o.rc = cb.finish();
        CHECK(cb.good() == (o.rc == SBV_OK));
    }
    for (size_t i = 0; i < N; ++i) CHECK(key[i] == uint8_t(3 * i + 1));        // zeroing is for the device copy alone
    o.fake = g_fake;
    if (secret && !o.fake.blocks.empty()) o.secrets.push_back(o.fake.blocks[0].p);      // the key's buffer is the first one allocated
    return o;
}

bool sig_right(const Outcome& o, bool with_idx) {
    for (size_t i = 0; i < N; ++i)
        if (o.sig[i] != uint8_t(uint8_t(3 * i + 1) ^ uint8_t(7 * i + 2) ^ (with_idx ? i % 5 : 0))) return false;
    return true;
}

// what must hold when the buffers go; `except` names a teardown call that itself failed, whose effect cannot be asked for
void check_release(const Outcome& o, int except = -1) {
    for (const Block& b : o.fake.blocks) {
        CHECK(b.frees == 1);
        if (except != SYNC) CHECK(!b.pending_at_free);
        bool is_secret = false;
        for (const void* s : o.secrets) is_secret |= s == b.p;
        if (is_secret && except != MEMSET) CHECK(b.zero_at_free);
    }
}

void run(bool secret, bool with_idx) {
    const Outcome clean = scripted_call(secret, with_idx, -1);
    CHECK(clean.rc == SBV_OK && clean.err.empty() && sig_right(clean, with_idx));
    CHECK(clean.fake.blocks.size() == (with_idx ? 5u : 4u));
    CHECK(clean.secrets.size() == (secret ? 1u : 0u));
    CHECK(clean.fake.syncs == (secret ? 2 : 1));
    check_release(clean);
    const std::vector<Kind>& script = clean.fake.log;
    size_t teardown = 0;                // the first call after finish()'s synchronise: memsets, a synchronise, frees
    while (script[teardown] != SYNC) ++teardown;
    ++teardown;
    int n_d2h = 0;
    for (Kind k : script) n_d2h += k == D2H;
    CHECK(n_d2h == 1);                  // the download to a null host pointer is not issued

    for (size_t k = 0; k < script.size(); ++k) {
        const Outcome o = scripted_call(secret, with_idx, (long)k);
        CHECK(o.fake.log.size() > k && o.fake.log[k] == script[k]);            // the same call failed as was meant to
        if (k < teardown) {
            CHECK(o.rc == (script[k] == MALLOC ? SBV_ENOMEM : SBV_EDEVICE));
            CHECK(o.err == kKindText[script[k]]);
            for (size_t j = k + 1; j < o.fake.log.size(); ++j) {               // after the failure: waiting, zeroing and freeing only
                const Kind later = o.fake.log[j];
                CHECK(later == SYNC || later == MEMSET || later == FREE);
            }
            check_release(o);
        } else {
            // the call was over and its status returned when this failed; the teardown goes on and reports nothing
            CHECK(o.rc == SBV_OK && o.err.empty() && sig_right(o, with_idx));
            CHECK(o.fake.log.size() == script.size());
            check_release(o, script[k]);
        }
        // everything failing from call k on: the first failure's code and text stay, and every buffer is still freed once
        const Outcome all = scripted_call(secret, with_idx, (long)k, true);
        if (k < teardown) {
            CHECK(all.rc == (script[k] == MALLOC ? SBV_ENOMEM : SBV_EDEVICE));
            CHECK(all.err == kKindText[script[k]]);
        } else {
            CHECK(all.rc == SBV_OK && all.err.empty());
        }
        for (const Block& b : all.fake.blocks) CHECK(b.frees == 1);
    }
}

// upload of no bytes from a present array: a buffer, no copy; copy_in of no bytes: nothing
void zero_bytes() {
    g_what = "zero bytes";
    g_fake = Fake();
    std::string err;
    uint8_t host[1] = {9};
    {
        sbv::CallBuffers cb(kStream, &err);
        CHECK(cb.upload(host, 0) != nullptr);
        uint8_t* d = cb.alloc(16);
        CHECK(cb.copy_in(d, nullptr, 0));
        CHECK(cb.finish() == SBV_OK);
    }
    const std::vector<Kind> want = {MALLOC, MALLOC, SYNC, FREE, FREE};
    CHECK(g_fake.log == want && err.empty());
}

}  // namespace

int main() {
    for (int secret = 0; secret < 2; ++secret)
        for (int with_idx = 0; with_idx < 2; ++with_idx) run(secret != 0, with_idx != 0);
    zero_bytes();
    std::puts("call_buffers: ok");
    return 0;
}
