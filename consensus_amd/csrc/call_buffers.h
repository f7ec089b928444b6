// call_buffers.h — the device buffers and the status of one host-pointer call (sbv_api.hip: the sign, recover and Schnorr entries).
//
// Such a call allocates buffers of its own size, uploads, launches once, downloads, waits, and releases everything before it returns.
// CallBuffers owns the buffers and carries the status, so that the call is written straight down:
//
//     sbv::CallBuffers cb(stream, &g_err);
//     const uint8_t* d_keys = cb.upload(keys, n_keys * 32, /*secret=*/true);
//     const u32* d_idx = cb.upload(key_index, n * 4);            // key_index == nullptr: nothing allocated, d_idx == nullptr
//     uint8_t* d_sig = cb.alloc(n * 64);
//     if (cb.good()) cb.launch(sbv::launch_...(d_keys, d_idx, ..., d_sig, stream));
//     cb.download(sigs, d_sig, n * 64);
//     return cb.finish();
//
// The first failure wins: its code (SBV_ENOMEM from an allocation, SBV_EDEVICE from anything else) and its hipGetErrorString text are
// kept, and every later operation does nothing and returns null / false.  The destructor waits for whatever the call enqueued, unless
// finish() already did; zeroes every buffer marked secret and waits for that; then frees.  So nothing of the call is in flight when
// its buffers go, and no private key outlives the call in released device memory, whichever way the call ends.
//
// Host code only, and nothing of the library's context: g++ compiles this header against any definition of the six runtime functions
// it calls (tests/emul/call_buffers_test.cc brings a fake one).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbv.h"

namespace sbv {

class CallBuffers {
public:
    CallBuffers(hipStream_t stream, std::string* err) : stream_(stream), err_(err) {}
    CallBuffers(const CallBuffers&) = delete;
    CallBuffers& operator=(const CallBuffers&) = delete;

    ~CallBuffers() {
        if (pending_) (void)hipStreamSynchronize(stream_);
        bool zeroed = false;
        for (const Buf& b : bufs_)
            if (b.secret) { (void)hipMemsetAsync(b.p, 0, b.bytes, stream_); zeroed = true; }
        if (zeroed) (void)hipStreamSynchronize(stream_);
        for (const Buf& b : bufs_) (void)hipFree(b.p);
    }

    bool good() const { return rc_ == SBV_OK; }

    template <class T = uint8_t>
    T* alloc(size_t bytes, bool secret = false) {
        void* p = nullptr;
        if (!good() || !check(SBV_ENOMEM, hipMalloc(&p, bytes))) return nullptr;
        bufs_.push_back({p, bytes, secret});
        return static_cast<T*>(p);
    }

    // host -> device into a buffer of this call's; bytes == 0 copies nothing
    bool copy_in(void* dev, const void* host, size_t bytes) {
        if (!good()) return false;
        if (bytes == 0) return true;
        pending_ = true;
        return check(SBV_EDEVICE, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream_));
    }

    // alloc + copy_in; an absent (null) host array gets no buffer
    template <class T>
    T* upload(const T* host, size_t bytes, bool secret = false) {
        if (!host) return nullptr;
        T* d = alloc<T>(bytes, secret);
        return copy_in(d, host, bytes) ? d : nullptr;
    }

    // the result of the sbv::launch_* call: `if (cb.good()) cb.launch(sbv::launch_...(...));`, so that no kernel follows a failure
    bool launch(hipError_t e) {
        if (!good()) return false;
        pending_ = true;
        return check(SBV_EDEVICE, e);
    }

    // device -> host; an absent (null) host array is skipped
    bool download(void* host, const void* dev, size_t bytes) {
        if (!good()) return false;
        if (!host) return true;
        pending_ = true;
        return check(SBV_EDEVICE, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream_));
    }

    // waits for the call's work and returns its status
    int finish() {
        if (good() && check(SBV_EDEVICE, hipStreamSynchronize(stream_))) pending_ = false;
        return rc_;
    }

private:
    struct Buf { void* p; size_t bytes; bool secret; };

    bool check(int code, hipError_t e) {
        if (e == hipSuccess) return true;
        rc_ = code;                     // only reached while good(): the first failure is the one kept
        *err_ = hipGetErrorString(e);
        return false;
    }

    hipStream_t stream_;
    std::string* err_;
    std::vector<Buf> bufs_;
    int rc_ = SBV_OK;
    bool pending_ = false;              // something was enqueued that no successful synchronise has covered yet
};

}  // namespace sbv
