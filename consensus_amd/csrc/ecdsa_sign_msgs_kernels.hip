// ecdsa_sign_msgs_kernels.hip — gfx950 kernels in front of and behind the two ECDSA batch signers (ecdsa_sign_msgs.h; include/sbv.h:
// sbv_sha256_msgs, sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs and their _stream forms).
//
//   k_sha256_msgs          one lane per message, 256 per workgroup: the lane's slice of the packed messages -> 32 digest bytes.  Every
//                          lane checks ITS OWN offset pair as k_msg_frontend_tuples does; a refused pair hashes the empty message and
//                          marks the lane refused (mark[i] = 1, else 0) where the caller gives a mark array.
//   k_ecdsa_sig_finish<c>  one lane per signature: the signer's r | s and ok -> the 72-byte DER record (18 dword stores, zero behind
//                          its length) and the length byte; low-S for P-256 when asked (the secp256k1 signer applies its own flag),
//                          with bit 0 of recid flipped when s is negated here.  A lane whose signer said no, or that k_sha256_msgs
//                          marked refused, writes 72 zero bytes, length 0, ok 0 and recid 0.  The mark travels in the call's own
//                          length array: k_sha256_msgs writes it there, this kernel reads lens[i] before it stores the length.
//                          sbv_debug_ecdsa_der_op (test only) launches it on given r | s with every lane ok and no pair to check.
//
// The signing step between them is the launch of k_p256_sign / k_k256_sign as it was.  A translation unit of its own, so that no
// other kernel compiles differently.  No LDS, no atomics, no cross-lane traffic.  The compiler's figures are in DESIGN.md
// ("Raw-message ECDSA signing").
#include <hip/hip_runtime.h>

#include "ecdsa_sign_msgs.h"
#include "ecdsa_sign_msgs_kernels.h"

namespace sbv {

#ifndef SBV_SHA256_MSGS_WORDS
#define SBV_SHA256_MSGS_WORDS 1         // 0: the byte loader of sha256_msg (the measurement of DESIGN.md chose)
#endif

// mark may be null (sbv_sha256_msgs: nobody reads it)
__global__ __launch_bounds__(256) void k_sha256_msgs(const uint8_t* __restrict__ msgs, const u64* __restrict__ moff, size_t n, u64 mbytes,
                                                     u32* __restrict__ digests, uint8_t* __restrict__ mark) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u32 h[8];
    const bool taken = sha256_msgs_lane(msgs, moff[i], moff[i + 1], mbytes, SBV_SHA256_MSGS_WORDS != 0, h);
    if (mark) mark[i] = taken ? 0 : 1;
#pragma unroll
    for (int k = 0; k < 8; ++k) digests[i * 8 + k] = h[k];
}

// marked: lens[i] holds k_sha256_msgs' mark on entry (the debug entry has none).  recid may be null.  ok_in (null: every lane ok) and
// ok_out may be the same array.
template <int CURVE>
__global__ __launch_bounds__(256) void k_ecdsa_sig_finish(const u32* __restrict__ rs, const uint8_t* ok_in, u32 marked, size_t n, u32 low_s,
                                                          u32* __restrict__ records, uint8_t* __restrict__ lens, uint8_t* recid,
                                                          uint8_t* ok_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool good = ok_in ? ok_in[i] != 0 : true;
    if (marked) good = good && lens[i] == 0;
    u32 in[16], rec[SBV_ECDSA_DER_WORDS], len, rid = recid ? recid[i] : 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) in[k] = rs[i * 16 + k];
    ecdsa_sig_finish_lane(CURVE, in, good, low_s != 0, rec, len, rid);
#pragma unroll
    for (int k = 0; k < SBV_ECDSA_DER_WORDS; ++k) records[i * SBV_ECDSA_DER_WORDS + k] = rec[k];
    lens[i] = (uint8_t)len;
    if (recid) recid[i] = (uint8_t)rid;
    if (ok_out) ok_out[i] = good ? 1 : 0;
}

static unsigned grid256(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_sha256_msgs(const uint8_t* d_msgs, const u64* d_moff, size_t n, u64 mbytes, uint8_t* d_digests, uint8_t* d_mark,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sha256_msgs, dim3(grid256(n)), dim3(256), 0, stream, d_msgs, d_moff, n, mbytes, reinterpret_cast<u32*>(d_digests), d_mark);
    return hipGetLastError();
}

hipError_t launch_ecdsa_sig_finish(int curve, const uint8_t* d_rs, const uint8_t* d_ok_in, bool marked, size_t n, bool low_s,
                                   uint8_t* d_records, uint8_t* d_lens, uint8_t* d_recid, uint8_t* d_ok_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (curve == SBV_ECDSA_CURVE_P256)
        hipLaunchKernelGGL(k_ecdsa_sig_finish<SBV_ECDSA_CURVE_P256>, dim3(grid256(n)), dim3(256), 0, stream, reinterpret_cast<const u32*>(d_rs),
                           d_ok_in, marked ? 1u : 0u, n, low_s ? 1u : 0u, reinterpret_cast<u32*>(d_records), d_lens, d_recid, d_ok_out);
    else
        hipLaunchKernelGGL(k_ecdsa_sig_finish<SBV_ECDSA_CURVE_K256>, dim3(grid256(n)), dim3(256), 0, stream, reinterpret_cast<const u32*>(d_rs),
                           d_ok_in, marked ? 1u : 0u, n, low_s ? 1u : 0u, reinterpret_cast<u32*>(d_records), d_lens, d_recid, d_ok_out);
    return hipGetLastError();
}

}  // namespace sbv
