// k256_recover_kernels.hip — gfx950 kernels of the secp256k1 batch public-key recovery (k256_recover.h; include/sbv.h:
// sbv_secp256k1_recover and its _stream form).
//
//   k_k256_recover      one signature per lane per pass: r | s, recid, digest -> Qx | Qy and ok
//   k_k256_recover_op   test only (sbv_debug_secp256k1_recover_op): one case of a unit operation per lane
//
// A lane needs a strip of SBV_K256_QTAB_WORDS dwords in HBM for the table 1..8 R' (as k_k256_verify does for 1..8 Q), so the grid is
// capped at SBV_K256_RECOVER_LANES lanes — one full residency of the device, DESIGN.md "secp256k1 public-key recovery" — and lane L
// handles items L, L + LANES, L + 2 LANES, ... on its own strip: the workspace is min(n, LANES) strips whatever n is.  No LDS, no
// atomics, no cross-lane traffic.  A strip is a multiple of 16 bytes from a 16-byte aligned base, so the table's 16-byte loads are
// aligned as k_k256_verify's are.  The walk is the one-lane verifier's (k256_mul_u2Q, k256_add_u1G), so the launch bounds are its.
#include <hip/hip_runtime.h>

#include "k256_recover.h"
#include "k256_recover_kernels.h"
#include "../../include/sbv.h"

namespace sbv {

static_assert(SBV_K256_QTAB_WORDS % 4 == 0, "strips keep the 16-byte alignment of the workspace");
static_assert(SBV_K256_RECOVER_LANES % SBV_VERIFY_BLOCK == 0, "whole workgroups");

// sigs / digests / pubs are byte strings as on the wire (big-endian 32-byte integers)
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_recover(const u32* __restrict__ sigs, const uint8_t* __restrict__ recid,
                                                                    const u32* __restrict__ digests, size_t n, u32 flags,
                                                                    const kapt* __restrict__ gtab, u32* __restrict__ work,
                                                                    u32* __restrict__ pubs, uint8_t* __restrict__ ok) {
    const size_t L = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;          // < SBV_K256_RECOVER_LANES by the launch
    if (L >= n) return;
    u32* strip = work + L * (size_t)SBV_K256_QTAB_WORDS;
    SBV_NOUNROLL
    for (size_t i = L; i < n; i += SBV_K256_RECOVER_LANES) {
        u32 rs[16], h[8], q[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) rs[k] = __builtin_bswap32(sigs[i * 16 + k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = __builtin_bswap32(digests[i * 8 + k]);
        const bool good = k256_recover_lane(rs, recid[i], h, flags, strip, gtab, q);
#pragma unroll
        for (int k = 0; k < 16; ++k) pubs[i * 16 + k] = __builtin_bswap32(q[k]);
        ok[i] = good ? 1 : 0;
    }
}

// in: n x 192 bytes, out: n x 128 bytes (the records of include/sbv.h); work: n strips
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_recover_op(int op, const u32* __restrict__ in, u32* __restrict__ out, size_t n,
                                                                       const kapt* __restrict__ gtab, u32* __restrict__ work) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_IN_WORDS; ++k) a[k] = __builtin_bswap32(in[i * SBV_K256_SIGN_OP_IN_WORDS + k]);
    k256_recover_op_lane(op, a, work + i * (size_t)SBV_K256_QTAB_WORDS, gtab, r);
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_OUT_WORDS; ++k) out[i * SBV_K256_SIGN_OP_OUT_WORDS + k] = __builtin_bswap32(r[k]);
}

size_t k256_recover_strip_bytes() { return (size_t)SBV_K256_QTAB_WORDS * sizeof(u32); }

hipError_t launch_k256_recover(const uint8_t* d_sigs, const uint8_t* d_recid, const uint8_t* d_digests, size_t n, u32 flags, const kapt* d_gtab,
                               u32* d_work, uint8_t* d_pubs, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lanes = n < (size_t)SBV_K256_RECOVER_LANES ? n : (size_t)SBV_K256_RECOVER_LANES;
    hipLaunchKernelGGL(k_k256_recover, dim3((unsigned)((lanes + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK)), dim3(SBV_VERIFY_BLOCK), 0, stream,
                       reinterpret_cast<const u32*>(d_sigs), d_recid, reinterpret_cast<const u32*>(d_digests), n, flags, d_gtab, d_work,
                       reinterpret_cast<u32*>(d_pubs), d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_recover_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const kapt* d_gtab, u32* d_work, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_recover_op, dim3((unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK)), dim3(SBV_VERIFY_BLOCK), 0, stream, op,
                       reinterpret_cast<const u32*>(d_in), reinterpret_cast<u32*>(d_out), n, d_gtab, d_work);
    return hipGetLastError();
}

}  // namespace sbv
