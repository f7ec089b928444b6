// k256_schnorr_kernels.hip — gfx950 kernels of the BIP-340 Schnorr entries over secp256k1 (k256_schnorr.h; include/sbv.h:
// sbv_secp256k1_schnorr_verify, _expand_keys, _sign and their _stream forms).
//
//   k_k256_schnorr_verify   one signature per lane per pass: x-only key, message, R.x | s -> ok
//   k_k256_schnorr_expand   one lane per key: d' -> the record d | P.x, P.x alone (optional) and ok
//   k_k256_schnorr_sign     one lane per signature: record + message + aux -> R.x | s and ok
//   k_k256_schnorr_op       test only (sbv_debug_secp256k1_schnorr_op): one case of a unit operation per lane
//
// The verifier is shaped exactly like k_k256_recover (k256_recover_kernels.hip): a lane needs a strip of SBV_K256_QTAB_WORDS dwords
// for the table 1..8 P, the grid is capped at SBV_K256_RECOVER_LANES lanes, lane L handles items L, L + LANES, ... on its own strip of
// the caller's workspace.  Expand and sign are launched like k_k256_pubkeys and k_k256_sign: one lane per item.  No LDS declared, no
// atomics, no cross-lane traffic.  The SHA-256 compression is a call (hmac_sha256_dev.h).  The compiler's figures for the kernels are
// in DESIGN.md ("BIP-340 Schnorr signatures").
//
// Expand and sign are NOT constant-time (see k256_schnorr.h).
#include <hip/hip_runtime.h>

#include "k256_schnorr.h"
#include "k256_schnorr_kernels.h"
#include "../../include/sbv.h"

namespace sbv {

static_assert(SBV_K256_QTAB_WORDS % 4 == 0, "strips keep the 16-byte alignment of the workspace");
static_assert(SBV_K256_RECOVER_LANES % SBV_VERIFY_BLOCK == 0, "whole workgroups");

// pks / msgs / sigs are byte strings as on the wire (big-endian 32-byte integers)
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_verify(const u32* __restrict__ pks, const u32* __restrict__ msgs,
                                                                           const u32* __restrict__ sigs, size_t n,
                                                                           const kapt* __restrict__ gtab, u32* __restrict__ work,
                                                                           uint8_t* __restrict__ ok) {
    const size_t L = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;          // < SBV_K256_RECOVER_LANES by the launch
    if (L >= n) return;
    u32* strip = work + L * (size_t)SBV_K256_QTAB_WORDS;
    SBV_NOUNROLL
    for (size_t i = L; i < n; i += SBV_K256_RECOVER_LANES) {
        u32 pk[8], m[8], rs[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            pk[k] = __builtin_bswap32(pks[i * 8 + k]);
            m[k] = __builtin_bswap32(msgs[i * 8 + k]);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) rs[k] = __builtin_bswap32(sigs[i * 16 + k]);
        ok[i] = k256_schnorr_verify_lane(pk, m, rs, strip, gtab) ? 1 : 0;
    }
}

__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_expand(const u32* __restrict__ keys, size_t m,
                                                                           const kapt* __restrict__ gtab, u32* __restrict__ expanded,
                                                                           u32* __restrict__ pks, uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= m) return;
    u32 d[8], rec[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = __builtin_bswap32(keys[i * 8 + k]);
    const bool good = k256_schnorr_expand_lane(d, gtab, rec);
#pragma unroll
    for (int k = 0; k < 16; ++k) expanded[i * 16 + k] = __builtin_bswap32(rec[k]);
    if (pks) {
#pragma unroll
        for (int k = 0; k < 8; ++k) pks[i * 8 + k] = __builtin_bswap32(rec[8 + k]);
    }
    ok[i] = good ? 1 : 0;
}

// key_index may be null (i % n_keys); aux may be null (32 zero bytes for every item)
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_sign(const u32* __restrict__ expanded, u32 n_keys,
                                                                         const u32* __restrict__ key_index, const u32* __restrict__ msgs,
                                                                         const u32* __restrict__ aux, size_t n,
                                                                         const kapt* __restrict__ gtab, u32* __restrict__ sigs,
                                                                         uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
    const bool known = kidx < n_keys;
    if (!known) kidx = 0;
    u32 rec[16], m[8], a[8], rs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) rec[k] = __builtin_bswap32(expanded[(size_t)kidx * 16 + k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        m[k] = __builtin_bswap32(msgs[i * 8 + k]);
        a[k] = aux ? __builtin_bswap32(aux[i * 8 + k]) : 0u;
    }
    const bool good = k256_schnorr_sign_lane(rec, m, a, gtab, rs) && known;
#pragma unroll
    for (int k = 0; k < 16; ++k) sigs[i * 16 + k] = good ? __builtin_bswap32(rs[k]) : 0u;
    ok[i] = good ? 1 : 0;
}

// in: n x 192 bytes, out: n x 128 bytes (the records of include/sbv.h); work: n strips
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_op(int op, const u32* __restrict__ in, u32* __restrict__ out, size_t n,
                                                                       const kapt* __restrict__ gtab, u32* __restrict__ work) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_IN_WORDS; ++k) a[k] = __builtin_bswap32(in[i * SBV_K256_SIGN_OP_IN_WORDS + k]);
    k256_schnorr_op_lane(op, a, work + i * (size_t)SBV_K256_QTAB_WORDS, gtab, r);
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_OUT_WORDS; ++k) out[i * SBV_K256_SIGN_OP_OUT_WORDS + k] = __builtin_bswap32(r[k]);
}

static unsigned schnorr_grid(size_t n) { return (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK); }

hipError_t launch_k256_schnorr_verify(const uint8_t* d_pks, const uint8_t* d_msgs, const uint8_t* d_sigs, size_t n, const kapt* d_gtab,
                                      u32* d_work, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lanes = n < (size_t)SBV_K256_RECOVER_LANES ? n : (size_t)SBV_K256_RECOVER_LANES;
    hipLaunchKernelGGL(k_k256_schnorr_verify, dim3(schnorr_grid(lanes)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_pks),
                       reinterpret_cast<const u32*>(d_msgs), reinterpret_cast<const u32*>(d_sigs), n, d_gtab, d_work, d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_schnorr_expand(const uint8_t* d_keys, size_t m, const kapt* d_gtab, uint8_t* d_expanded, uint8_t* d_pks, uint8_t* d_ok,
                                      hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_schnorr_expand, dim3(schnorr_grid(m)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_keys), m,
                       d_gtab, reinterpret_cast<u32*>(d_expanded), reinterpret_cast<u32*>(d_pks), d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_schnorr_sign(const uint8_t* d_expanded, u32 n_keys, const u32* d_key_index, const uint8_t* d_msgs, const uint8_t* d_aux,
                                    size_t n, const kapt* d_gtab, uint8_t* d_sigs, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_schnorr_sign, dim3(schnorr_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_expanded),
                       n_keys, d_key_index, reinterpret_cast<const u32*>(d_msgs), reinterpret_cast<const u32*>(d_aux), n, d_gtab,
                       reinterpret_cast<u32*>(d_sigs), d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_schnorr_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const kapt* d_gtab, u32* d_work, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_schnorr_op, dim3(schnorr_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, op, reinterpret_cast<const u32*>(d_in),
                       reinterpret_cast<u32*>(d_out), n, d_gtab, d_work);
    return hipGetLastError();
}

}  // namespace sbv
