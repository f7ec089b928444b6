// k256_sign_kernels.hip — gfx950 kernels of the secp256k1 batch signer (k256_sign.h; include/sbv.h: sbv_secp256k1_sign_batch,
// sbv_secp256k1_pubkeys and their _stream forms).
//
//   k_k256_sign      one lane per signature: private key + digest -> r | s, the recovery id and ok
//   k_k256_pubkeys   one lane per key: d -> Qx | Qy and ok
//   k_k256_sign_op   test only (sbv_debug_secp256k1_sign_op): one case of a unit operation per lane
//
// One lane per item, SBV_VERIFY_BLOCK lanes per workgroup, launched like k_p256_sign; no LDS declared (the compiler moves a small
// runtime-indexed private array there on its own), no atomics, no cross-lane traffic: a
// lane reads its own 32-byte digest and a 32-byte key shared by the signatures of that key, and walks k * G over the 16-bit comb of G
// exactly as the one-lane verifier does (k256_add_u1G: 17 mixed additions), so the launch bounds are k_k256_verify's.  The SHA-256
// compression is a call (hmac_sha256_dev.h).  The compiler's figures for the kernels are in DESIGN.md ("secp256k1 batch signing").
//
// NOT constant-time (see k256_sign.h).
#include <hip/hip_runtime.h>

#include "k256_sign.h"
#include "k256_sign_kernels.h"

namespace sbv {

#ifndef SBV_K256_SIGN_LB_WAVES
#define SBV_K256_SIGN_LB_WAVES 2
#endif

// keys / digests / sigs are byte strings as on the wire (big-endian 32-byte integers); recid may be null
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_K256_SIGN_LB_WAVES) void k_k256_sign(const u32* __restrict__ keys, u32 n_keys,
                                                                                       const u32* __restrict__ key_index,
                                                                                       const u32* __restrict__ digests, size_t n,
                                                                                       const kapt* __restrict__ gtab, u32 flags,
                                                                                       u32* __restrict__ sigs, uint8_t* __restrict__ recid,
                                                                                       uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
    const bool known = kidx < n_keys;
    if (!known) kidx = 0;
    u32 d[8], h[8], rs[16], rid;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        d[k] = __builtin_bswap32(keys[(size_t)kidx * 8 + k]);
        h[k] = __builtin_bswap32(digests[i * 8 + k]);
    }
    const bool good = k256_sign_lane(d, h, gtab, flags, rs, rid) && known;
#pragma unroll
    for (int k = 0; k < 16; ++k) sigs[i * 16 + k] = good ? __builtin_bswap32(rs[k]) : 0u;
    if (recid) recid[i] = good ? (uint8_t)rid : 0;
    ok[i] = good ? 1 : 0;
}

__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_K256_SIGN_LB_WAVES) void k_k256_pubkeys(const u32* __restrict__ keys, size_t m,
                                                                                          const kapt* __restrict__ gtab,
                                                                                          u32* __restrict__ pubs, uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= m) return;
    u32 d[8], q[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = __builtin_bswap32(keys[i * 8 + k]);
    const bool good = k256_pubkey_lane(d, gtab, q);
#pragma unroll
    for (int k = 0; k < 16; ++k) pubs[i * 16 + k] = __builtin_bswap32(q[k]);
    ok[i] = good ? 1 : 0;
}

// in: n x 192 bytes, out: n x 128 bytes (the records of include/sbv.h)
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_K256_SIGN_LB_WAVES) void k_k256_sign_op(int op, const u32* __restrict__ in, u32* __restrict__ out,
                                                                                          size_t n, const kapt* __restrict__ gtab) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_IN_WORDS; ++k) a[k] = __builtin_bswap32(in[i * SBV_K256_SIGN_OP_IN_WORDS + k]);
    k256_sign_op_lane(op, a, gtab, r);
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_OUT_WORDS; ++k) out[i * SBV_K256_SIGN_OP_OUT_WORDS + k] = __builtin_bswap32(r[k]);
}

static unsigned sign_grid(size_t n) { return (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK); }

hipError_t launch_k256_sign(const uint8_t* d_keys, u32 n_keys, const u32* d_key_index, const uint8_t* d_digests, size_t n, const kapt* d_gtab,
                            u32 flags, uint8_t* d_sigs, uint8_t* d_recid, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_sign, dim3(sign_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_keys), n_keys, d_key_index,
                       reinterpret_cast<const u32*>(d_digests), n, d_gtab, flags, reinterpret_cast<u32*>(d_sigs), d_recid, d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_pubkeys(const uint8_t* d_keys, size_t m, const kapt* d_gtab, uint8_t* d_pubs, uint8_t* d_ok, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_pubkeys, dim3(sign_grid(m)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_keys), m, d_gtab,
                       reinterpret_cast<u32*>(d_pubs), d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_sign_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const kapt* d_gtab, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_sign_op, dim3(sign_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, op, reinterpret_cast<const u32*>(d_in),
                       reinterpret_cast<u32*>(d_out), n, d_gtab);
    return hipGetLastError();
}

}  // namespace sbv
