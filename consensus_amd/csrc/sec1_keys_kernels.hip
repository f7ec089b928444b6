// sec1_keys_kernels.hip — gfx950 kernels that decode SEC1 public keys (sec1_keys.h; include/sbv.h: sbv_p256_decode_keys,
// sbv_secp256k1_decode_keys, their _stream forms and the _sec1 verify entries).
//
//   k_sec1_decode_keys<CURVE>   one lane per key, 256 per workgroup: 33 or 65 bytes -> the 64 bytes X | Y that every ECDSA entry and
//                               k_msg_frontend_tuples take, zero bytes for a refused key; optionally one ok byte per key
//   k_sec1_op<CURVE>            test only (sbv_debug_sec1_op): the square root and the lift, one case per lane
//
// No LDS, no atomics, no cross-lane traffic, no scratch strip.  A file of its own: no kernel of another object changes with it.  The
// compiler's figures for the kernels are in DESIGN.md ("SEC1 public keys").
#include <hip/hip_runtime.h>

#include "sec1_keys.h"
#include "sec1_keys_kernels.h"

namespace sbv {

// koff == nullptr: the fixed 33-byte stride.  Otherwise every lane checks ITS OWN pair of offsets against the upload (monotone, inside
// it: the rule k_msg_frontend_tuples applies to message offsets); a pair that is not turns into an empty key — refused, 64 zero
// bytes — instead of a read outside the buffer.  ok may be null.
template <int CURVE>
__global__ __launch_bounds__(256) void k_sec1_decode_keys(const uint8_t* __restrict__ keys, const u64* __restrict__ koff, u64 key_bytes,
                                                          size_t m, u32* __restrict__ keys64, uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    u64 k0, k1;
    if (koff) { k0 = koff[i]; k1 = koff[i + 1]; }
    else      { k0 = (u64)i * 33; k1 = k0 + 33; }
    if (!(k0 <= k1 && k1 <= key_bytes)) k0 = k1 = 0;
    u32 out[16];
    const bool good = sec1_decode_lane<CURVE>(keys + k0, (size_t)(k1 - k0), out);
#pragma unroll
    for (int k = 0; k < 16; ++k) keys64[i * 16 + k] = __builtin_bswap32(out[k]);
    if (ok) ok[i] = good ? 1 : 0;
}

// in: n x 192 bytes, out: n x 128 bytes (the records of include/sbv.h)
template <int CURVE>
__global__ __launch_bounds__(256) void k_sec1_op(int op, const u32* __restrict__ in, u32* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_IN_WORDS; ++k) a[k] = __builtin_bswap32(in[i * SBV_K256_SIGN_OP_IN_WORDS + k]);
    sec1_op_lane<CURVE>(op, a, r);
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_OUT_WORDS; ++k) out[i * SBV_K256_SIGN_OP_OUT_WORDS + k] = __builtin_bswap32(r[k]);
}

static unsigned sec1_grid(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_sec1_decode_keys(int curve, const uint8_t* d_keys, const u64* d_key_offsets, size_t key_bytes, size_t m, uint8_t* d_keys64,
                                   uint8_t* d_ok, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    if (m > SBV_SEC1_MAX_M || (curve != SBV_SEC1_P256 && curve != SBV_SEC1_K256)) return hipErrorInvalidValue;
    if (curve == SBV_SEC1_P256)
        hipLaunchKernelGGL(k_sec1_decode_keys<SBV_SEC1_P256>, dim3(sec1_grid(m)), dim3(256), 0, stream, d_keys, d_key_offsets, (u64)key_bytes, m,
                           reinterpret_cast<u32*>(d_keys64), d_ok);
    else
        hipLaunchKernelGGL(k_sec1_decode_keys<SBV_SEC1_K256>, dim3(sec1_grid(m)), dim3(256), 0, stream, d_keys, d_key_offsets, (u64)key_bytes, m,
                           reinterpret_cast<u32*>(d_keys64), d_ok);
    return hipGetLastError();
}

hipError_t launch_sec1_op(int curve, int op, const uint8_t* d_in, uint8_t* d_out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > SBV_SEC1_MAX_M || (curve != SBV_SEC1_P256 && curve != SBV_SEC1_K256) || op < 0 || op >= SBV_SEC1_OPS) return hipErrorInvalidValue;
    if (curve == SBV_SEC1_P256)
        hipLaunchKernelGGL(k_sec1_op<SBV_SEC1_P256>, dim3(sec1_grid(n)), dim3(256), 0, stream, op, reinterpret_cast<const u32*>(d_in),
                           reinterpret_cast<u32*>(d_out), n);
    else
        hipLaunchKernelGGL(k_sec1_op<SBV_SEC1_K256>, dim3(sec1_grid(n)), dim3(256), 0, stream, op, reinterpret_cast<const u32*>(d_in),
                           reinterpret_cast<u32*>(d_out), n);
    return hipGetLastError();
}

}  // namespace sbv
