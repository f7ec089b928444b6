// msg_frontend_kernels.hip — gfx950 kernel of the generic verifiers' message front end (SURVEY.md §8f row 1 for the tuple path).
//
//   k_msg_frontend_tuples   one lane per signature, 256 per workgroup: SHA-256 of the message, strict DER -> (r, s), the signer's 64 key
//                           bytes copied (16 dwords in, 40 dwords out): the 160-byte tuples k_p256_prep and k_k256_prep consume.  The
//                           lane (sha256_dev.h: msg_frontend_tuple_lane) knows nothing of the curve: both curves launch this kernel.
//
// A translation unit of its own, so that the kernels of p256_kernels.hip compile exactly as they did before it existed.
#include <hip/hip_runtime.h>

#include "msg_frontend_kernels.h"
#include "sha256_dev.h"

namespace sbv {

// mbase / sbase / mbytes / sbytes: as in k_msg_frontend (p256_kernels.hip).  Every lane checks ITS OWN slice of both offset tables
// against the uploads (monotone, inside them); a slice that is not turns into an empty message and an empty signature — a DER failure,
// r = s = 0, rejected — instead of a read outside the staging buffers.  The key is read from the lane's own 64 bytes of an n x 64 array.
__global__ __launch_bounds__(256) void k_msg_frontend_tuples(const uint8_t* __restrict__ msgs, const u64* __restrict__ moff,
                                                             const uint8_t* __restrict__ sigs, const u64* __restrict__ soff,
                                                             const u32* __restrict__ keys, size_t n, u32* __restrict__ tuples,
                                                             u64 mbase, u64 sbase, u64 mbytes, u64 sbytes) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u64 m0 = moff[i] - mbase, m1 = moff[i + 1] - mbase, s0 = soff[i] - sbase, s1 = soff[i + 1] - sbase;
    if (!(m0 <= m1 && m1 <= mbytes && s0 <= s1 && s1 <= sbytes)) { m0 = m1 = 0; s0 = s1 = 0; }      // unsigned: an offset below the base wraps far above the bound
    u32 key[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) key[k] = keys[i * 16 + k];
    u32 t[40];
    msg_frontend_tuple_lane(msgs + m0, (size_t)(m1 - m0), sigs + s0, (size_t)(s1 - s0), key, t);
#pragma unroll
    for (int k = 0; k < 40; ++k) tuples[i * 40 + k] = t[k];
}

hipError_t launch_msg_frontend_tuples(const uint8_t* d_msgs, const u64* d_moff, const uint8_t* d_sigs, const u64* d_soff, const uint8_t* d_keys,
                                      size_t n, u32* d_tuples, hipStream_t stream, u64 mbase, u64 sbase, u64 mbytes, u64 sbytes) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_msg_frontend_tuples, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_msgs, d_moff, d_sigs, d_soff,
                       reinterpret_cast<const u32*>(d_keys), n, d_tuples, mbase, sbase, mbytes, sbytes);
    return hipGetLastError();
}

}  // namespace sbv
