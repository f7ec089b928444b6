// shaloader.hip — measurement only (tools/bench_ecdsa_sign_msgs.py): k_sha256_msgs of consensus_amd/csrc/ecdsa_sign_msgs_kernels.hip built
// twice from the same lane, once on the word loader (sha256_msg_words) and once on the byte loader (sha256_msg), so that one process can
// time them alternately on the same buffers.  Not linked into libsbv.so.
#include <hip/hip_runtime.h>

#include "../consensus_amd/csrc/ecdsa_sign_msgs.h"

namespace sbv {

template <bool WORDS>
__global__ __launch_bounds__(256) void k_sha256_msgs_loader(const uint8_t* __restrict__ msgs, const u64* __restrict__ moff, size_t n, u64 mbytes,
                                                            u32* __restrict__ digests) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u32 h[8];
    (void)sha256_msgs_lane(msgs, moff[i], moff[i + 1], mbytes, WORDS, h);
#pragma unroll
    for (int k = 0; k < 8; ++k) digests[i * 8 + k] = h[k];
}

}  // namespace sbv

// words != 0: the word loader.  Device pointers; asynchronous on `stream`.  Returns the hipError_t of the launch.
extern "C" int sbvlb_sha256_msgs(int words, const void* d_msgs, const void* d_moff, size_t n, uint64_t mbytes, void* d_digests, void* stream) {
    if (n == 0) return 0;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (words)
        hipLaunchKernelGGL(sbv::k_sha256_msgs_loader<true>, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(d_msgs),
                           static_cast<const sbv::u64*>(d_moff), n, mbytes, static_cast<sbv::u32*>(d_digests));
    else
        hipLaunchKernelGGL(sbv::k_sha256_msgs_loader<false>, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(d_msgs),
                           static_cast<const sbv::u64*>(d_moff), n, mbytes, static_cast<sbv::u32*>(d_digests));
    return (int)hipGetLastError();
}
