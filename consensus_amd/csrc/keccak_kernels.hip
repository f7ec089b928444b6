// keccak_kernels.hip — gfx950 kernels of Keccak-256 and of Ethereum-style addresses (keccak256_dev.h; include/sbv.h:
// sbv_keccak256_msgs, sbv_secp256k1_addresses, sbv_secp256k1_recover_addresses and their _stream forms).
//
//   k_keccak256_msgs      one message per lane: bytes and an offset table -> 32-byte digests
//   k_k256_addresses      one 64-byte key per lane -> the 20-byte address; a pure hash, no curve check
//   k_k256_recover_addr   the lane of k_k256_recover (k256_recover_kernels.hip: capped grid, the caller's strips, items L, L + LANES, ...)
//                         followed by k256_address: r | s, recid, digest -> address and ok
//   k_keccak_op           test only (sbv_debug_keccak_op): one case of a unit operation per lane
//
// The Keccak state is 50 VGPRs of a lane and never leaves them.  No LDS, no atomics, no cross-lane traffic.  An address is five dwords:
// the stride of addrs is 20 bytes and a lane stores exactly five.
#include <hip/hip_runtime.h>

#include "k256_recover.h"
#include "keccak256_dev.h"
#include "keccak_kernels.h"
#include "../../include/sbv.h"

namespace sbv {

static_assert(SBV_K256_RECOVER_LANES % SBV_VERIFY_BLOCK == 0, "whole workgroups");

__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 4) void k_keccak256_msgs(const uint8_t* __restrict__ msgs, const u64* __restrict__ moff, size_t n,
                                                                  u32* __restrict__ digests) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 m0 = moff[i], m1 = moff[i + 1];
    u32 h[8];
    if (m1 < m0) {                                  // a decreasing offset pair: nothing of the messages is read
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = 0;
    } else {
        keccak256(msgs + m0, (size_t)(m1 - m0), h);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) digests[i * 8 + k] = __builtin_bswap32(h[k]);
}

__global__ __launch_bounds__(SBV_VERIFY_BLOCK) void k_k256_addresses(const u32* __restrict__ pubs, size_t n, u32* __restrict__ addrs) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 q[16], a[5];
#pragma unroll
    for (int k = 0; k < 16; ++k) q[k] = __builtin_bswap32(pubs[i * 16 + k]);
    k256_address(q, a);
#pragma unroll
    for (int k = 0; k < 5; ++k) addrs[i * 5 + k] = __builtin_bswap32(a[k]);
}

// sigs / digests are byte strings as on the wire (big-endian 32-byte integers), as in k_k256_recover
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_recover_addr(const u32* __restrict__ sigs, const uint8_t* __restrict__ recid,
                                                                         const u32* __restrict__ digests, size_t n, u32 flags,
                                                                         const kapt* __restrict__ gtab, u32* __restrict__ work,
                                                                         u32* __restrict__ addrs, uint8_t* __restrict__ ok) {
    const size_t L = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;          // < SBV_K256_RECOVER_LANES by the launch
    if (L >= n) return;
    u32* strip = work + L * (size_t)SBV_K256_QTAB_WORDS;
    SBV_NOUNROLL
    for (size_t i = L; i < n; i += SBV_K256_RECOVER_LANES) {
        u32 rs[16], h[8], q[16], a[5];
#pragma unroll
        for (int k = 0; k < 16; ++k) rs[k] = __builtin_bswap32(sigs[i * 16 + k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = __builtin_bswap32(digests[i * 8 + k]);
        const bool good = k256_recover_lane(rs, recid[i], h, flags, strip, gtab, q);
        k256_address(q, a);                         // the point is dead here: the state takes registers the walk has released
#pragma unroll
        for (int k = 0; k < 5; ++k) addrs[i * 5 + k] = good ? __builtin_bswap32(a[k]) : 0u;
        ok[i] = good ? 1 : 0;
    }
}

// in, out: n x 200 bytes, the 25 little-endian lanes of a state
__global__ __launch_bounds__(SBV_VERIFY_BLOCK) void k_keccak_op(int op, const u32* __restrict__ in, u32* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 a[50], r[50];
#pragma unroll
    for (int k = 0; k < 50; ++k) a[k] = in[i * 50 + k];
    keccak_op_lane(op, a, r);
#pragma unroll
    for (int k = 0; k < 50; ++k) out[i * 50 + k] = r[k];
}

static unsigned lane_grid(size_t n) { return (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK); }

hipError_t launch_keccak256_msgs(const uint8_t* d_msgs, const u64* d_moff, size_t n, uint8_t* d_digests, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_keccak256_msgs, dim3(lane_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, d_msgs, d_moff, n, reinterpret_cast<u32*>(d_digests));
    return hipGetLastError();
}

hipError_t launch_k256_addresses(const uint8_t* d_pubs, size_t n, uint8_t* d_addrs, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_k256_addresses, dim3(lane_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_pubs), n,
                       reinterpret_cast<u32*>(d_addrs));
    return hipGetLastError();
}

hipError_t launch_k256_recover_addr(const uint8_t* d_sigs, const uint8_t* d_recid, const uint8_t* d_digests, size_t n, u32 flags, const kapt* d_gtab,
                                    u32* d_work, uint8_t* d_addrs, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lanes = n < (size_t)SBV_K256_RECOVER_LANES ? n : (size_t)SBV_K256_RECOVER_LANES;
    hipLaunchKernelGGL(k_k256_recover_addr, dim3(lane_grid(lanes)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_sigs), d_recid,
                       reinterpret_cast<const u32*>(d_digests), n, flags, d_gtab, d_work, reinterpret_cast<u32*>(d_addrs), d_ok);
    return hipGetLastError();
}

hipError_t launch_keccak_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_keccak_op, dim3(lane_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, op, reinterpret_cast<const u32*>(d_in),
                       reinterpret_cast<u32*>(d_out), n);
    return hipGetLastError();
}

}  // namespace sbv
