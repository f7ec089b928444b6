// ed25519_sign_kernels.hip — gfx950 kernels of the Ed25519 batch signer (ed25519_sign.h; include/sbv.h: sbv_ed25519_expand_keys,
// sbv_ed25519_sign_msgs and their _stream forms).
//
//   k_ed_sign_expand   one lane per key: seed -> the 96-byte expanded record (a mod L | prefix | A_enc) and, optionally, the public key
//   k_ed_sign          one lane per signature: record + message -> R | S and ok
//   k_ed_sign_op       test only (sbv_debug_ed25519_sign_op): one case of a unit operation per lane
//
// One lane per item, 256 lanes per workgroup, no LDS: a lane's inputs are its own byte ranges (the messages have any length) and a
// record shared by every signature of its key, so there is no contiguous tile to stage.  Between two SHA-512s and one inversion the
// signing lane walks [r]B over the 16-bit comb of B exactly as the one-lane verifier does (ed_add_sB: 16 mixed additions, the next
// entry fetched one addition ahead), so the launch bounds are the verifier's: three wavefronts per SIMD.  The compiler's figures for
// both kernels are in DESIGN.md ("Ed25519 batch signing").
//
// NOT constant-time (see ed25519_sign.h).
#include <hip/hip_runtime.h>

#include "ed25519_kernels.h"
#include "ed25519_sign.h"

namespace sbv {

#ifndef SBV_ED_SIGN_LB_WAVES
#define SBV_ED_SIGN_LB_WAVES 3
#endif

__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_SIGN_LB_WAVES) void k_ed_sign_expand(const u32* __restrict__ seeds, size_t m,
                                                                                          const aniels* __restrict__ btab,
                                                                                          u32* __restrict__ expanded, u32* __restrict__ pks) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= m) return;
    u32 seed[8], rec[SBV_ED_SIGN_REC_WORDS];
#pragma unroll
    for (int k = 0; k < 8; ++k) seed[k] = seeds[i * 8 + k];
    ed_sign_expand_lane(seed, btab, rec);
#pragma unroll
    for (int k = 0; k < SBV_ED_SIGN_REC_WORDS; ++k) expanded[i * SBV_ED_SIGN_REC_WORDS + k] = rec[k];
    if (pks) {
#pragma unroll
        for (int k = 0; k < 8; ++k) pks[i * 8 + k] = rec[16 + k];
    }
}

// sigs is read back by the lane that wrote it (ed_sign_lane: R_enc feeds the challenge hash), so it carries no __restrict__.
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_SIGN_LB_WAVES) void k_ed_sign(const u32* expanded, u32 n_keys, const u32* __restrict__ key_index,
                                                                                   const uint8_t* msgs, const u64* __restrict__ moff, size_t n,
                                                                                   const aniels* __restrict__ btab, u32* sigs,
                                                                                   uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
    const u64 m0 = moff[i], m1 = moff[i + 1];
    u32* sig = sigs + i * 16;
    if (kidx >= n_keys || m1 < m0) {                 // an unknown key or a decreasing offset pair: nothing of the message is read
#pragma unroll
        for (int k = 0; k < 16; ++k) sig[k] = 0u;
        ok[i] = 0;
        return;
    }
    ed_sign_lane(expanded + (size_t)kidx * SBV_ED_SIGN_REC_WORDS, msgs + m0, (size_t)(m1 - m0), btab, sig);
    ok[i] = 1;
}

// op 0: sc25519_muladd, in = k | a | r (96 bytes);  op 1: sc25519_reduce256 (32 bytes);  op 2: encode([s]B), s < L (32 bytes).  out: 32 bytes.
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_SIGN_LB_WAVES) void k_ed_sign_op(int op, const u32* __restrict__ in, u32* __restrict__ out, size_t n,
                                                                                      const aniels* __restrict__ btab) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    u256 res;
    if (op == 0) {
        u256 k, a, r;
#pragma unroll
        for (int j = 0; j < 8; ++j) { k.v[j] = in[i * 24 + j]; a.v[j] = in[i * 24 + 8 + j]; r.v[j] = in[i * 24 + 16 + j]; }
        sc25519_muladd(res, k, a, r);
    } else {
        u256 s;
#pragma unroll
        for (int j = 0; j < 8; ++j) s.v[j] = in[i * 8 + j];
        if (op == 1) sc25519_reduce256(res, s);
        else ed_encode_sB(res.v, s, btab);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) out[i * 8 + j] = res.v[j];
}

static unsigned sign_grid(size_t n) { return (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK); }

hipError_t launch_ed_sign_expand(const uint8_t* d_seeds, size_t m, const aniels* d_btab, uint8_t* d_expanded, uint8_t* d_pks, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed_sign_expand, dim3(sign_grid(m)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_seeds), m, d_btab,
                       reinterpret_cast<u32*>(d_expanded), reinterpret_cast<u32*>(d_pks));
    return hipGetLastError();
}

hipError_t launch_ed_sign(const uint8_t* d_expanded, u32 n_keys, const u32* d_key_index, const uint8_t* d_msgs, const u64* d_moff, size_t n,
                          const aniels* d_btab, uint8_t* d_sigs, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed_sign, dim3(sign_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_expanded), n_keys, d_key_index,
                       d_msgs, d_moff, n, d_btab, reinterpret_cast<u32*>(d_sigs), d_ok);
    return hipGetLastError();
}

hipError_t launch_ed_sign_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const aniels* d_btab, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed_sign_op, dim3(sign_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, op, reinterpret_cast<const u32*>(d_in),
                       reinterpret_cast<u32*>(d_out), n, d_btab);
    return hipGetLastError();
}

}  // namespace sbv
