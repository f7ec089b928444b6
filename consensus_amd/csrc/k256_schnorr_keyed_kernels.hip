// k256_schnorr_keyed_kernels.hip — gfx950 kernels of BIP-340 Schnorr verification against registered secp256k1 keys
// (k256_schnorr_keyed.h; include/sbv.h: sbv_secp256k1_schnorr_verify_keyed, sbv_secp256k1_schnorr_lift_keys and their _stream forms).
//
//   k_k256_schnorr_verify_keyed   one lane per item: message, R.x | s and a slot -> ok.  The challenge from the slot's registered Qx, s G
//                                 from the context's comb of G, -+e Q from the slot's comb — the 16-bit comb when the ballots find that
//                                 every live lane of the wavefront owns one (the rule of k_k256_keyed_verify), else the 8-bit comb — one
//                                 field inversion, one byte stored.  No stage A, no workspace, no cap on the grid.
//   k_k256_schnorr_lift           one lane per x-only key: x -> x | y of lift_x, the bytes sbv_secp256k1_register_keys takes
//   k_k256_schnorr_keyed_op       test only (sbv_debug_secp256k1_schnorr_keyed_op): u1 G + u2 Q_slot through the same walk and ballots
//
// No LDS declared, no atomics; the only cross-lane traffic is the ballots (and the wave_any of k256_qphase_point's carry window).  The
// SHA-256 compression is a call (hmac_sha256_dev.h).  A file of its own: no kernel of another object changes with it.  The
// compiler's figures for the kernels are in DESIGN.md ("BIP-340 Schnorr against registered keys").
#include <hip/hip_runtime.h>

#include "k256_schnorr_keyed.h"
#include "k256_keyed_kernels.h"
#include "k256_schnorr_keyed_kernels.h"

namespace sbv {

// msgs / sigs are byte strings as on the wire (big-endian 32-byte integers).  The lanes behind the batch's end take the last item's
// tables and store nothing, as in k_k256_keyed_verify.
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_verify_keyed(const u32* __restrict__ msgs, const u32* __restrict__ sigs,
                                                                                 const u32* __restrict__ slots, size_t n, K256KeyedRegistry reg,
                                                                                 const uint8_t* __restrict__ kkeys, kgcomb gc,
                                                                                 uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    const bool in = i < n;
    const size_t ii = in ? i : n - 1;
    const u32 slot = slots[ii];
    u32 m[8], rs[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = __builtin_bswap32(msgs[ii * 8 + k]);
#pragma unroll
    for (int k = 0; k < 16; ++k) rs[k] = __builtin_bswap32(sigs[ii * 16 + k]);
    const bool live = in && k256_schnorr_keyed_live(rs, slot, reg);
    // the ballots: dead lanes never decide their wavefront
    const bool lane_wide = k256_keyed_slot_wide(slot, reg);
    const bool wide = k256_keyed_wave_wide(live, lane_wide);
    const bool accept = k256_schnorr_keyed_lane(m, rs, slot, live, reg, kkeys, gc, wide);
    if (in) ok[i] = accept ? 1 : 0;
}

// ok may be null
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_lift(const u32* __restrict__ pks, size_t m, u32* __restrict__ keys,
                                                                         uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= m) return;
    u32 pk[8], key[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) pk[k] = __builtin_bswap32(pks[i * 8 + k]);
    const bool good = k256_schnorr_lift_lane(pk, key);
#pragma unroll
    for (int k = 0; k < 16; ++k) keys[i * 16 + k] = __builtin_bswap32(key[k]);
    if (ok) ok[i] = good ? 1 : 0;
}

// in: n x 192 bytes, out: n x 128 bytes (the records of include/sbv.h)
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_schnorr_keyed_op(const u32* __restrict__ in_recs, const u32* __restrict__ slots,
                                                                             u32* __restrict__ out, size_t n, K256KeyedRegistry reg, kgcomb gc) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    const bool in = i < n;
    const size_t ii = in ? i : n - 1;
    const u32 slot = slots[ii];
    u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_IN_WORDS; ++k) a[k] = __builtin_bswap32(in_recs[ii * SBV_K256_SIGN_OP_IN_WORDS + k]);
    const bool live = in && k256_schnorr_keyed_op_live(slot, reg);
    const bool lane_wide = k256_keyed_slot_wide(slot, reg);
    const bool wide = k256_keyed_wave_wide(live, lane_wide);
    k256_schnorr_keyed_op_lane(a, slot, live, reg, gc, wide, r);
    if (!in) return;
#pragma unroll
    for (int k = 0; k < SBV_K256_SIGN_OP_OUT_WORDS; ++k) out[i * SBV_K256_SIGN_OP_OUT_WORDS + k] = __builtin_bswap32(r[k]);
}

static unsigned schnorr_keyed_grid(size_t n) { return (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK); }

hipError_t launch_k256_schnorr_verify_keyed(const uint8_t* d_msgs, const uint8_t* d_sigs, const u32* d_slots, size_t n, const K256KeyedRegistry& reg,
                                            const uint8_t* d_kkeys, const kapt* d_gcomb, int gcomb_bits, uint8_t* d_ok, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > SBV_K256_SCHNORR_KEYED_MAX_N || reg.nkeys == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_k256_schnorr_verify_keyed, dim3(schnorr_keyed_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_msgs),
                       reinterpret_cast<const u32*>(d_sigs), d_slots, n, reg, d_kkeys, kgcomb_make(d_gcomb, gcomb_bits), d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_schnorr_lift(const uint8_t* d_pks, size_t m, uint8_t* d_keys64, uint8_t* d_ok, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    if (m > SBV_K256_SCHNORR_KEYED_MAX_N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_k256_schnorr_lift, dim3(schnorr_keyed_grid(m)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_pks), m,
                       reinterpret_cast<u32*>(d_keys64), d_ok);
    return hipGetLastError();
}

hipError_t launch_k256_schnorr_keyed_op(const uint8_t* d_in, const u32* d_slots, uint8_t* d_out, size_t n, const K256KeyedRegistry& reg,
                                        const kapt* d_gcomb, int gcomb_bits, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > SBV_K256_SCHNORR_KEYED_MAX_N || reg.nkeys == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_k256_schnorr_keyed_op, dim3(schnorr_keyed_grid(n)), dim3(SBV_VERIFY_BLOCK), 0, stream, reinterpret_cast<const u32*>(d_in), d_slots,
                       reinterpret_cast<u32*>(d_out), n, reg, kgcomb_make(d_gcomb, gcomb_bits));
    return hipGetLastError();
}

}  // namespace sbv
