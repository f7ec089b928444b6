// k256_schnorr_keyed_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of
// k256_schnorr_keyed_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "k256_keyed.h"
#include "p256_kernels.h"

namespace sbv {

// items per launch: one lane per item, so the bound is the grid's (2^24 workgroups x SBV_VERIFY_BLOCK lanes at the least)
#define SBV_K256_SCHNORR_KEYED_MAX_N ((size_t)1 << 32)

// n items on `stream`: msgs n x 32 B, sigs n x 64 B (R.x | s), slots n x u32 against the registry `reg` (reg.nkeys > 0) and its key
// array d_kkeys (64 B per slot); d_gcomb: the `gcomb_bits`-wide comb of G of the grouped step -> ok n B.  No scratch.
hipError_t launch_k256_schnorr_verify_keyed(const uint8_t* d_msgs, const uint8_t* d_sigs, const u32* d_slots, size_t n, const K256KeyedRegistry& reg,
                                            const uint8_t* d_kkeys, const kapt* d_gcomb, int gcomb_bits, uint8_t* d_ok, hipStream_t stream);
// pks m x 32 B (x-only) -> keys64 m x 64 B (x | y of lift_x; x | 0^32 for a refused key), ok m B (or nullptr)
hipError_t launch_k256_schnorr_lift(const uint8_t* d_pks, size_t m, uint8_t* d_keys64, uint8_t* d_ok, hipStream_t stream);
// test only (sbv_debug_secp256k1_schnorr_keyed_op): in n x 192 B (u1 | u2), slots n x u32 -> out n x 128 B
hipError_t launch_k256_schnorr_keyed_op(const uint8_t* d_in, const u32* d_slots, uint8_t* d_out, size_t n, const K256KeyedRegistry& reg,
                                        const kapt* d_gcomb, int gcomb_bits, hipStream_t stream);

}  // namespace sbv
