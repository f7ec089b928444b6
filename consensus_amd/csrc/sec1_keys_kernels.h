// sec1_keys_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of sec1_keys_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "sbv_common.h"

namespace sbv {

// the curves and the number of unit ops (sec1_keys.h defines the same values for the builds that take the lane code alone)
#ifndef SBV_SEC1_P256
#define SBV_SEC1_P256 0
#define SBV_SEC1_K256 1
#define SBV_SEC1_OPS 2
#endif

// keys per launch: one lane per key, so the bound is the grid's (2^24 workgroups x 256 lanes at the least)
#define SBV_SEC1_MAX_M ((size_t)1 << 32)

// curve: 0 = P-256, 1 = secp256k1 (anything else: hipErrorInvalidValue).  m SEC1 keys packed in d_keys (key_bytes bytes in all, any
// address).  d_key_offsets == nullptr: key i = d_keys[33 i .. 33 i + 33), and key_bytes must cover 33 m.  Otherwise m + 1 offsets,
// 8-byte aligned; each lane checks its own pair (monotone, inside key_bytes) and a pair that fails is a refused key.
// -> d_keys64 m x 64 B (X | Y, zero for a refused key; 4-byte aligned), d_ok m B (or nullptr).
hipError_t launch_sec1_decode_keys(int curve, const uint8_t* d_keys, const u64* d_key_offsets, size_t key_bytes, size_t m, uint8_t* d_keys64,
                                   uint8_t* d_ok, hipStream_t stream);
// test only (sbv_debug_sec1_op): in n x 192 B -> out n x 128 B; op 0 / 1
hipError_t launch_sec1_op(int curve, int op, const uint8_t* d_in, uint8_t* d_out, size_t n, hipStream_t stream);

}  // namespace sbv
