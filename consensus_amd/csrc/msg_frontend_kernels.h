// msg_frontend_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and msg_frontend_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "sbv_common.h"

namespace sbv {

// The message front end of the GENERIC verifiers (P-256 and secp256k1 alike): signature i = message d_msgs[d_moff[i] .. d_moff[i + 1]),
// DER bytes d_sigs[d_soff[i] .. d_soff[i + 1]) and key d_keys[64 i .. 64 i + 64) (Qx | Qy; d_keys 4-byte aligned) -> the 160-byte tuple
// r | s | SHA-256(message) | Qx | Qy at d_tuples + 160 i (4-byte aligned).  mbase / sbase / mbytes / sbytes as in launch_msg_frontend:
// the offset-table values of the first byte held in d_msgs / d_sigs and the bytes uploaded behind them; a lane whose slice of the tables
// decreases or leaves the upload gets an empty message and an empty signature (r = s = 0: rejected) and reads nothing outside.
hipError_t launch_msg_frontend_tuples(const uint8_t* d_msgs, const u64* d_moff, const uint8_t* d_sigs, const u64* d_soff, const uint8_t* d_keys,
                                      size_t n, u32* d_tuples, hipStream_t stream, u64 mbase, u64 sbase, u64 mbytes, u64 sbytes);

}  // namespace sbv
