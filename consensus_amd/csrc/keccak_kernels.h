// keccak_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of keccak_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "p256_kernels.h"

namespace sbv {

// Keccak-256 of n messages: message i is d_msgs[d_moff[i] .. d_moff[i + 1]) (d_moff: n + 1 entries, 8-byte aligned; d_msgs any alignment,
// null allowed when every message is empty) -> digests n x 32 B; a decreasing offset pair gives 32 zero bytes and reads nothing
hipError_t launch_keccak256_msgs(const uint8_t* d_msgs, const u64* d_moff, size_t n, uint8_t* d_digests, hipStream_t stream);
// pubs n x 64 B (Qx | Qy, not checked against the curve) -> addrs n x 20 B, Keccak-256(Qx | Qy)[12:]
hipError_t launch_k256_addresses(const uint8_t* d_pubs, size_t n, uint8_t* d_addrs, hipStream_t stream);
// launch_k256_recover (k256_recover_kernels.h) with the address in place of the key: addrs n x 20 B (zero where ok is 0), ok n B
hipError_t launch_k256_recover_addr(const uint8_t* d_sigs, const uint8_t* d_recid, const uint8_t* d_digests, size_t n, u32 flags, const kapt* d_gtab,
                                    u32* d_work, uint8_t* d_addrs, uint8_t* d_ok, hipStream_t stream);
// test only: one case of unit operation `op` per lane (sbv_debug_keccak_op): in n x 200 B, out n x 200 B
hipError_t launch_keccak_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, hipStream_t stream);

}  // namespace sbv
