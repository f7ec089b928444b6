// k256_recover_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of k256_recover_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "p256_kernels.h"

namespace sbv {

// bytes of one lane's table strip (SBV_K256_QTAB_WORDS dwords: a multiple of 16 bytes)
size_t k256_recover_strip_bytes();
// batch recovery (k256_recover.h): sigs n x 64 B (r | s), recid n B, digests n x 32 B, d_gtab = the 16-bit comb of G, flags =
// SBV_K256_RECOVER_LOW_S or 0, d_work = min(n, SBV_K256_RECOVER_LANES) strips, 16-byte aligned -> pubs n x 64 B (Qx | Qy), ok n B
hipError_t launch_k256_recover(const uint8_t* d_sigs, const uint8_t* d_recid, const uint8_t* d_digests, size_t n, u32 flags, const kapt* d_gtab,
                               u32* d_work, uint8_t* d_pubs, uint8_t* d_ok, hipStream_t stream);
// test only: one case of unit operation `op` per lane (sbv_debug_secp256k1_recover_op): in n x 192 B, out n x 128 B, d_work n strips
hipError_t launch_k256_recover_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const kapt* d_gtab, u32* d_work, hipStream_t stream);

}  // namespace sbv
