// k256_sign_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of k256_sign_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "p256_kernels.h"

namespace sbv {

// batch signing (k256_sign.h): keys n_keys x 32 B, key_index n x u32 or nullptr (i % n_keys), digests n x 32 B, d_gtab = the 16-bit comb
// of G (host_build_k256_gtable), flags = SBV_K256_SIGN_LOW_S or 0 -> sigs n x 64 B (r | s), recid n B (or nullptr), ok n B
hipError_t launch_k256_sign(const uint8_t* d_keys, u32 n_keys, const u32* d_key_index, const uint8_t* d_digests, size_t n, const kapt* d_gtab,
                            u32 flags, uint8_t* d_sigs, uint8_t* d_recid, uint8_t* d_ok, hipStream_t stream);
// keys m x 32 B -> pubs m x 64 B (Qx | Qy), ok m B
hipError_t launch_k256_pubkeys(const uint8_t* d_keys, size_t m, const kapt* d_gtab, uint8_t* d_pubs, uint8_t* d_ok, hipStream_t stream);
// test only: one case of unit operation `op` per lane (sbv_debug_secp256k1_sign_op): in n x 192 B, out n x 128 B
hipError_t launch_k256_sign_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const kapt* d_gtab, hipStream_t stream);

}  // namespace sbv
