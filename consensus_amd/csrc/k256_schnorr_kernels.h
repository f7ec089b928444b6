// k256_schnorr_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of k256_schnorr_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "p256_kernels.h"

namespace sbv {

// batch verification (k256_schnorr.h): pks n x 32 B (x-only), msgs n x 32 B, sigs n x 64 B (R.x | s), d_gtab = the 16-bit comb of G,
// d_work = min(n, SBV_K256_RECOVER_LANES) strips of k256_recover_strip_bytes(), 16-byte aligned -> ok n B
hipError_t launch_k256_schnorr_verify(const uint8_t* d_pks, const uint8_t* d_msgs, const uint8_t* d_sigs, size_t n, const kapt* d_gtab,
                                      u32* d_work, uint8_t* d_ok, hipStream_t stream);
// keys m x 32 B -> expanded m x 64 B (d | P.x), pks m x 32 B (or nullptr), ok m B
hipError_t launch_k256_schnorr_expand(const uint8_t* d_keys, size_t m, const kapt* d_gtab, uint8_t* d_expanded, uint8_t* d_pks, uint8_t* d_ok,
                                      hipStream_t stream);
// expanded n_keys x 64 B, key_index n x u32 or nullptr (i % n_keys), msgs n x 32 B, aux n x 32 B or nullptr (zero bytes) ->
// sigs n x 64 B, ok n B
hipError_t launch_k256_schnorr_sign(const uint8_t* d_expanded, u32 n_keys, const u32* d_key_index, const uint8_t* d_msgs, const uint8_t* d_aux,
                                    size_t n, const kapt* d_gtab, uint8_t* d_sigs, uint8_t* d_ok, hipStream_t stream);
// test only: one case of unit operation `op` per lane (sbv_debug_secp256k1_schnorr_op): in n x 192 B, out n x 128 B, d_work n strips
hipError_t launch_k256_schnorr_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const kapt* d_gtab, u32* d_work, hipStream_t stream);

}  // namespace sbv
