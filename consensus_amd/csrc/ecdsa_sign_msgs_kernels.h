// ecdsa_sign_msgs_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of ecdsa_sign_msgs_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "sbv_common.h"

#ifndef SBV_ECDSA_CURVE_P256            // ecdsa_sign_msgs.h
#define SBV_ECDSA_CURVE_P256 0
#define SBV_ECDSA_CURVE_K256 1
#endif

namespace sbv {

// msgs packed, moff n + 1 offsets into them -> digests n x 32 B.  mbytes = the bytes behind d_msgs (~0 when the caller vouches for
// the table): a pair that decreases or ends behind them hashes the empty message and gets mark[i] = 1 (else 0; d_mark n B, or nullptr).
hipError_t launch_sha256_msgs(const uint8_t* d_msgs, const u64* d_moff, size_t n, u64 mbytes, uint8_t* d_digests, uint8_t* d_mark,
                              hipStream_t stream);
// curve = SBV_ECDSA_CURVE_P256 / _K256 (ecdsa_sign_msgs.h).  rs n x 64 B and ok_in n B (or nullptr: every lane ok) from the signer,
// marked: d_lens holds launch_sha256_msgs' marks on entry, and a marked lane is refused -> records n x 72 B, lens n B, ok_out n B (or
// nullptr; may be ok_in);
// low_s negates s > (n - 1) / 2 here and flips bit 0 of recid[i] (n B, or nullptr), which is zeroed for a lane that is not ok.
hipError_t launch_ecdsa_sig_finish(int curve, const uint8_t* d_rs, const uint8_t* d_ok_in, bool marked, size_t n, bool low_s,
                                   uint8_t* d_records, uint8_t* d_lens, uint8_t* d_recid, uint8_t* d_ok_out, hipStream_t stream);

}  // namespace sbv
