#pragma once
#include <hip/hip_runtime.h>

#include "ed25519_core.h"
#include "p256_kernels.h"

namespace sbv {
hipError_t launch_ed25519_verify(const uint8_t* d_tuples, size_t n, u32* d_qtab, const aniels* d_btab, uint8_t* d_bitmap,
                                 hipStream_t stream);
// device buffers of the Ed25519 grouped step that the P-256 GroupBuffers do not already provide
struct EdGroupBuffers {
    // This scheme's comb pool.  ktab: aniels [kc.cap + max_groups][32 x 128] combs of -A; kc is keyed by the 32 key bytes (padded to the
    // cache's 16 words).  kvalid (1 = the slot's key decompressed) is NOT GroupBuffers::kvalid: bytes [0, kc.cap) of that array belong to
    // the P-256 key-table cache and outlive the batch — an Ed25519 batch writing its own group verdicts there invalidated cached P-256
    // keys (found in round 3 by test order).  Hot keys (ed25519_group.h, round 6): combs of -A, SBV_ED_HOT_COMB_BYTES each (16 x 32 768
    // entries at a 128-byte pitch); ptmp = SBV_ED_HOT_TMP_WORDS per resident lane of the builder.
    KeyPool kp;
    uint8_t* okb = nullptr;       // [cap] S < L && k < L
    u32* ungxy = nullptr;         // [cap][20] X | Y of the ungrouped list's keys, left by the key check for the quad form of the one-lane kernel
    size_t cap = 0;
};
// Grouped step (ed25519_group.h).  `b` supplies the grouping arrays, jbases, tmp, acc and gacc (32 words per
// tuple, stride b.gacc_cap); ev_fork of `y` must have been recorded on `stream` before the call.
hipError_t launch_ed25519_verify_grouped(const uint8_t* d_tuples, size_t n, const GroupBuffers& b, const EdGroupBuffers& eb,
                                         u32* d_qtab, const aniels* d_btab, const edcomb& bcomb, uint8_t* d_bitmap, hipStream_t stream,
                                         const GroupSync& y, hipEvent_t* prof = nullptr, int* prof_pairs = nullptr);   // prof: 2 * chunks events, a pair around every k_ed_qphase launch
// message front end: raw signatures / keys / messages -> 128-byte tuples on the device (sha512_dev.h)
hipError_t launch_ed_msg_frontend(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs, const u64* d_moff, size_t n,
                                  u32* d_tuples, hipStream_t stream);
// Registered keys (ed25519_keyed.h): the device view of the registry of the default context
struct EdKeyedRegistry {
    const aniels* ktab;           // [key_cap][32 x 128] 8-bit combs of -A
    const uint8_t* kvalid;        // [key_cap] 1 = the encoding is a point
    const uint8_t* kenc;          // [key_cap][32] the registered encodings
    const uint8_t* wtab;          // 16-bit combs of the widened slots (SBV_ED_HOT_COMB_BYTES each), or nullptr
    const u32* kwidx;             // [key_cap] comb of each slot or SBV_ED_WIDE_NONE; nullptr = no slot is wide
    u32 nkeys;
};
// records (n x 96: R | S | k) + slots -> 128-byte tuples; or signatures + messages + slots -> tuples (k hashed on the device)
hipError_t launch_ed_keyed_expand(const uint8_t* d_recs, const u32* d_slots, size_t n, const EdKeyedRegistry& r, uint8_t* d_tuples, hipStream_t stream);
hipError_t launch_ed_keyed_msg_frontend(const uint8_t* d_sigs, const u32* d_slots, const EdKeyedRegistry& r, const uint8_t* d_msgs, const u64* d_moff,
                                        size_t n, uint8_t* d_tuples, hipStream_t stream);
// G phase | keyed Q phase | finish | pack on `stream`; gacc: n x 160 bytes (16-byte aligned), okb / acc: n bytes
hipError_t launch_ed25519_verify_keyed(const uint8_t* d_tuples, const u32* d_slots, size_t n, const EdKeyedRegistry& r, const edcomb& bcomb,
                                       u32* d_gacc, uint8_t* d_okb, uint8_t* d_acc, uint8_t* d_bitmap, hipStream_t stream);
// 16-bit combs of `count` slots from their 8-bit combs: plist = (slot, comb index) pairs; tmp = blocks x 64 x SBV_ED_HOT_TMP_WORDS words
hipError_t launch_ed_keyed_widen(const u32* d_plist, u32 count, const aniels* d_ktab, u32* d_tmp, u32 blocks, uint8_t* d_wtab, hipStream_t stream);
// Batch signing (ed25519_sign.h, ed25519_sign_kernels.hip).  btab = the 16-bit comb of B of the one-lane kernel (host_build_ed_b16).
// seeds m x 32 -> expanded m x 96 (a mod L | prefix | A_enc) and, unless null, pks m x 32
hipError_t launch_ed_sign_expand(const uint8_t* d_seeds, size_t m, const aniels* d_btab, uint8_t* d_expanded, uint8_t* d_pks, hipStream_t stream);
// signature i = sign(expanded[key_index[i]] or, with a null index, expanded[i % n_keys]; msgs[moff[i] .. moff[i+1])): sigs n x 64, ok n bytes
hipError_t launch_ed_sign(const uint8_t* d_expanded, u32 n_keys, const u32* d_key_index, const uint8_t* d_msgs, const u64* d_moff, size_t n,
                          const aniels* d_btab, uint8_t* d_sigs, uint8_t* d_ok, hipStream_t stream);
// test only: one case of unit operation `op` per lane (sbv_debug_ed25519_sign_op)
hipError_t launch_ed_sign_op(int op, const uint8_t* d_in, uint8_t* d_out, size_t n, const aniels* d_btab, hipStream_t stream);
#define SBV_ED_KEYTAB_ENTRIES_PER_KEY 4096  // 32 windows x 128 entries (ed25519_group.h)
void host_build_ed_b16(aniels* out);      // 16 x 32768 affine-Niels multiples of B: the comb of the one-lane kernel
void host_build_ed_bcomb(int bits, aniels* out);   // edcomb_entries(bits) entries: the grouped step's comb (SBV_ED_B_BITS, default 20), one host thread per window
}  // namespace sbv
