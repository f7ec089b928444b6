// ed25519_keyed.h — registered Ed25519 keys (include/sbv.h: sbv_ed25519_register_keys), the lanes of the keyed step.
//
// A registered key owns a slot of the Ed25519 registry: the 8-bit comb of -A in the layout of the grouped step's per-batch combs
// (32 windows x 128 affine-Niels entries, 384 KiB; ed_qphase_lane reads it), a valid byte and the 32-byte encoding.  Widened slots also
// own a 16-bit comb in the hot-key pool's layout (16 x 32 768 entries at a 128-byte pitch, 64 MiB; ed_qphase_wide_lane walks it).
// A keyed record is R | S | k (96 bytes, little-endian): the 128-byte tuple without A.  The keyed step is four launches:
//
//   ed_keyed_expand_lane     record + slot -> the 128-byte tuple, A copied from the registry (the _msgs_keyed entry instead runs
//                            ed_keyed_msg_frontend_lane, which hashes R | A | M with A from the registry and writes the tuple)
//   ed_gphase_lane           [S]B, unchanged (ed25519_group.h), tuple-major accumulator
//   ed_keyed_qphase_lane     += [k](-A) from the slot's comb, all 32 windows (or 16 from the wide comb); marks the tuple pending
//   ed_finish_lane           unchanged: encode(R) == R_enc, one inversion per SBV_ED_FINISH_T tuples
//
// Nothing here forks the field or point arithmetic: the keyed Q lane is ed_qphase_lane / ed_qphase_wide_lane with the slot taken
// from the caller instead of from the batch's grouping.  Shared host/device source (tests/emul/ed_keyed_emul.cc runs the same lanes).
#pragma once
#include <string.h>

#include "ed25519_group.h"
#include "sha512_dev.h"

namespace sbv {

#define SBV_ED_REC_BYTES 96                // R | S | k
#define SBV_ED_REG_MAX_KEYS 65536u         // registry capacity: 65 536 x 384 KiB = 24 GiB of 8-bit combs
#define SBV_ED_WIDE_NONE 0xFFFFFFFFu       // kwidx[slot] of a slot without a 16-bit comb

// record i + the registry's encoding of slots[i] -> tuple i (R | S | A | k).  An out-of-range slot gets A = 0; the Q lane rejects it.
// 16-byte vectors: records, encodings and tuples are 16-byte aligned.
SBV_HD void ed_keyed_expand_lane(const uint8_t* recs, const u32* slots, size_t i, u32 nkeys, const uint8_t* kenc, uint8_t* tuples) {
    const ed_q4* r = reinterpret_cast<const ed_q4*>(recs + i * SBV_ED_REC_BYTES);
    ed_q4* t = reinterpret_cast<ed_q4*>(tuples + i * 128);
    const u32 slot = slots[i];
    const ed_q4 z = {0u, 0u, 0u, 0u};
    const ed_q4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5];
    ed_q4 a0 = z, a1 = z;
    if (slot < nkeys) {
        const ed_q4* a = reinterpret_cast<const ed_q4*>(kenc + (size_t)slot * 32);
        a0 = a[0];
        a1 = a[1];
    }
    t[0] = r0; t[1] = r1; t[2] = r2; t[3] = r3;
    t[4] = a0; t[5] = a1;
    t[6] = r4; t[7] = r5;
}

// The keyed twin of the message front end (sha512_dev.h: ed_msg_frontend_lane): k = SHA-512(R | A | M) mod L with A = the registry's
// encoding of `slot`.  An out-of-range slot hashes slot 0's encoding (nkeys >= 1 here); its tuple is rejected by the Q lane all the same.
SBV_HD void ed_keyed_msg_frontend_lane(const uint8_t* sig64, u32 slot, u32 nkeys, const uint8_t* kenc, const uint8_t* msg, size_t mlen,
                                       u32* tuple_out) {
    ed_msg_frontend_lane(sig64, kenc + (size_t)(slot < nkeys ? slot : 0u) * 32, msg, mlen, tuple_out);
}

// Does `slot` own a 16-bit comb?  (kwidx == nullptr: no slot does)
SBV_HD bool ed_keyed_slot_wide(u32 slot, u32 nkeys, const u32* kwidx) {
    return kwidx != nullptr && slot < nkeys && kwidx[slot] != SBV_ED_WIDE_NONE;
}

// R (tuple-major gacc, from the G phase) += [k](-A) of tuple i from the registry comb of `slot`: all 32 windows of the 8-bit comb,
// or — wide = the caller found that every lane of its wavefront has a 16-bit comb — the 16 windows of the slot's wide comb.  The
// return value is the tuple's pending flag: S < L, k < L, the slot in range and its key a point.  Every slot keeps its 8-bit comb, so
// a lane of a mixed wavefront is correct either way.
SBV_HD bool ed_keyed_qphase_lane(const uint8_t* tuples, size_t i, u32 slot, u32 nkeys, const aniels* ktab, const uint8_t* kvalid,
                                 const uint8_t* wtab, const u32* kwidx, bool wide, u32* gacc, const uint8_t* okb) {
    if (wide) return ed_qphase_wide_lane(tuples, i, kvalid[slot] != 0, wtab + (size_t)kwidx[slot] * SBV_ED_HOT_COMB_BYTES, gacc, okb);
    return ed_qphase_lane(tuples, i, slot, nkeys, ktab, kvalid, gacc, 0, okb, 0, SBV_ED_KEY_WINDOWS, true, true);
}

// Host: the registry comb of one encoding, 32 x 128 entries, entry (j, m) = m * 2^(8 j) * (-A), canonical affine-Niels (the reference
// builder of the base-point and hot-key combs, ed25519_core.h: build_ed_window_of).  false = Go's SetBytes refuses the encoding: the
// comb is zeroed and the slot is flagged invalid.
inline bool ed_keyed_host_comb(const uint8_t enc[32], aniels* tab) {
    u32 w[8];
    memcpy(w, enc, 32);
    ept A;
    if (!ed_decompress(A, w)) {
        memset((void*)tab, 0, (size_t)SBV_ED_KEYTAB_ENTRIES * sizeof(aniels));
        return false;
    }
    fe25_neg(A.X, A.X);
    fe25_neg(A.T, A.T);
    for (int j = 0; j < SBV_ED_KEY_WINDOWS; ++j) build_ed_window_of(A, 8, j, tab + (size_t)j * SBV_ED_KEY_PER_WINDOW);
    return true;
}

}  // namespace sbv
