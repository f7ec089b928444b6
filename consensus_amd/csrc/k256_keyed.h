// k256_keyed.h — registered secp256k1 keys (include/sbv.h: sbv_secp256k1_register_keys), the lanes of the keyed step.
//
// A registered key owns a slot of the secp256k1 registry: its 64 key bytes, a valid byte and the 8-bit comb of Q in the layout of
// the grouped step's per-batch combs (33 windows x 128 affine entries of 64 bytes, 270 KiB; k256_qphase_point walks it).  Widened
// slots also own a 16-bit comb in the layout of the comb of G (17 windows x 32 768 entries, 35.7 MB; k256_gphase_point walks it as a
// kgcomb{tab, 16, 17}).  A keyed record is r | s | hash (96 bytes, big-endian): the 160-byte tuple without its key.
//
//   k256_keyed_prep_*        stage A on records: k256_prep_chunk (k256_core.h) behind an accessor that serves r | s | hash from the
//                            record and a zero key — nothing of the key is needed before stage B
//   k256_keyed_verify_lane   stage B, one lane per signature: u1 * G from the context's comb of G, u2 * Q from all 33 windows of the
//                            slot's 8-bit comb — or, when every live lane of the wavefront owns one, from the slot's 16-bit comb —
//                            then k256_rx_matches.  No doublings, no grouping state, every addition exact (kpt_madd).
//   k256_reg_*               the 8-bit comb of a fresh slot on the device: the grouped step's chain / rows / fill lanes with the key
//                            taken from the registry's key array (k256_chain_run_key), so that a slot's table is byte for byte the
//                            grouped step's table of the same key
//   k256_widetab_lane        the 16-bit comb of a slot from its 8-bit comb: no doubling chain (B_j = 2^(16 j) Q is entry 1 of row 2 j,
//                            C_j = 2^8 B_j entry 1 of row 2 j + 1, and rows 2 j + 1 hold a C_j for a = 1..128)
//   k256_keyed_host_comb,    the host builders (k256_core.h: k256_build_window_of): the reference of the self-check and of the
//   k256_keyed_host_wide     emulator
//
// Nothing here forks the field or point arithmetic.  Shared host/device source (tests/emul/k256_keyed_emul.cc runs the same lanes).
#pragma once
#include <string.h>

#include "k256_group.h"

namespace sbv {

#define SBV_K256_REC_BYTES 96                 // r | s | hash
#define SBV_K256_KEY_BYTES 64                 // Qx | Qy
#define SBV_K256_REG_MAX_KEYS 65536u          // registry capacity
#define SBV_K256_WIDE_NONE 0xFFFFFFFFu        // kwidx[slot] of a slot without a 16-bit comb
#define SBV_K256_KEYTAB_ENTRIES (SBV_GTAB_WINDOWS * SBV_GTAB_PER_WINDOW)      // 33 x 128
#define SBV_K256_WIDE_BITS 16
#define SBV_K256_WIDE_WINDOWS 17
#define SBV_K256_WIDE_PER_WINDOW 32768
#define SBV_K256_WIDE_ENTRIES ((size_t)SBV_K256_WIDE_WINDOWS * SBV_K256_WIDE_PER_WINDOW)
#define SBV_K256_WIDE_COMB_BYTES (SBV_K256_WIDE_ENTRIES * 64)                 // 35.7 MB
// the wide-comb builder: a lane fills a run of 64 consecutive multiples of one window; 16 full windows x 512 runs
#define SBV_K256_WIDE_RUN 64
#define SBV_K256_WIDE_RUNS_PER_WINDOW (SBV_K256_WIDE_PER_WINDOW / SBV_K256_WIDE_RUN)
#define SBV_K256_WIDE_LANES ((SBV_K256_WIDE_WINDOWS - 1) * SBV_K256_WIDE_RUNS_PER_WINDOW + 1)
#define SBV_K256_WIDE_TMP_WORDS (SBV_K256_WIDE_RUN * 36)                      // per lane: 64 points x (X, Y, Z, prefix)
// the hot-key pool's builder (k256_group_kernels.hip: k_k256_promote_build): a bounded grid of 64-lane workgroups walks the
// promotions' SBV_K256_WIDE_LANES lanes each; at most 4 wavefronts per CU and 9 KiB of scratch per lane of the grid = 604 MB, fewer
// for a pool so small that a batch's promotions (at most 64, at most the pool) have fewer lanes than that
#define SBV_K256_HOT_BUILD_BLOCKS 1024u
SBV_HD u32 k256_hot_build_blocks(u32 pool) {
    const u32 combs = pool < 64u ? pool : 64u;
    const u32 need = (combs * (u32)SBV_K256_WIDE_LANES + 63u) / 64u;
    return need < SBV_K256_HOT_BUILD_BLOCKS ? need : SBV_K256_HOT_BUILD_BLOCKS;
}

// the device half of the registry as the kernels see it
struct K256KeyedRegistry {
    const kapt* ktab = nullptr;         // [nkeys][33 x 128]
    const uint8_t* kvalid = nullptr;    // [nkeys]
    const kapt* wtab = nullptr;         // 16-bit combs, comb w at w * SBV_K256_WIDE_ENTRIES
    const u32* kwidx = nullptr;         // [nkeys] comb of the slot or SBV_K256_WIDE_NONE; nullptr = no slot is wide
    u32 nkeys = 0;
};

// ---- stage A on records -------------------------------------------------------------------------------------------------------
// The 40 dwords k256_prep_chunk reads of a tuple, from a 96-byte record: r | s | hash, and a zero key (which passes the range check
// Qx, Qy < p: the flag stage A leaves is the verdict on r and s alone; the key's verdict is the slot's valid byte).
struct KRecordWords {
    const u32* p;
    SBV_HD u32 operator[](int i) const { return i < 24 ? p[i] : 0u; }
};
// T records per lane with one inversion (large n), or one record per lane (T = 1: the shorter chain of a small batch).  The lane of
// block b, thread l covers records b * 64 T + l + 64 k.
SBV_HD void k256_keyed_prep_lane(const uint8_t* recs, size_t n, const Scratch& s, size_t first, size_t step, int T) {
    auto words = [&](size_t idx) { return KRecordWords{reinterpret_cast<const u32*>(recs + idx * SBV_K256_REC_BYTES)}; };
    k256_prep_chunk(words, n, s, first, step, T);
}
// records per inversion by batch size: below 2^14 records the device is not full, and one record per lane ends soonest
SBV_HD int k256_keyed_prep_T(size_t n) { return n < ((size_t)1 << 14) ? 1 : n < ((size_t)1 << 17) ? 4 : 8; }

// ---- stage B ------------------------------------------------------------------------------------------------------------------
// Is the lane's signature still undecided: the slot in range, its key a point, r and s in [1, n - 1]
SBV_HD bool k256_keyed_live(const Scratch& s, size_t i, u32 slot, const K256KeyedRegistry& reg) {
    return slot < reg.nkeys && reg.kvalid[slot] != 0 && s.ok[i] != 0;
}
SBV_HD bool k256_keyed_slot_wide(u32 slot, const K256KeyedRegistry& reg) {
    return reg.kwidx != nullptr && slot < reg.nkeys && reg.kwidx[slot] != SBV_K256_WIDE_NONE;
}
// One lane of stage B.  `wide` is uniform over the wavefront: every live lane's slot owns a 16-bit comb (and a lane is live).  A
// dead lane walks slot 0's tables — every slot keeps its 8-bit comb, and comb 0 exists whenever a wavefront is wide — and rejects.
SBV_HD bool k256_keyed_verify_lane(const Scratch& s, size_t i, u32 slot, bool live, const K256KeyedRegistry& reg, const kgcomb& gc, bool wide) {
    u256 u1, u2;
    soa_load(u1, s.u1, s.cap, i);
    soa_load(u2, s.u2, s.cap, i);
    if (!live) slot = 0;
    kjpt R;
    kpt_set_inf(R);
    k256_gphase_point(R, u1, gc);
    if (wide) {
        const u32 w = live ? reg.kwidx[slot] : 0u;
        const kgcomb wc = {reg.wtab + (size_t)w * SBV_K256_WIDE_ENTRIES, SBV_K256_WIDE_BITS, SBV_K256_WIDE_WINDOWS};
        k256_gphase_point(R, u2, wc);
    } else {
        k256_qphase_point(R, u2, reg.ktab + (size_t)slot * SBV_K256_KEYTAB_ENTRIES, 0, SBV_GTAB_WINDOWS);
    }
    u256 r;
    soa_load(r, s.r, s.cap, i);
    return live && k256_rx_matches(R, r);
}

// ---- the 8-bit comb of a registered slot, on the device -----------------------------------------------------------------------
// Chain k of a build covers slot slot0 + k; its scratch (jstate, bases, tmp) is indexed by k as the grouped step's is by the group.
template <class QX>
SBV_HD void k256_reg_chain_run(QX& q, const uint8_t* kkeys, u32 slot0, u32 k, u32* jstate, u32* bases, uint8_t* kvalid) {
    const u32* key = reinterpret_cast<const u32*>(kkeys + (size_t)(slot0 + k) * SBV_K256_KEY_BYTES);
    k256_chain_run_key(q, [&](kfe& x, kfe& y) { return k256_key_load_words(key, x, y); }, k, jstate, bases, kvalid + slot0 + k, 0,
                       SBV_GTAB_WINDOWS - 1);
}
// lane = (k * 33 + j) * 2 + which
SBV_HD void k256_reg_rows_lane(u32 lane, u32 count, u32 slot0, const u32* bases, u32* tmp, kapt* ktab) {
    const u32 which = lane & 1u, w = lane >> 1;
    const u32 k = w / SBV_GTAB_WINDOWS, j = w % SBV_GTAB_WINDOWS;
    if (k >= count) return;
    if (which == 1 && j == SBV_GTAB_WINDOWS - 1) return;
    k256_rows_lane(bases + (size_t)w * SBV_K256_BASES_STRIDE, (int)which, j == SBV_GTAB_WINDOWS - 1,
                   tmp + (size_t)w * SBV_K256_WINDOW_TMP + (size_t)which * SBV_K256_ROWS_TMP_WORDS,
                   ktab + ((size_t)(slot0 + k) * SBV_GTAB_WINDOWS + j) * SBV_GTAB_PER_WINDOW);
}
// lane = (k * 33 + j) * 7 + (a - 1)
SBV_HD void k256_reg_fill_lane(u32 lane, u32 count, u32 slot0, u32* tmp, kapt* ktab) {
    const u32 r = lane % 7u, w = lane / 7u;
    const u32 k = w / SBV_GTAB_WINDOWS, j = w % SBV_GTAB_WINDOWS;
    if (k >= count || j == SBV_GTAB_WINDOWS - 1) return;
    k256_fill_lane(1 + (int)r, tmp + (size_t)w * SBV_K256_WINDOW_TMP + (size_t)r * SBV_K256_FILL_TMP_WORDS,
                   ktab + ((size_t)(slot0 + k) * SBV_GTAB_WINDOWS + j) * SBV_GTAB_PER_WINDOW);
}

// ---- the 16-bit comb of a slot from its 8-bit comb ----------------------------------------------------------------------------
// Window j < 16, run q (0..511): the multiples m0 + 1 .. m0 + 64 of B_j = 2^(16 j) Q with m0 = 64 q = 256 a + 64 c.  The lane climbs to
// m0 B_j with at most two exact additions from the 8-bit comb — a C_j + 64 c B_j for c <= 2, (a + 1) C_j - 64 B_j for c = 3 (the rows
// hold multiples up to 128) — then adds B_j 64 times (kpt_madd: infinity and the doubling at m = 2 are its own cases) and normalises
// the run with one inversion.  Entries are canonical (kapt_store).  Lane 8192 writes the one entry a walk ever reads of window 16:
// 1 * 2^256 Q, entry 1 of row 32 (the scalar is below 2^256, so the top signed digit is 0 or 1); the rest of that window stays zero.
SBV_HD void k256_widetab_lane(const kapt* qtab, u32 lane, u32* tmp, kapt* wide) {
    if (lane == SBV_K256_WIDE_LANES - 1) {
        wide[(size_t)(SBV_K256_WIDE_WINDOWS - 1) * SBV_K256_WIDE_PER_WINDOW] = qtab[(size_t)(SBV_GTAB_WINDOWS - 1) * SBV_GTAB_PER_WINDOW];
        return;
    }
    const u32 j = lane / SBV_K256_WIDE_RUNS_PER_WINDOW, q = lane % SBV_K256_WIDE_RUNS_PER_WINDOW;
    const u32 a = q >> 2, c = q & 3u;
    const kapt* rowB = qtab + (size_t)(2 * j) * SBV_GTAB_PER_WINDOW;
    const kapt* rowC = rowB + SBV_GTAB_PER_WINDOW;
    kfe bx, by, x, y;
    kapt_load(bx, by, rowB);
    kjpt T;
    kpt_set_inf(T);
    const u32 ca = c == 3 ? a + 1 : a;                              // multiple of C_j
    kapt_load(x, y, rowC + (ca == 0 ? 0 : ca - 1));
    kpt_madd(T, T, x, y, false, ca == 0);
    kapt_load(x, y, rowB + 63 + (c == 2 ? 64 : 0));                 // 64 B_j or 128 B_j
    kpt_madd(T, T, x, y, c == 3, c == 0);
    kfe acc = kfe_one();
    SBV_NOUNROLL
    for (int k = 0; k < SBV_K256_WIDE_RUN; ++k) {
        kpt_madd(T, T, bx, by, false, false);                       // never infinity: 0 < m <= 32768 < the group order
        u32* rec = tmp + k * 36;
        kfe_store_raw(rec, T.X); kfe_store_raw(rec + 9, T.Y); kfe_store_raw(rec + 18, T.Z); kfe_store_raw(rec + 27, acc);
        kfe_mul(acc, acc, T.Z);
    }
    kfe inv;
    kfe_inv(inv, acc);
    kapt* out = wide + (size_t)j * SBV_K256_WIDE_PER_WINDOW + (size_t)q * SBV_K256_WIDE_RUN;
    SBV_NOUNROLL
    for (int k = SBV_K256_WIDE_RUN - 1; k >= 0; --k) {
        const u32* rec = tmp + k * 36;
        kfe X, Y, Z, pre, zi, zi2, zi3;
        kfe_load_raw(X, rec); kfe_load_raw(Y, rec + 9); kfe_load_raw(Z, rec + 18); kfe_load_raw(pre, rec + 27);
        kfe_mul(zi, inv, pre);
        kfe_mul(inv, inv, Z);
        kfe_sqr(zi2, zi);
        kfe_mul(zi3, zi2, zi);
        kfe_mul(X, X, zi2);
        kfe_mul(Y, Y, zi3);
        kapt_store(out + k, X, Y);
    }
}

// ---- host builders: the reference ---------------------------------------------------------------------------------------------
// The registry comb of one key, 33 x 128 entries: entry (j, m) = m * 2^(8 j) * Q; window 32 holds its first entry only (the carry
// window's digit is 0 or 1), the others of it are zero.  false = k256_key_load refuses the key: the comb is zeroed, the slot invalid.
inline bool k256_keyed_host_comb(const uint8_t key[SBV_K256_KEY_BYTES], kapt* tab) {
    u32 w[16];
    memcpy(w, key, sizeof(w));
    memset((void*)tab, 0, (size_t)SBV_K256_KEYTAB_ENTRIES * sizeof(kapt));
    kfe x, y;
    if (!k256_key_load_words(w, x, y)) return false;
    for (int j = 0; j < SBV_GTAB_WINDOWS; ++j)
        k256_build_window_of(x, y, 8, j, tab + (size_t)j * SBV_GTAB_PER_WINDOW, j == SBV_GTAB_WINDOWS - 1 ? 1 : SBV_GTAB_PER_WINDOW);
    return true;
}
// Window j of the `bits`-wide comb of a valid key (x, y): 2^(bits - 1) entries, the top window (257 bits of digits) its first only.
// `row` must be zeroed by the caller.
inline void k256_keyed_host_wide_window(const kfe& x, const kfe& y, int bits, int j, kapt* row) {
    const int windows = (257 + bits - 1) / bits;
    k256_build_window_of(x, y, bits, j, row, j == windows - 1 ? 1 : 1 << (bits - 1));
}

}  // namespace sbv
