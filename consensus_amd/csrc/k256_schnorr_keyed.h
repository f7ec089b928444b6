// k256_schnorr_keyed.h — BIP-340 Schnorr verification against registered secp256k1 keys (include/sbv.h:
// sbv_secp256k1_schnorr_verify_keyed, sbv_secp256k1_schnorr_lift_keys), one item per lane.
//
// The registry is the one of k256_keyed.h: a slot holds the 64 key bytes Qx | Qy, the 8-bit comb of Q and, when widened, its 16-bit
// comb.  One slot serves both signature schemes of a key, so the registered Qy has either parity.  BIP-340's key is P = lift_x(Qx), the
// point with even y: P = Q for an even Qy and P = -Q for an odd one.  R = s G - e P is therefore s G + u2 Q with u2 = n - e (0 for
// e = 0) under an even Qy and u2 = e under an odd one, and nothing of the per-item work of k256_schnorr_verify_lane that depends on the
// key alone is left: no square root, no table 1..8 P, no doublings, no strip.  Per lane: two compressions (the challenge), the comb of
// G (13 additions at 20 bits), the slot's comb (32.2 additions at 8 bits, 17 at 16 bits) and the one field inversion "y even" needs.
//
//   k256_schnorr_keyed_lane     the verdict of one item; the walk is k256_keyed_verify_lane's (k256_schnorr_keyed_walk is its copy, as
//                               recovery copied its walk: that lane reads its scalars from the scratch planes of stage A)
//   k256_schnorr_lift_lane      x-only key -> x | y of lift_x, the key bytes sbv_secp256k1_register_keys takes; x | 0^32 for a refused key
//   k256_schnorr_keyed_op_lane  test only: u1 | u2 and a slot -> the affine u1 G + u2 Q_slot through the same walk
//
// Which comb a wavefront walks is decided by the caller with the rule of the ECDSA keyed step: k256_keyed_slot_wide per lane
// (k256_keyed.h) and the two ballots of k256_keyed_wave_wide (k256_keyed_kernels.h), the one function k_k256_keyed_verify calls too.
//
// Shared host/device source (tests/emul/k256_schnorr_keyed_emul.cc compiles it with g++).
#pragma once
#include "k256_keyed.h"
#include "k256_schnorr.h"

namespace sbv {

// R = u1 G + u2 Q_slot: the comb of G, then the slot's 16-bit comb when `wide` (uniform over the wavefront), else all 33 windows of
// its 8-bit comb.  A dead lane walks slot 0's tables, as in k256_keyed_verify_lane.
SBV_HD void k256_schnorr_keyed_walk(kjpt& R, const u256& u1, const u256& u2, u32 slot, bool live, const K256KeyedRegistry& reg, const kgcomb& gc,
                                    bool wide) {
    if (!live) slot = 0;
    kpt_set_inf(R);
    k256_gphase_point(R, u1, gc);
    if (wide) {
        const u32 w = live ? reg.kwidx[slot] : 0u;
        const kgcomb wc = {reg.wtab + (size_t)w * SBV_K256_WIDE_ENTRIES, SBV_K256_WIDE_BITS, SBV_K256_WIDE_WINDOWS};
        k256_gphase_point(R, u2, wc);
    } else {
        k256_qphase_point(R, u2, reg.ktab + (size_t)slot * SBV_K256_KEYTAB_ENTRIES, 0, SBV_GTAB_WINDOWS);
    }
}

// Is the item still undecided: the slot in range, its key a point, r < p and s < n (s = 0 is legal, as in k256_schnorr_verify_front).
// sig = r | s as 16 big-endian words.
SBV_HD bool k256_schnorr_keyed_live(const u32 sig[16], u32 slot, const K256KeyedRegistry& reg) {
    u256 r, s;
    u256_from_be_words(r, sig);
    u256_from_be_words(s, sig + 8);
    return slot < reg.nkeys && reg.kvalid[slot] != 0 && lt256(r, k256_p_words()) && lt256(s, k256_n_words());
}

// The scalars of a live item: u1 = s, u2 = -+e by the parity of the registered Qy.  The challenge is hashed before the walk, so that
// only u1, u2 (and r, which the caller keeps) live across the comb loops.  kkeys: the registry's key array, 64 bytes Qx | Qy per slot,
// as registered; a dead lane reads slot 0's key and its scalars are walked but never decide.
SBV_HD void k256_schnorr_keyed_scalars(const u32 msg[8], const u32 sig[16], u32 slot, bool live, const uint8_t* kkeys, u256& u1, u256& u2) {
    const u32* key = reinterpret_cast<const u32*>(kkeys + (size_t)(live ? slot : 0u) * SBV_K256_KEY_BYTES);
    u32 px[8];
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) px[i] = bswap32(key[i]);
    const bool y_odd = (bswap32(key[15]) & 1u) != 0;                  // the low bit of byte 63
    u256 e, ne;
    k256_schnorr_challenge(e, sig, px, msg);
    const u256 zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    (void)sub256(ne, k256_n_words(), e);
    select256(ne, is_zero256(e), zero, ne);                            // e = 0: u2 = 0, not n
    select256(u2, y_odd, e, ne);
    u256_from_be_words(u1, sig + 8);
}

// One item: msg 8 big-endian words, sig = r | s 16 big-endian words.  `live` is k256_schnorr_keyed_live of the lane (false behind the
// batch's end), `wide` the wavefront's verdict of k256_keyed_wave_wide.
SBV_HD bool k256_schnorr_keyed_lane(const u32 msg[8], const u32 sig[16], u32 slot, bool live, const K256KeyedRegistry& reg, const uint8_t* kkeys,
                                    const kgcomb& gc, bool wide) {
    u256 u1, u2;
    k256_schnorr_keyed_scalars(msg, sig, slot, live, kkeys, u1, u2);
    kjpt R;
    k256_schnorr_keyed_walk(R, u1, u2, slot, live, reg, gc, wide);
    u32 q[16];
    return k256_schnorr_final(R, sig, q) && live;
}

// x-only key (8 big-endian words) -> key = x | y of lift_x as 16 big-endian words.  For x >= p or x^3 + 7 no square: x | 0^32 and false.
// No curve point has y = 0 (the group order is odd), so the registry refuses such a key and its slot is invalid.
SBV_HD bool k256_schnorr_lift_lane(const u32 pk[8], u32 key[16]) {
    u256 xw, yw;
    u256_from_be_words(xw, pk);
    kfe x, y;
    const bool ok = k256_lift_r(x, y, xw, 0);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) { key[i] = pk[i]; key[8 + i] = 0; }
    if (ok) {
        kfe_to_words(yw, y);
        u256_to_be_words(key + 8, yw);
    }
    return ok;
}

// ---- test only: one case of the keyed walk (include/sbv.h: sbv_debug_secp256k1_schnorr_keyed_op), in the records of the signer's ----
// op 0: u1 | u2 (below n, the walkers' contract) and a slot -> the affine x | y of u1 G + u2 Q_slot;
// ok = 0 and zero bytes for infinity and for a dead lane (slot out of range or invalid).
#define SBV_K256_SCHNORR_KEYED_OPS 1
SBV_HD bool k256_schnorr_keyed_op_live(u32 slot, const K256KeyedRegistry& reg) { return slot < reg.nkeys && reg.kvalid[slot] != 0; }
SBV_HD void k256_schnorr_keyed_op_lane(const u32 in[SBV_K256_SIGN_OP_IN_WORDS], u32 slot, bool live, const K256KeyedRegistry& reg, const kgcomb& gc,
                                       bool wide, u32 out[SBV_K256_SIGN_OP_OUT_WORDS]) {
    SBV_UNROLL
    for (int i = 0; i < SBV_K256_SIGN_OP_OUT_WORDS; ++i) out[i] = 0;
    u256 u1, u2;
    u256_from_be_words(u1, in);
    u256_from_be_words(u2, in + 8);
    kjpt R;
    k256_schnorr_keyed_walk(R, u1, u2, slot, live, reg, gc, wide);
    u32 q[16];
    const bool ok = k256_recover_finish(R, q) && live;
    if (ok) {
        SBV_UNROLL
        for (int i = 0; i < 16; ++i) out[i] = q[i];
    }
    out[31] = ok ? 1u : 0u;
}

}  // namespace sbv
