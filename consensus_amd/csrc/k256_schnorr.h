// k256_schnorr.h — BIP-340 Schnorr signatures over secp256k1, one item per lane: verification of (x-only key, 32-byte message,
// R.x | s), the expansion of a private key into a signing record, and "Default Signing" without its optional final self-verification.
// Nothing of the curve is written again: lift_x is k256_lift_r with recid = 0 (the even root), R = s G - e P is recovery's
// double-scalar walk with u1 = s and u2 = n - e (k256_recover_walk), the affine result is k256_recover_finish, k G comes from the
// 16-bit comb of G (k256_base_mul_affine) and the three tagged hashes are sha256_compress from the midstate of their tag block.
//
// Per lane, verify: one square root, two compressions, the walk (table 1..8 P in the lane's strip, 32 signed 4-bit GLV windows, the
// comb of G), one field inversion; no scalar inversion.  Sign: five compressions, one base multiplication with its field inversion,
// one product mod n.  Expand: one base multiplication, paid once per key and not once per signature (as sbv_ed25519_expand_keys).
//
// The sign and expand lanes are NOT constant-time, for the reasons of k256_sign.h: the comb lookups are indexed by digits of the secret
// nonce (and of the key, in expand) and the table lives in HBM, and the inversion (modinv30) is variable-time.  This is for test
// traffic and for a trusted, single-tenant host that already holds the keys in memory.
//
// Shared host/device source (tests/emul/k256_schnorr_emul.cc compiles it with g++; consensus_amd/host/k256_host.cc builds the CPU
// forms from the same lanes).
#pragma once
#include "k256_recover.h"

namespace sbv {

// ---- the tagged hashes: SHA256(SHA256(tag) | SHA256(tag) | data), started from the state after the constant 64-byte tag block ----------
#define SBV_K256_SCHNORR_TAG_AUX 0
#define SBV_K256_SCHNORR_TAG_NONCE 1
#define SBV_K256_SCHNORR_TAG_CHALLENGE 2
SBV_HD void k256_schnorr_midstate(u32 st[8], int tag) {
    const u32 mid[3][8] = {
        {0x24dd3219u, 0x4eba7e70u, 0xca0fabb9u, 0x0fa3166du, 0x3afbe4b1u, 0x4c44df97u, 0x4aac2739u, 0x249e850au},      // BIP0340/aux
        {0x46615b35u, 0xf4bfbff7u, 0x9f8dc671u, 0x83627ab3u, 0x60217180u, 0x57358661u, 0x21a29e54u, 0x68b07b4cu},      // BIP0340/nonce
        {0x9cecba11u, 0x23925381u, 0x11679112u, 0xd1627e0fu, 0x97c87550u, 0x003cc765u, 0x90f61164u, 0x33e9b66au}};     // BIP0340/challenge
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) st[i] = tag == SBV_K256_SCHNORR_TAG_AUX ? mid[0][i] : tag == SBV_K256_SCHNORR_TAG_NONCE ? mid[1][i] : mid[2][i];
}
// 32 bytes of data: one compression, 64 + 32 bytes in all.  out may be a.
SBV_HD void k256_schnorr_hash32(u32 out[8], int tag, const u32 a[8]) {
    u32 st[8], w[16];
    k256_schnorr_midstate(st, tag);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = a[i];
    w[8] = 0x80000000u;
    SBV_UNROLL
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 32) * 8;
    sha256_compress_call(st, w);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = st[i];
}
// 96 bytes of data a | b | c: two compressions, 64 + 96 bytes in all.  out may be any of the inputs.
SBV_HD void k256_schnorr_hash96(u32 out[8], int tag, const u32 a[8], const u32 b[8], const u32 c[8]) {
    u32 st[8], w[16];
    k256_schnorr_midstate(st, tag);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) { w[i] = a[i]; w[8 + i] = b[i]; }
    sha256_compress_call(st, w);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = c[i];
    w[8] = 0x80000000u;
    SBV_UNROLL
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 96) * 8;
    sha256_compress_call(st, w);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = st[i];
}
// e = int(H_challenge(rx | px | msg)) mod n; 0 is a legal value
SBV_HD void k256_schnorr_challenge(u256& e, const u32 rx[8], const u32 px[8], const u32 msg[8]) {
    u32 h[8];
    k256_schnorr_hash96(h, SBV_K256_SCHNORR_TAG_CHALLENGE, rx, px, msg);
    u256_from_be_words(e, h);
    ksc_cond_sub_n(e, e);                          // 2^256 < 2 n
}

// ---- verification --------------------------------------------------------------------------------------------------------------------
// The last step of BIP-340 "Verify": R must not be infinity, its affine x must equal r as an integer and its y must be even.
// q = x | y as 16 big-endian words (untouched for infinity).
SBV_HD bool k256_schnorr_final(const kjpt& R, const u32 r_be[8], u32 q[16]) {
    if (!k256_recover_finish(R, q)) return false;
    u32 diff = 0;
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) diff |= q[i] ^ r_be[i];
    return diff == 0 && (q[15] & 1u) == 0;
}

// The checks and the scalars of "Verify": false for r >= p, s >= n (s = 0 is legal), pk >= p or pk^3 + 7 no square; else (x, y) =
// lift_x(pk), the root with even y, u1 = s and u2 = n - e (0 for e = 0), so that R = u2 (x, y) + u1 G = s G - e P.
// pk, msg: 8 big-endian words each; sig = r | s as 16 big-endian words.
SBV_HD bool k256_schnorr_verify_front(const u32 pk[8], const u32 msg[8], const u32 sig[16], kfe& x, kfe& y, u256& u1, u256& u2) {
    u256 pkw, r, e;
    u256_from_be_words(pkw, pk);
    u256_from_be_words(r, sig);
    u256_from_be_words(u1, sig + 8);
    if (!lt256(r, k256_p_words()) || !lt256(u1, k256_n_words())) return false;
    if (!k256_lift_r(x, y, pkw, 0)) return false;
    k256_schnorr_challenge(e, sig, pk, msg);
    const u256 zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    (void)sub256(u2, k256_n_words(), e);
    select256(u2, is_zero256(e), zero, u2);        // e = 0: u2 = 0, not n
    return true;
}

// strip: SBV_K256_QTAB_WORDS dwords, 16-byte aligned
SBV_HD bool k256_schnorr_verify_lane(const u32 pk[8], const u32 msg[8], const u32 sig[16], u32* strip, const kapt* gtab) {
    kfe x, y;
    u256 u1, u2;
    if (!k256_schnorr_verify_front(pk, msg, sig, x, y, u1, u2)) return false;
    kjpt R;
    k256_recover_walk(R, x, y, u1, u2, strip, gtab);
    u32 q[16];
    return k256_schnorr_final(R, sig, q);
}

// ---- key expansion -------------------------------------------------------------------------------------------------------------------
// rec = d | P.x as 16 big-endian words for the affine P = (x, y) = d' G: d = d' when y is even, else n - d'
SBV_HD void k256_schnorr_expand_finish(const u256& d0, const u256& x, const u256& y, u32 rec[16]) {
    u256 d, nd;
    (void)sub256(nd, k256_n_words(), d0);
    select256(d, (y.v[0] & 1u) != 0, nd, d0);
    u256_to_be_words(rec, d);
    u256_to_be_words(rec + 8, x);
}
// false (rec all zero) for d' outside [1, n - 1]
SBV_HD bool k256_schnorr_expand_lane(const u32 key[8], const kapt* gtab, u32 rec[16]) {
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) rec[i] = 0;
    u256 d, x, y;
    u256_from_be_words(d, key);
    if (!ksc_valid(d)) return false;
    k256_base_mul_affine(x, y, d, gtab);
    k256_schnorr_expand_finish(d, x, y, rec);
    return true;
}

// ---- signing -------------------------------------------------------------------------------------------------------------------------
// Steps 3 to 5 of the signing lane on plain integers, for the affine R = (x, y) = k' G: k = k' or n - k' by the parity of y, e from
// x | px | msg, sig = x | (k + e d) mod n.  d < n, k' in [1, n - 1].
SBV_HD void k256_schnorr_sign_finish(const u256& d, const u32 px[8], const u256& k0, const u256& x, const u256& y, const u32 msg[8], u32 sig[16]) {
    u256 k, nk, e, t, sum, dd;
    (void)sub256(nk, k256_n_words(), k0);
    select256(k, (y.v[0] & 1u) != 0, nk, k0);
    u32 rx[8];
    u256_to_be_words(rx, x);
    k256_schnorr_challenge(e, rx, px, msg);
    ksc_mul(t, e, d);
    const u32 c = add256(sum, t, k);               // e d + k < 2 n: one conditional subtraction (with the carry)
    const u32 bw = sub256(dd, sum, k256_n_words());
    select256(t, c != 0 || bw == 0, dd, sum);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) sig[i] = rx[i];
    u256_to_be_words(sig + 8, t);
}
// false (sig untouched) for k' outside [1, n - 1]
SBV_HD bool k256_schnorr_sign_with_nonce(const u256& d, const u32 px[8], const u256& k0, const u32 msg[8], const kapt* gtab, u32 sig[16]) {
    if (!ksc_valid(k0)) return false;
    u256 x, y;
    k256_base_mul_affine(x, y, k0, gtab);
    k256_schnorr_sign_finish(d, px, k0, x, y, msg, sig);
    return true;
}

// Steps 1 and 2: t = d XOR H_aux(aux), k' = int(H_nonce(t | P.x | msg)) mod n.  rec = d | P.x from k256_schnorr_expand_lane, msg and aux
// 8 big-endian words each; false for d outside [1, n - 1] (the record of a refused key) or k' = 0.
SBV_HD bool k256_schnorr_nonce(const u32 rec[16], const u32 msg[8], const u32 aux[8], u256& d, u256& k0) {
    u256_from_be_words(d, rec);
    if (!ksc_valid(d)) return false;
    u32 t[8];
    k256_schnorr_hash32(t, SBV_K256_SCHNORR_TAG_AUX, aux);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) t[i] ^= rec[i];
    k256_schnorr_hash96(t, SBV_K256_SCHNORR_TAG_NONCE, t, rec + 8, msg);
    u256_from_be_words(k0, t);
    ksc_cond_sub_n(k0, k0);
    return !is_zero256(k0);
}

// false (sig all zero) for a refused record or a nonce of 0.  NOT constant-time (see the head of this file).
SBV_HD bool k256_schnorr_sign_lane(const u32 rec[16], const u32 msg[8], const u32 aux[8], const kapt* gtab, u32 sig[16]) {
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) sig[i] = 0;
    u256 d, k0;
    if (!k256_schnorr_nonce(rec, msg, aux, d, k0)) return false;
    return k256_schnorr_sign_with_nonce(d, rec + 8, k0, msg, gtab, sig);
}

// ---- test only: one case of a unit operation (include/sbv.h: sbv_debug_secp256k1_schnorr_op), in the records of the signer's -------------
#define SBV_K256_SCHNORR_OPS 4
SBV_HD void k256_schnorr_op_lane(int op, const u32 in[SBV_K256_SIGN_OP_IN_WORDS], u32* strip, const kapt* gtab, u32 out[SBV_K256_SIGN_OP_OUT_WORDS]) {
    (void)strip;
    SBV_UNROLL
    for (int i = 0; i < SBV_K256_SIGN_OP_OUT_WORDS; ++i) out[i] = 0;
    bool ok = true;
    if (op == 0) {                                 // a | b | c, selector in in[47] -> the tagged hash (aux: of a alone)
        const u32 sel = in[47];
        if (sel == 0) k256_schnorr_hash32(out, SBV_K256_SCHNORR_TAG_AUX, in);
        else k256_schnorr_hash96(out, sel == 1 ? SBV_K256_SCHNORR_TAG_NONCE : SBV_K256_SCHNORR_TAG_CHALLENGE, in, in + 8, in + 16);
    } else if (op == 1) {                          // x -> y of lift_x
        u256 xw, yw;
        u256_from_be_words(xw, in);
        kfe x, y;
        ok = k256_lift_r(x, y, xw, 0);
        if (ok) {
            kfe_to_words(yw, y);
            u256_to_be_words(out, yw);
        }
    } else if (op == 2) {                          // X | Y | Z | r (coordinates below p) -> affine x | y; ok = the final check
        u256 w;
        kjpt R;
        u256_from_be_words(w, in);      kfe_from_words(R.X, w);
        u256_from_be_words(w, in + 8);  kfe_from_words(R.Y, w);
        u256_from_be_words(w, in + 16); kfe_from_words(R.Z, w);
        R.inf = is_zero256(w);
        ok = k256_schnorr_final(R, in + 24, out);
    } else {                                       // d | Px | k' | m -> R.x | s
        u256 d, k0;
        u256_from_be_words(d, in);
        u256_from_be_words(k0, in + 16);
        ok = k256_schnorr_sign_with_nonce(d, in + 8, k0, in + 24, gtab, out);
    }
    out[31] = ok ? 1u : 0u;
}

}  // namespace sbv
