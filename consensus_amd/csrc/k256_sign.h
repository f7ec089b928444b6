// k256_sign.h — ECDSA signing over secp256k1, one signature per lane, with the deterministic nonce of RFC 6979 §3.2 (HMAC-SHA256
// DRBG): the batch form of api.Signer.Sign for the secp256k1 variant, bit-identical with flags = 0 to the host Signer of
// consensus_amd/host (k256_host.cc: k256_sign_rfc6979) and pinned on the community RFC 6979 known answers
// (tests/golden/rfc6979_k256.json).  Two things beyond the P-256 signer (p256_sign.h), because secp256k1 users expect them:
//   SBV_K256_SIGN_LOW_S   s > (n - 1) / 2 is replaced by n - s (the form Bitcoin- and Ethereum-shaped verifiers insist on; this
//                         layer's own verifier has no such rule and accepts both)
//   recid                 the recovery id 0..3: bit 0 = parity of R.y (flipped when s was negated), bit 1 = R.x >= n
//
// Per lane: 20 SHA-256 compressions for the nonce (hmac_sha256_dev.h, shared with p256_sign.h; 8 more per rejected candidate), k * G
// from the 16-bit comb of G (k256_add_u1G from infinity: 17 mixed additions), one field inversion for the affine x and y, one scalar
// inversion for k^-1, three products mod n.
//
// NOT constant-time: the comb lookups are indexed by digits of the secret nonce and the table lives in HBM, and both inversions
// (modinv30) are variable-time.  This is for test traffic and for a trusted, single-tenant host that already holds the keys in
// memory; a deployment that shares the GPU with untrusted work keeps signing on the CPU.
//
// Shared host/device source (tests/emul/k256_sign_emul.cc compiles it with g++).
#pragma once
#include "hmac_sha256_dev.h"
#include "k256_core.h"

#ifndef SBV_K256_SIGN_LOW_S
#define SBV_K256_SIGN_LOW_S 1u          // include/sbv.h
#endif

namespace sbv {

SBV_HD bool ksc_valid(const u256& a) { return !is_zero256(a) && lt256(a, k256_n_words()); }      // 1 <= a <= n - 1

// affine k * G for k in [1, n - 1], canonical words: the comb walker from infinity and ONE inversion of Z
SBV_HD void k256_base_mul_affine(u256& x, u256& y, const u256& k, const kapt* gtab) {
    kjpt R;
    kpt_set_inf(R);
    k256_add_u1G(R, k, gtab);
    kfe zi, zi2, zi3, ax, ay;
    kfe_inv(zi, R.Z);
    kfe_sqr(zi2, zi);
    kfe_mul(zi3, zi2, zi);
    kfe_mul(ax, R.X, zi2);
    kfe_mul(ay, R.Y, zi3);
    kfe_to_words(x, ax);
    kfe_to_words(y, ay);
}

// The signing equation on plain integers: x is ANY 256-bit value (this function does not know that it was a point's coordinate, so
// that x >= n, which no real nonce reaches — probability ~2^-128 — can be put in front of it), d, e < n, k in [1, n - 1].
// r = x mod n, recid = y_odd | (x >= n ? 2 : 0), s = k^-1 (e + r d) mod n; false when r = 0 or s = 0.
SBV_HD bool k256_sign_finish(const u256& x, bool y_odd, const u256& d, const u256& k, const u256& e, u32 flags, u256& r, u256& s, u32& recid) {
    const u256 n_ = k256_n_words();
    ksc_cond_sub_n(r, x);                          // x < 2^256 < 2 n
    if (is_zero256(r)) return false;
    recid = (y_odd ? 1u : 0u) | (lt256(x, n_) ? 0u : 2u);
    u256 ki, t, sum, dd;
    ksc_inv(ki, k);
    ksc_mul(t, r, d);
    const u32 c = add256(sum, t, e);               // r d + e < 2 n: one conditional subtraction (with the carry)
    const u32 bw = sub256(dd, sum, n_);
    select256(t, c != 0 || bw == 0, dd, sum);
    ksc_mul(s, ki, t);
    if (is_zero256(s)) return false;
    const u256 half = {{0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu}};   // (n - 1) / 2
    if ((flags & SBV_K256_SIGN_LOW_S) && lt256(half, s)) {
        (void)sub256(s, n_, s);                    // -R has the same x and the other y: the verifier's point for (r, n - s)
        recid ^= 1u;
    }
    return true;
}

// (r, s, recid) for a candidate nonce k (plain integers; d in [1, n - 1], e < n); false when k is outside [1, n - 1] or r or s is 0
SBV_HD bool k256_sign_with_nonce(const u256& d, const u256& k, const u256& e, const kapt* gtab, u32 flags, u256& r, u256& s, u32& recid) {
    if (!ksc_valid(k)) return false;
    u256 x, y;
    k256_base_mul_affine(x, y, k, gtab);
    return k256_sign_finish(x, (y.v[0] & 1u) != 0, d, k, e, flags, r, s, recid);
}

// ---- the RFC 6979 §3.2 DRBG, in the steps of sign29_lane (p256_sign.h) -------------------------------------------------------------
struct k256_drbg { u32 K[8], V[8]; hmac_key hk; };     // hk = the key schedule of K

// §3.2 b-g: d_be = int2octets(x), h1 = bits2octets(hash), 8 big-endian words each
SBV_HD void k256_drbg_init(k256_drbg& g, const u32 d_be[8], const u32 h1[8]) {
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) { g.V[i] = 0x01010101u; g.K[i] = 0; }
    SBV_NOUNROLL
    for (u32 round = 0; round < 2; ++round) {
        hmac_set_key(g.hk, g.K);
        hmac_v_tag(g.hk, g.V, round, d_be, h1, false, g.K);
        hmac_set_key(g.hk, g.K);
        hmac_v(g.hk, g.V, g.V);
    }
}
// §3.2 h.2: the next candidate is V (qlen = hlen: one block)
SBV_HD void k256_drbg_next(k256_drbg& g) { hmac_v(g.hk, g.V, g.V); }
// §3.2 h.3 after a rejected candidate: K = HMAC(K, V || 00), V = HMAC(K, V)
SBV_HD void k256_drbg_reject(k256_drbg& g) {
    hmac_v_tag(g.hk, g.V, 0, g.V, g.V, true, g.K);      // tail_only: the two 32-byte fields are not read
    hmac_set_key(g.hk, g.K);
    hmac_v(g.hk, g.V, g.V);
}

// d_be, digest: 8 big-endian words each.  rs: r | s as 16 big-endian words.  false: d outside [1, n - 1] (rs and recid zeroed).
SBV_HD bool k256_sign_lane(const u32 d_be[8], const u32 digest[8], const kapt* gtab, u32 flags, u32 rs[16], u32& recid) {
    u256 d, e;
    u256_from_be_words(d, d_be);
    u256_from_be_words(e, digest);
    ksc_cond_sub_n(e, e);                          // bits2int(h1) mod n; also the e of the signing equation
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) rs[i] = 0;
    recid = 0;
    if (!ksc_valid(d)) return false;
    u32 h1[8];
    u256_to_be_words(h1, e);                       // bits2octets
    k256_drbg g;
    k256_drbg_init(g, d_be, h1);
    SBV_NOUNROLL
    for (int attempt = 0; attempt < 64; ++attempt) {          // §3.2 h; a second pass has probability ~2^-128
        k256_drbg_next(g);
        u256 k, r, s;
        u32 rid;
        u256_from_be_words(k, g.V);
        if (k256_sign_with_nonce(d, k, e, gtab, flags, r, s, rid)) {
            u256_to_be_words(rs, r);
            u256_to_be_words(rs + 8, s);
            recid = rid;
            return true;
        }
        k256_drbg_reject(g);
    }
    return false;
}

// q = Qx | Qy of d * G as 16 big-endian words; false (q zeroed) when d is outside [1, n - 1]
SBV_HD bool k256_pubkey_lane(const u32 d_be[8], const kapt* gtab, u32 q[16]) {
    u256 d, x, y;
    u256_from_be_words(d, d_be);
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) q[i] = 0;
    if (!ksc_valid(d)) return false;
    k256_base_mul_affine(x, y, d, gtab);
    u256_to_be_words(q, x);
    u256_to_be_words(q + 8, y);
    return true;
}

// ---- test only: one case of a unit operation (include/sbv.h: sbv_debug_secp256k1_sign_op) --------------------------------------------
// in: 6 fields, out: 4 fields, each field 8 big-endian words; out field 3 is the operation's ok (0 or 1) as an integer
#define SBV_K256_SIGN_OP_IN_WORDS 48
#define SBV_K256_SIGN_OP_OUT_WORDS 32
#define SBV_K256_SIGN_OPS 4
SBV_HD void k256_sign_op_lane(int op, const u32 in[SBV_K256_SIGN_OP_IN_WORDS], const kapt* gtab, u32 out[SBV_K256_SIGN_OP_OUT_WORDS]) {
    SBV_UNROLL
    for (int i = 0; i < SBV_K256_SIGN_OP_OUT_WORDS; ++i) out[i] = 0;
    bool ok = true;
    if (op == 0) {                                 // d | digest -> k | K | V: the first candidate and the state behind it (V = k)
        u256 d, e;
        u256_from_be_words(d, in);
        u256_from_be_words(e, in + 8);
        ksc_cond_sub_n(e, e);
        ok = ksc_valid(d);
        if (ok) {
            u32 h1[8];
            u256_to_be_words(h1, e);
            k256_drbg g;
            k256_drbg_init(g, in, h1);
            k256_drbg_next(g);
            SBV_UNROLL
            for (int i = 0; i < 8; ++i) { out[i] = g.V[i]; out[8 + i] = g.K[i]; out[16 + i] = g.V[i]; }
        }
    } else if (op == 1) {                          // K | V -> K' | V' | k': the update after a rejected candidate V, and the next one
        k256_drbg g;
        SBV_UNROLL
        for (int i = 0; i < 8; ++i) { g.K[i] = in[i]; g.V[i] = in[8 + i]; }
        hmac_set_key(g.hk, g.K);
        k256_drbg_reject(g);
        SBV_UNROLL
        for (int i = 0; i < 8; ++i) { out[i] = g.K[i]; out[8 + i] = g.V[i]; }
        k256_drbg_next(g);
        SBV_UNROLL
        for (int i = 0; i < 8; ++i) out[16 + i] = g.V[i];
    } else if (op == 2) {                          // k -> affine x | y of k * G
        ok = k256_pubkey_lane(in, gtab, out);
    } else {                                       // x | y_odd | d | k | e | flags -> r | s | recid: k256_sign_finish
        u256 x, d, k, e, r, s;
        u256_from_be_words(x, in);
        u256_from_be_words(d, in + 16);
        u256_from_be_words(k, in + 24);
        u256_from_be_words(e, in + 32);
        u32 rid = 0;
        ok = k256_sign_finish(x, (in[15] & 1u) != 0, d, k, e, in[47], r, s, rid);
        if (ok) {
            u256_to_be_words(out, r);
            u256_to_be_words(out + 8, s);
            out[23] = rid;
        }
    }
    out[31] = ok ? 1u : 0u;
}

}  // namespace sbv
