// sec1_keys.h — SEC1 public keys (65 bytes 04 | X | Y, 33 bytes 02/03 | X) -> the 64 raw bytes X | Y every ECDSA entry takes, one key per
// lane, for P-256 and secp256k1 (include/sbv.h: sbv_p256_decode_keys, sbv_secp256k1_decode_keys, the _sec1 verify entries).
//
// The rules are SEC1 2.3.4 as Go applies them (elliptic.Unmarshal, elliptic.UnmarshalCompressed):
//   len 65, prefix 04        accepted iff X < p, Y < p and Y^2 = X^3 + a X + b
//   len 33, prefix 02 / 03   accepted iff X < p and X^3 + a X + b is a square; Y is the root whose low bit is the prefix's
//   everything else          refused: any other length, the hybrid prefixes 06 / 07, the one-byte point at infinity
// A refused key is 64 zero bytes: (0, 0) is on neither curve (b != 0), so every verifier rejects against it.
//
// secp256k1 has the arithmetic already (kfe_sqrt and k256_lift_r, k256_recover.h: a compressed key is lift_r with the prefix's low
// bit as the parity).  P-256 had no square root: f29_sqrt below is it, on the carry-free 9 x 29 Montgomery field of p256_fe29.h.
// Nothing here is secret: variable time is fine.
//
// Shared host/device source (tests/emul/sec1_emul.cc compiles it with g++ and the contract assertions; consensus_amd/host builds the
// CPU decoders from the same text).
#pragma once
#include "p256_fe29.h"
#include "k256_recover.h"

namespace sbv {

#ifndef SBV_SEC1_P256
#define SBV_SEC1_P256 0
#define SBV_SEC1_K256 1
#define SBV_SEC1_OPS 2
#endif

// r = a^(2^k), k >= 1.  A loop, never unrolled: the chain below is 253 of these.
SBV_HD void f29_sqr_n(fe29& r, const fe29& a, int k) {
    r = a;
    SBV_NOUNROLL
    for (int i = 0; i < k; ++i) f29_sqr(r, r);
}

// y = a^((p + 1) / 4), a square root of a when a is a square (p = 3 mod 4); returns y^2 == a, which fails exactly for the non-residues
// (y is then a root of -a).  Montgomery domain in and out (R = 2^261).
//   (p + 1) / 4 = 2^254 - 2^222 + 2^190 + 2^94 = (2^32 - 1) 2^222 + 2^190 + 2^94
// so the chain builds a^(2^32 - 1) by doubling the run of ones (31 squarings, 5 products), then 32 squarings . a, 96 squarings . a,
// 94 squarings: 253 squarings and 7 products, and one squaring more for the check.
//
// Reduction form: the full f29_sqr / f29_mul (f29_reduce), not f29_sqrx + f29_red_q.  Input contract: a tight (limbs 0..7 in
// [0, 2^29)) with value in (-3p, 3p).  f29_reduce returns limbs 0..7 EXACT and a value in (A B / R, A B / R + p); with |A|, |B| < 3p
// and R = 32 * 2^256 that is inside (-9p/32, 9p/32 + p), i.e. inside (-0.3p, 1.3p) — tighter than the input bound.  So the bounds are
// a fixed point of the map: every one of the 260 intermediate values is tight with |value| < 1.3p, every column sum is below
// 9 * 2^58 < 3 * 2^60, every doubled limb below 2^30, at any depth.  The wide form would save 16 of ~110 multiply-accumulates per
// squaring but its result (+-4p and more) has to pass f29_red_q before the next squaring, which gives most of that back in a chain
// where every squaring feeds the next one; the full form keeps the contract self-evident.
SBV_HD bool f29_sqrt(fe29& y, const fe29& a) {
    fe29 t, u;
    f29_sqr(t, a);          f29_mul(t, t, a);       // 2 ones
    f29_sqr_n(u, t, 2);     f29_mul(t, u, t);       // 4
    f29_sqr_n(u, t, 4);     f29_mul(t, u, t);       // 8
    f29_sqr_n(u, t, 8);     f29_mul(t, u, t);       // 16
    f29_sqr_n(u, t, 16);    f29_mul(t, u, t);       // 32
    f29_sqr_n(u, t, 32);    f29_mul(u, u, a);       // (2^32 - 1) 2^32 + 1
    f29_sqr_n(u, u, 96);    f29_mul(u, u, a);       // (2^32 - 1) 2^128 + 2^96 + 1
    f29_sqr_n(u, u, 94);                            // (p + 1) / 4
    y = u;
    f29_sqr(t, u);
    fe29 d;
    f29_sub(d, t, a);                               // two tight values: |value| < 4.3p, inside f29_is_zero's 16p
    return f29_is_zero(d);
}

SBV_HD u256 p256_p_words() { u256 r = {SBV_P_LIMBS}; return r; }

// x^3 - 3x + b for a tight X = x R (f29_mul output): c = X (X^2 - 3) + b.  X^2 - 3 has limbs in (-3 * 2^29, 2^29) and X (..) + b
// limbs up to 2^30, both too loose for a product's columns, so each passes one carry step (f29_norm: limbs 0..7 in [0, 2^29 + 4),
// value unchanged).  Values: X^2 - 3 in (-3p, 1.3p), the result in (-0.4p, 2.3p) — inside f29_sqrt's input contract.
SBV_HD void p256_curve_rhs(fe29& c, const fe29& X) {
    const fe29 one = f29_one();
    fe29 t, u;
    f29_sqr(t, X);
    f29_sub(t, t, one);
    f29_sub(t, t, one);
    f29_sub(t, t, one);
    f29_norm(u, t);
    f29_mul(t, X, u);
    f29_add(t, t, f29_b());
    f29_norm(c, t);
}

// Montgomery value -> canonical plain words: one product with the plain integer 1 (a R * 1 / R), then the canonical form
SBV_HD void f29_to_plain(u256& w, const fe29& a) {
    fe29 one = f29_zero(), t, c;
    one.v[0] = 1;
    f29_mul(t, a, one);
    f29_canon(c, t);
    f29_pack(w.v, c);
}

// the point of P-256 with the given x: y = the root of x^3 - 3x + b whose canonical low bit is `parity`.  x (Montgomery) and y
// (Montgomery) for the callers that go on computing, yw the canonical y.  False for xw >= p or when x^3 - 3x + b is no square.
SBV_HD bool p256_lift_x(fe29& x, fe29& y, u256& yw, const u256& xw, u32 parity) {
    if (!lt256(xw, p256_p_words())) return false;
    f29_from_plain(x, xw);
    fe29 c;
    p256_curve_rhs(c, x);
    if (!f29_sqrt(y, c)) return false;
    u256 ny;
    f29_to_plain(yw, y);
    (void)sub256(ny, p256_p_words(), yw);           // y is never 0: the group order is prime, so no point of order two exists
    const bool flip = (yw.v[0] & 1u) != (parity & 1u);
    select256(yw, flip, ny, yw);
    f29_cneg(y, y, flip);
    return true;
}
SBV_HD bool p256_lift_x(fe29& x, fe29& y, const u256& xw, u32 parity) {
    u256 yw;
    return p256_lift_x(x, y, yw, xw, parity);
}

// X < p, Y < p and (X, Y) on the curve
SBV_HD bool p256_point_valid(const u256& xw, const u256& yw) {
    if (!lt256(xw, p256_p_words()) || !lt256(yw, p256_p_words())) return false;
    fe29 x, y, c, l, d;
    f29_from_plain(x, xw);
    f29_from_plain(y, yw);
    p256_curve_rhs(c, x);
    f29_sqr(l, y);
    f29_sub(d, l, c);
    return f29_is_zero(d);
}
SBV_HD bool k256_point_valid(const u256& xw, const u256& yw) {
    if (!lt256(xw, k256_p_words()) || !lt256(yw, k256_p_words())) return false;
    kfe x, y;
    kfe_from_words(x, xw);
    kfe_from_words(y, yw);
    return k256_on_curve(x, y);
}

// One key: key[0 .. len) -> out = X | Y as 16 big-endian words (the layout k_msg_frontend_tuples reads, after the kernel's byte swap).
// Only key[0 .. len) is read, byte by byte, at any alignment: 33 or 65 byte loads against ~270 field multiplications.
template <int CURVE>
SBV_HD bool sec1_decode_lane(const uint8_t* key, size_t len, u32 out[16]) {
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) out[i] = 0;
    if (len != 33 && len != 65) return false;
    const u32 prefix = key[0];
    u256 xw, yw;
    from_be32(xw, key + 1);
    bool ok;
    if (len == 65) {
        if (prefix != 0x04u) return false;
        from_be32(yw, key + 33);
        ok = CURVE == SBV_SEC1_P256 ? p256_point_valid(xw, yw) : k256_point_valid(xw, yw);
    } else {
        if (prefix != 0x02u && prefix != 0x03u) return false;
        if (CURVE == SBV_SEC1_P256) {
            fe29 x, y;
            ok = p256_lift_x(x, y, yw, xw, prefix & 1u);
        } else {
            kfe x, y;
            ok = k256_lift_r(x, y, xw, prefix & 1u);
            if (ok) kfe_to_words(yw, y);
        }
    }
    if (!ok) return false;
    u256_to_be_words(out, xw);
    u256_to_be_words(out + 8, yw);
    return true;
}

// ---- test only: one case of a unit operation (include/sbv.h: sbv_debug_sec1_op), in the records of sbv_debug_secp256k1_recover_op ----
// op 0: a (words 0..7, any 256-bit value: taken mod p) -> a^((p + 1) / 4) in words 0..7; ok = a is a square
// op 1: x (words 0..7), parity (word 15) -> x | y of the lifted point; ok = false for x >= p, a parity above 1 or no point
template <int CURVE>
SBV_HD void sec1_op_lane(int op, const u32 in[SBV_K256_SIGN_OP_IN_WORDS], u32 out[SBV_K256_SIGN_OP_OUT_WORDS]) {
    SBV_UNROLL
    for (int i = 0; i < SBV_K256_SIGN_OP_OUT_WORDS; ++i) out[i] = 0;
    u256 aw, yw;
    u256_from_be_words(aw, in);
    bool ok;
    if (op == 0) {
        if (CURVE == SBV_SEC1_P256) {
            fe29 a, y;
            f29_from_plain(a, aw);
            ok = f29_sqrt(y, a);
            if (ok) f29_to_plain(yw, y);
        } else {
            kfe a, y;
            kfe_from_words(a, aw);
            ok = kfe_sqrt(y, a);
            if (ok) kfe_to_words(yw, y);
        }
        if (ok) u256_to_be_words(out, yw);
    } else {
        if (CURVE == SBV_SEC1_P256) {
            fe29 x, y;
            ok = in[15] <= 1u && p256_lift_x(x, y, yw, aw, in[15]);
        } else {
            kfe x, y;
            ok = in[15] <= 1u && k256_lift_r(x, y, aw, in[15]);
            if (ok) kfe_to_words(yw, y);
        }
        if (ok) {
            u256_to_be_words(out, aw);
            u256_to_be_words(out + 8, yw);
        }
    }
    out[31] = ok ? 1u : 0u;
}

}  // namespace sbv
