// k256_recover.h — ECDSA public-key recovery over secp256k1, one signature per lane: (r, s, recid, digest) -> Q, the other half of
// the recovery id that the signer emits (k256_sign.h).  The rules are libsecp256k1's ecdsa_recover (include/sbv.h states them):
//   r, s in [1, n - 1], recid in 0..3; x = r (+ n when recid & 2) must be below p; y^2 = x^3 + 7 must be a square and y is the root
//   whose canonical parity is recid & 1; e = digest mod n; u1 = (n - e) r^-1, u2 = s r^-1 (mod n); Q = u2 R' + u1 G must not be
//   infinity.  SBV_K256_RECOVER_LOW_S also refuses s > (n - 1) / 2.
//
// Per lane: one square root (kfe_sqrt: 253 squarings and 13 products, one more squaring for its check), one scalar inversion, the
// one-lane verifier's double-scalar walk on R' instead of a key (k256_mul_u2Q below: the table 1..8 R' in the lane's strip and 32
// signed 4-bit GLV windows), the 16-bit comb of G (k256_add_u1G) and one field inversion for the affine result.  Nothing here is
// secret: variable time is fine.
//
// Shared host/device source (tests/emul/k256_recover_emul.cc compiles it with g++; consensus_amd/host/k256_host.cc builds the CPU
// form from the same front and back ends).
#pragma once
#include "k256_sign.h"

#ifndef SBV_K256_RECOVER_LOW_S
#define SBV_K256_RECOVER_LOW_S 1u       // include/sbv.h
#endif

namespace sbv {

// r = a^(2^k)
SBV_HD void kfe_sqr_n(kfe& r, const kfe& a, int k) {
    r = a;
    SBV_NOUNROLL
    for (int i = 0; i < k; ++i) kfe_sqr(r, r);
}

// y = a^((p + 1) / 4), a square root of a when a is a square (p = 3 mod 4); returns y^2 == a, which fails exactly for the
// non-residues (y is then a root of -a).  (p + 1) / 4 = 2^254 - 2^30 - 244 is, from the top, 223 ones, a zero, 22 ones, four zeros,
// two ones and two zeros, so the chain builds a^(2^k - 1) for k = 2, 3, 6, 9, 11, 22, 44, 88, 176, 220, 223 and joins the three runs:
// 253 squarings and 13 products, then one squaring for the check.  Every operand is a reduced value (the contract of k256_fe.h).
SBV_HD bool kfe_sqrt(kfe& y, const kfe& a) {
    kfe x2, x3, x22, x44, t, u;
    kfe_sqr(t, a);          kfe_mul(x2, t, a);      // 2 ones
    kfe_sqr(t, x2);         kfe_mul(x3, t, a);      // 3
    kfe_sqr_n(t, x3, 3);    kfe_mul(t, t, x3);      // 6
    kfe_sqr_n(t, t, 3);     kfe_mul(t, t, x3);      // 9
    kfe_sqr_n(t, t, 2);     kfe_mul(t, t, x2);      // 11
    kfe_sqr_n(u, t, 11);    kfe_mul(x22, u, t);     // 22
    kfe_sqr_n(u, x22, 22);  kfe_mul(x44, u, x22);   // 44
    kfe_sqr_n(u, x44, 44);  kfe_mul(t, u, x44);     // 88
    kfe_sqr_n(u, t, 88);    kfe_mul(u, u, t);       // 176
    kfe_sqr_n(u, u, 44);    kfe_mul(u, u, x44);     // 220
    kfe_sqr_n(u, u, 3);     kfe_mul(u, u, x3);      // 223
    kfe_sqr_n(u, u, 23);    kfe_mul(u, u, x22);     // 223 ones, a zero, 22 ones
    kfe_sqr_n(u, u, 6);     kfe_mul(u, u, x2);      // four zeros, two ones
    kfe_sqr_n(u, u, 2);                             // two zeros
    y = u;
    kfe_sqr(t, u);
    return kfe_equal(t, a);
}

// the point R' of a signature: x = r (+ n when recid & 2), y = the root of x^3 + 7 with canonical parity recid & 1.  r is any 256-bit
// value here (the range of r is the caller's rule); false when x >= p (only r < p - n can take the + n branch) or x^3 + 7 is no square.
SBV_HD bool k256_lift_r(kfe& x, kfe& y, const u256& r, u32 recid) {
    u256 xw = r;
    if (recid & 2u) {
        if (add256(xw, r, k256_n_words())) return false;
    }
    if (!lt256(xw, k256_p_words())) return false;
    kfe_from_words(x, xw);
    kfe t, c;
    kfe_sqr(t, x);
    kfe_mul(c, t, x);
    kfe seven = kfe_zero();
    seven.v[0] = 7;
    kfe_add(c, c, seven);
    if (!kfe_sqrt(y, c)) return false;
    u256 yw, ny;
    kfe_to_words(yw, y);
    (void)sub256(ny, k256_p_words(), yw);           // y is never 0: the curve has no point of order two
    select256(yw, (yw.v[0] & 1u) != (recid & 1u), ny, yw);
    kfe_from_words(y, yw);
    return true;
}

// the checks and the scalars: false for r or s outside [1, n - 1], recid > 3, a high s under SBV_K256_RECOVER_LOW_S, or no point R'
SBV_HD bool k256_recover_front(const u32 rs[16], u32 recid, const u32 digest[8], u32 flags, kfe& x, kfe& y, u256& u1, u256& u2) {
    u256 r, s, e;
    u256_from_be_words(r, rs);
    u256_from_be_words(s, rs + 8);
    u256_from_be_words(e, digest);
    if (!ksc_valid(r) || !ksc_valid(s) || recid > 3u) return false;
    const u256 half = {{0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu}};   // (n - 1) / 2
    if ((flags & SBV_K256_RECOVER_LOW_S) && lt256(half, s)) return false;
    if (!k256_lift_r(x, y, r, recid)) return false;
    ksc_cond_sub_n(e, e);                          // as the verifier reduces the digest: e < 2^256 < 2 n
    u256 ri, ne;
    const u256 zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    (void)sub256(ne, k256_n_words(), e);
    select256(ne, is_zero256(e), zero, ne);        // e = 0: u1 = 0, not n
    ksc_inv(ri, r);
    ksc_mul(u1, ne, ri);
    ksc_mul(u2, s, ri);
    return true;
}

// R = u2 * (qx, qy) for a point of the curve: the table build (1..8 Q in the lane's strip, one inversion) and the 4-bit signed-window
// GLV walk that k256_verify_lane runs (k256_core.h), statement for statement.  It is a copy and not a function shared with the verifier:
// factoring the walk out of k256_verify_lane moved the scratch bytes of k_k256_verify and k_k256_gphase_generic (DESIGN.md
// "secp256k1 public-key recovery" has the table), so the verifier's source stays untouched.
SBV_HD void k256_mul_u2Q(kjpt& R, const kfe& qx, const kfe& qy, const u256& u2, u32* qtab) {
    // table k * Q, k = 1..8: Jacobian chain parked raw behind the table, normalised with ONE inversion (Montgomery's trick)
    kapt* tab = reinterpret_cast<kapt*>(qtab);
    u32* raw = qtab + 8 * 16;                   // record k - 2 (k = 2..8): X, Y, Z, prefix product of the Zs before it
    kapt_store(tab, qx, qy);
    {
        kjpt T;
        T.X = qx; T.Y = qy; T.Z = kfe_one(); T.inf = false;
        kfe acc = kfe_one();
        SBV_NOUNROLL
        for (int k = 2; k <= 8; ++k) {
            kpt_madd(T, T, qx, qy, false, false);            // k Q; k = 2 takes the doubling branch; never infinity (prime order > 8)
            u32* rec = raw + (k - 2) * 36;
            kfe_store_raw(rec, T.X); kfe_store_raw(rec + 9, T.Y); kfe_store_raw(rec + 18, T.Z); kfe_store_raw(rec + 27, acc);
            kfe_mul(acc, acc, T.Z);
        }
        kfe inv;
        kfe_inv(inv, acc);
        SBV_NOUNROLL
        for (int k = 8; k >= 2; --k) {
            const u32* rec = raw + (k - 2) * 36;
            kfe X, Y, Z, pre, zi, zi2, zi3;
            kfe_load_raw(X, rec); kfe_load_raw(Y, rec + 9); kfe_load_raw(Z, rec + 18); kfe_load_raw(pre, rec + 27);
            kfe_mul(zi, inv, pre);
            kfe_mul(inv, inv, Z);
            kfe_sqr(zi2, zi);
            kfe_mul(zi3, zi2, zi);
            kfe_mul(X, X, zi2);
            kfe_mul(Y, Y, zi3);
            kapt_store(tab + (k - 1), X, Y);
        }
    }
    // u2 * Q = k1 * (+-Q) + k2 * (+-phi(Q)) over 32 signed 4-bit windows and the carry window, as in k256_verify_lane
    u256 k1, k2;
    bool n1, n2;
    ksc_split_lambda(k1, n1, k2, n2, u2);
    const u256 eights = {{0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u, 0u, 0u, 0u, 0u}};
    u256 kk1, kk2;
    (void)add256(kk1, k1, eights);
    (void)add256(kk2, k2, eights);
    const kfe beta = {{0x119501EE, 0x09CB6143, 0x1D626570, 0x0092EA25, 0x034E99CF, 0x03CF561A, 0x1C41B991, 0x056CAF80, 0x007AE96A}};
    kpt_set_inf(R);
    {
        kfe bx;
        kfe_mul(bx, qx, beta);
        kpt_madd(R, R, qx, qy, n1, kk1.v[4] == 0);
        kpt_madd(R, R, bx, qy, n2, kk2.v[4] == 0);
    }
    SBV_NOUNROLL
    for (int j = 31; j >= 0; --j) {
        SBV_NOUNROLL
        for (int d = 0; d < 4; ++d) kpt_dbl(R, R);
        u32 w1 = 0, w2 = 0;
        SBV_UNROLL
        for (int w = 0; w < 4; ++w) { w1 = (j >> 3) == w ? kk1.v[w] : w1; w2 = (j >> 3) == w ? kk2.v[w] : w2; }
        const int d1 = (int)((w1 >> ((j & 7) * 4)) & 15u) - 8;
        const int d2 = (int)((w2 >> ((j & 7) * 4)) & 15u) - 8;
        const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
        kfe x, y;
        kapt_load(x, y, tab + (a1 == 0 ? 0 : a1 - 1));
        kpt_madd(R, R, x, y, (d1 < 0) != n1, d1 == 0);
        kapt_load(x, y, tab + (a2 == 0 ? 0 : a2 - 1));
        kfe_mul(x, x, beta);
        kpt_madd(R, R, x, y, (d2 < 0) != n2, d2 == 0);
    }
}

// Q = u2 (x, y) + u1 G for a point of the curve and u1, u2 < n, in Jacobian coordinates; strip: SBV_K256_QTAB_WORDS dwords, 16-byte aligned
SBV_HD void k256_recover_walk(kjpt& Q, const kfe& x, const kfe& y, const u256& u1, const u256& u2, u32* strip, const kapt* gtab) {
    k256_mul_u2Q(Q, x, y, u2, strip);
    k256_add_u1G(Q, u1, gtab);
}

// affine and canonical, with one inversion: q = Qx | Qy as 16 big-endian words; false (q untouched) for infinity
SBV_HD bool k256_recover_finish(const kjpt& Q, u32 q[16]) {
    if (Q.inf) return false;
    kfe zi, zi2, zi3, ax, ay;
    kfe_inv(zi, Q.Z);
    kfe_sqr(zi2, zi);
    kfe_mul(zi3, zi2, zi);
    kfe_mul(ax, Q.X, zi2);
    kfe_mul(ay, Q.Y, zi3);
    u256 xw, yw;
    kfe_to_words(xw, ax);
    kfe_to_words(yw, ay);
    u256_to_be_words(q, xw);
    u256_to_be_words(q + 8, yw);
    return true;
}

// rs = r | s and digest as big-endian words (the signer's), q = Qx | Qy likewise; a failed lane returns false and q all zero
SBV_HD bool k256_recover_lane(const u32 rs[16], u32 recid, const u32 digest[8], u32 flags, u32* strip, const kapt* gtab, u32 q[16]) {
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) q[i] = 0;
    kfe x, y;
    u256 u1, u2;
    if (!k256_recover_front(rs, recid, digest, flags, x, y, u1, u2)) return false;
    kjpt Q;
    k256_recover_walk(Q, x, y, u1, u2, strip, gtab);
    return k256_recover_finish(Q, q);
}

// ---- test only: one case of a unit operation (include/sbv.h: sbv_debug_secp256k1_recover_op), in the records of the signer's ------------
#define SBV_K256_RECOVER_OPS 3
SBV_HD void k256_recover_op_lane(int op, const u32 in[SBV_K256_SIGN_OP_IN_WORDS], u32* strip, const kapt* gtab, u32 out[SBV_K256_SIGN_OP_OUT_WORDS]) {
    SBV_UNROLL
    for (int i = 0; i < SBV_K256_SIGN_OP_OUT_WORDS; ++i) out[i] = 0;
    bool ok;
    if (op == 0) {                                 // a -> sqrt(a); ok = a is a square
        u256 aw, yw;
        u256_from_be_words(aw, in);
        kfe a, y;
        kfe_from_words(a, aw);
        ok = kfe_sqrt(y, a);
        if (ok) {
            kfe_to_words(yw, y);
            u256_to_be_words(out, yw);
        }
    } else if (op == 1) {                          // r | recid -> x | y of the lifted point
        u256 r, xw, yw;
        u256_from_be_words(r, in);
        kfe x, y;
        ok = in[15] <= 3u && k256_lift_r(x, y, r, in[15]);
        if (ok) {
            kfe_to_words(xw, x);
            kfe_to_words(yw, y);
            u256_to_be_words(out, xw);
            u256_to_be_words(out + 8, yw);
        }
    } else {                                       // x | y | u1 | u2 -> Qx | Qy of u2 (x, y) + u1 G; ok = 0: infinity
        u256 xw, yw, u1, u2;
        u256_from_be_words(xw, in);
        u256_from_be_words(yw, in + 8);
        u256_from_be_words(u1, in + 16);
        u256_from_be_words(u2, in + 24);
        kfe x, y;
        kfe_from_words(x, xw);
        kfe_from_words(y, yw);
        kjpt Q;
        k256_recover_walk(Q, x, y, u1, u2, strip, gtab);
        ok = k256_recover_finish(Q, out);
    }
    out[31] = ok ? 1u : 0u;
}

}  // namespace sbv
