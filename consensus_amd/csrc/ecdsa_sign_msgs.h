// ecdsa_sign_msgs.h — the lanes in front of and behind the two ECDSA batch signers (p256_sign.h, k256_sign.h) that turn them into
// raw-message signers (include/sbv.h: sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs, sbv_sha256_msgs):
//
//   sha256_msg_words   SHA-256 of one message, the result of sha256_msg (sha256_dev.h), with a loader that reads the aligned interior
//                      of the message as 32-bit words and only the at most 3 head and 3 tail bytes one by one
//   ecdsa_low_s        s > (n - 1) / 2 -> n - s for the order of P-256 or secp256k1
//   ecdsa_der_record   r | s -> the minimal DER SEQUENCE { INTEGER r, INTEGER s } as a 72-byte record, zero behind its length,
//                      byte for byte what der_encode_sig (consensus_amd/host/p256_host.cc) returns
//
// The signing step between them is the existing kernel of each curve, untouched.  Nothing here is secret-dependent beyond what the
// signers already are: NOT constant-time (low-S branches on s, the encoder on the leading bytes of r and s).
//
// Shared host/device source (tests/emul/ecdsa_sign_msgs_emul.cc compiles it with g++).
#pragma once
#include "sha256_dev.h"

#ifndef SBV_ECDSA_CURVE_P256            // also ecdsa_sign_msgs_kernels.h
#define SBV_ECDSA_CURVE_P256 0
#define SBV_ECDSA_CURVE_K256 1
#endif
#define SBV_ECDSA_DER_WORDS 18          // SBV_ECDSA_DER_MAX / 4 (include/sbv.h)

#ifndef SBV_ECDSA_CONTRACT
#define SBV_ECDSA_CONTRACT(cond) ((void)0)          // tests/emul defines it as an assertion
#endif

namespace sbv {

// ---- SHA-256 with a word loader ------------------------------------------------------------------------------------------------------
// The message is seen through the aligned dwords that cover it: with a = address of msg mod 4, virtual dword k holds the message
// bytes 4k - a .. 4k - a + 3, byte b of it in bits 8b .. 8b + 7 as a little-endian load delivers them.  A dword that lies inside
// msg[0 .. len) is one aligned 32-bit load.  The first dword when a > 0 and the last one when the message ends inside it are put
// together from their bytes inside the message (at most 3 each), the 0x80 that ends the message, and zeros: nothing outside
// msg[0 .. len) is read.  Positions in front of the message are never looked at: the funnel shift below drops them.
SBV_HD u32 sha_msg_dword(const uint8_t* msg, size_t len, size_t a, size_t k) {
    const size_t v = 4 * k;
    if (v >= a && v - a + 4 <= len) {
        const void* p = __builtin_assume_aligned(msg + (v - a), 4);
        u32 d;
        __builtin_memcpy(&d, p, 4);
        return d;
    }
    u32 d = 0;
    SBV_UNROLL
    for (int b = 0; b < 4; ++b) {
        if (v + b < a) continue;
        const size_t pos = v + b - a;
        u32 byte = 0;
        if (pos < len) byte = msg[pos];
        else if (pos == len) byte = 0x80u;
        d |= byte << (8 * b);
    }
    return d;
}

// bits 8 * bytes .. 8 * bytes + 31 of hi : lo, bytes in 0 .. 3
SBV_HD u32 sha_funnel_bytes(u32 hi, u32 lo, u32 bytes) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, bytes);
#else
    return bytes ? (lo >> (8 * bytes)) | (hi << (32 - 8 * bytes)) : lo;
#endif
}

// digest words as sha256_msg returns them; msg may be null when len == 0
SBV_HD void sha256_msg_words(const uint8_t* msg, size_t len, u32 out[8]) {
    u32 st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    const size_t total_blocks = (len + 9 + 63) / 64;
    const size_t a = (size_t)(reinterpret_cast<uintptr_t>(msg) & 3u);
    u32 lo = sha_msg_dword(msg, len, a, 0);
    for (size_t blk = 0; blk < total_blocks; ++blk) {
        u32 w[16];
        SBV_UNROLL
        for (int i = 0; i < 16; ++i) {
            const u32 hi = sha_msg_dword(msg, len, a, blk * 16 + (size_t)i + 1);
            w[i] = bswap32(sha_funnel_bytes(hi, lo, (u32)a));      // message bytes 64 blk + 4 i .. + 3 as a big-endian number
            lo = hi;
        }
        if (blk == total_blocks - 1) {
            const u64 bits = (u64)len * 8;
            w[14] = (u32)(bits >> 32);
            w[15] = (u32)bits;
        }
        sha256_compress(st, w);
    }
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = st[i];
}

// ---- low-S -----------------------------------------------------------------------------------------------------------------------------
// s: canonical limbs, 1 <= s <= n - 1.  Returns whether s was replaced by n - s.
SBV_HD bool ecdsa_low_s(int curve, u256& s) {
    const u256 n_p = {{0xFC632551u, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu}};
    const u256 h_p = {{0x7E3192A8u, 0x79DCE561u, 0xD38BCF42u, 0xDE737D56u, 0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u, 0x7FFFFFFFu}};   // (n - 1) / 2
    const u256 n_k = {{0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}};
    const u256 h_k = {{0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu}};   // (n - 1) / 2
    const u256& n_ = curve == SBV_ECDSA_CURVE_P256 ? n_p : n_k;
    const u256& half = curve == SBV_ECDSA_CURVE_P256 ? h_p : h_k;
    SBV_ECDSA_CONTRACT(curve == SBV_ECDSA_CURVE_P256 || curve == SBV_ECDSA_CURVE_K256);
    SBV_ECDSA_CONTRACT(!is_zero256(s) && lt256(s, n_));
    if (!lt256(half, s)) return false;
    (void)sub256(s, n_, s);
    return true;
}

// ---- DER -------------------------------------------------------------------------------------------------------------------------------
// The record is held as 18 big-endian-valued words W (byte o of the record in bits 24 - 8 (o mod 4) .. of W[o / 4]) and put together
// by OR: every index below is a compile-time constant once the loops are unrolled, so W and x stay in registers.

// ORs the 32 bytes of x (8 big-endian-valued words, word 0 first) into W at byte offset off, off in -31 .. 39; bytes that fall in front
// of the record are dropped (the caller only drops leading zero bytes)
SBV_HD void der_or_int(u32 W[SBV_ECDSA_DER_WORDS], const u32 x[8], int off) {
    SBV_ECDSA_CONTRACT(off >= -31 && off + 32 <= 4 * SBV_ECDSA_DER_WORDS);
    // x sits in front of the record, 32 bytes before it, and moves right by off + 32 = 1 .. 71 bytes: first by the odd bytes, then by
    // whole words in five steps of a barrel shifter.  T[8 ..] is the record.
    const u32 mv = (u32)(off + 32), bs = mv & 3u, ws = mv >> 2;
    u32 T[8 + SBV_ECDSA_DER_WORDS];
    SBV_UNROLL
    for (int j = 0; j < 8 + SBV_ECDSA_DER_WORDS; ++j) {
        const u32 cur = j < 8 ? x[j] : 0u, prev = (j > 0 && j < 9) ? x[j - 1] : 0u;
        T[j] = bs ? (cur >> (8 * bs)) | (prev << (32 - 8 * bs)) : cur;
    }
    SBV_UNROLL
    for (int step = 16; step >= 1; step >>= 1) {
        const bool move = (ws & (u32)step) != 0;
        SBV_UNROLL
        for (int t = 8 + SBV_ECDSA_DER_WORDS - 1; t >= 0; --t) {
            const u32 from = t >= step ? T[t - step] : 0u;
            T[t] = move ? from : T[t];
        }
    }
    SBV_UNROLL
    for (int t = 0; t < SBV_ECDSA_DER_WORDS; ++t) W[t] |= T[8 + t];
}

// x: 8 big-endian-valued words.  z = leading zero bytes that the INTEGER drops (at most 31: zero is one 00 byte), pad = 1 when the
// first byte kept has its top bit set and a 00 goes in front of it.
SBV_HD void der_int_shape(const u32 x[8], u32& z, u32& pad) {
    u32 word = 0, at = 7;
    bool found = false;
    SBV_UNROLL
    for (int i = 0; i < 8; ++i)
        if (!found && x[i] != 0) { found = true; word = x[i]; at = (u32)i; }
    if (!found) { z = 31; pad = 0; return; }
    const u32 lz = (u32)__builtin_clz(word);        // word != 0
    z = 4 * at + (lz >> 3);
    pad = (lz & 7u) == 0 ? 1u : 0u;
}

// rs: r | s as 16 big-endian-valued words (word 0 = the most significant of r), as the sign lanes return them.  rec: the record as
// 18 words IN MEMORY ORDER (store them as they are), zero behind len; len = 8 .. 72.
SBV_HD void ecdsa_der_record(const u32 rs[16], u32 rec[SBV_ECDSA_DER_WORDS], u32& len) {
    u32 zr, pr, zs, ps;
    der_int_shape(rs, zr, pr);
    der_int_shape(rs + 8, zs, ps);
    const u32 lr = 32 - zr + pr, ls = 32 - zs + ps;             // 1 .. 33 content bytes each
    const u32 body = 4 + lr + ls;                               // <= 70 < 128: short form
    u32 W[SBV_ECDSA_DER_WORDS];
    SBV_UNROLL
    for (int t = 0; t < SBV_ECDSA_DER_WORDS; ++t) W[t] = 0;
    W[0] = 0x30000000u | (body << 16) | 0x0200u | lr;
    der_or_int(W, rs, 4 + (int)pr - (int)zr);
    const u32 head_s[8] = {0x02000000u | (ls << 16), 0, 0, 0, 0, 0, 0, 0};      // 02 ls, through the same shifter: no runtime index
    der_or_int(W, head_s, 4 + (int)lr);
    der_or_int(W, rs + 8, 6 + (int)lr + (int)ps - (int)zs);
    len = 2 + body;
    SBV_ECDSA_CONTRACT(len >= 8 && len <= 4 * SBV_ECDSA_DER_WORDS);
    SBV_UNROLL
    for (int t = 0; t < SBV_ECDSA_DER_WORDS; ++t) rec[t] = bswap32(W[t]);
}

// ---- the lanes of the two kernels ------------------------------------------------------------------------------------------------------
// The slice check of k_sha256_msgs (that of k_msg_frontend_tuples): a pair that decreases or ends behind the mbytes message bytes is
// refused.
SBV_HD bool ecdsa_msg_slice_ok(u64 m0, u64 m1, u64 mbytes) { return m0 <= m1 && m1 <= mbytes; }

// k_sha256_msgs: the lane's slice [m0, m1) of the message bytes; a refused pair hashes the empty message.  Returns whether the pair
// was accepted.  digest: 8 words in memory order.
SBV_HD bool sha256_msgs_lane(const uint8_t* msgs, u64 m0, u64 m1, u64 mbytes, bool words, u32 digest[8]) {
    const bool in_order = ecdsa_msg_slice_ok(m0, m1, mbytes);
    if (!in_order) { m0 = m1 = 0; }
    u32 h[8];
    const uint8_t* msg = m1 > m0 ? msgs + m0 : nullptr;
    if (words) sha256_msg_words(msg, (size_t)(m1 - m0), h);
    else sha256_msg(msg, (size_t)(m1 - m0), h);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) digest[i] = bswap32(h[i]);
    return in_order;
}

// k_ecdsa_sig_finish: rs_mem = the signer's 64 bytes r | s as 16 words in memory order, ok = the signer's verdict and no refusal mark.  low_s: apply the
// rule here (P-256; the secp256k1 signer applies its own flag and its recid is already right).  recid is flipped in bit 0 when s is
// negated here.  A lane with ok = false writes zeros and len = 0.
SBV_HD void ecdsa_sig_finish_lane(int curve, const u32 rs_mem[16], bool ok, bool low_s, u32 rec[SBV_ECDSA_DER_WORDS], u32& len, u32& recid) {
    if (!ok) {
        SBV_UNROLL
        for (int t = 0; t < SBV_ECDSA_DER_WORDS; ++t) rec[t] = 0;
        len = 0;
        recid = 0;
        return;
    }
    u32 rs[16];
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) rs[i] = bswap32(rs_mem[i]);
    if (low_s) {
        u256 s;
        SBV_UNROLL
        for (int i = 0; i < 8; ++i) s.v[i] = rs[15 - i];
        if (ecdsa_low_s(curve, s)) recid ^= 1u;
        SBV_UNROLL
        for (int i = 0; i < 8; ++i) rs[15 - i] = s.v[i];
    }
    ecdsa_der_record(rs, rec, len);
}

}  // namespace sbv
