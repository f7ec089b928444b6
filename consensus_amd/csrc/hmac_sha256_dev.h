// hmac_sha256_dev.h — HMAC-SHA256 with a 32-byte key over the fixed message shapes of the RFC 6979 §3.2 DRBG (qlen = hlen = 256), as
// per-lane device code: V (32 bytes), V || tag (33 bytes) and V || tag || x || h (97 bytes).  Shared by the two ECDSA signers
// (p256_sign.h, k256_sign.h), so there is one copy of the schedule.  The SHA-256 compression stays behind a call: a lane's nonce
// costs 22 of them, and inlined they would cost more registers than the point arithmetic next to them.
//
// Shared host/device source (tests/emul compiles it with g++).
#pragma once
#include "sbv_common.h"
#include "sha256_dev.h"

namespace sbv {

inline SBV_HD_NOINLINE void sha256_compress_call(u32 st[8], const u32 w[16]) { sha256_compress(st, w); }

SBV_HD void sha256_iv(u32 st[8]) {
    const u32 iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) st[i] = iv[i];
}
// HMAC-SHA256 with a 32-byte key: the hash states after the key ^ ipad and key ^ opad blocks
struct hmac_key { u32 ist[8], ost[8]; };
SBV_HD void hmac_set_key(hmac_key& hk, const u32 K[8]) {
    u32 w[16];
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? K[i] : 0u) ^ 0x36363636u;
    sha256_iv(hk.ist);
    sha256_compress_call(hk.ist, w);
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? K[i] : 0u) ^ 0x5c5c5c5cu;
    sha256_iv(hk.ost);
    sha256_compress_call(hk.ost, w);
}
// outer hash over the 32-byte inner digest: one block, total length 64 + 32 bytes
SBV_HD void hmac_outer(const hmac_key& hk, const u32 inner[8], u32 out[8]) {
    u32 w[16];
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = inner[i];
    w[8] = 0x80000000u;
    SBV_UNROLL
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 32) * 8;
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = hk.ost[i];
    sha256_compress_call(out, w);
}
// HMAC(K, V), V = 32 bytes
SBV_HD void hmac_v(const hmac_key& hk, const u32 V[8], u32 out[8]) {
    u32 w[16], in[8];
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = V[i];
    w[8] = 0x80000000u;
    SBV_UNROLL
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 32) * 8;
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) in[i] = hk.ist[i];
    sha256_compress_call(in, w);
    hmac_outer(hk, in, out);
}
// HMAC(K, V || tag || x || h), x and h 32 bytes each (97 bytes); tail_only: HMAC(K, V || tag) (33 bytes)
SBV_HD void hmac_v_tag(const hmac_key& hk, const u32 V[8], u32 tag, const u32* x, const u32* h, bool tail_only, u32 out[8]) {
    u32 w[16], in[8];
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) { w[i] = V[i]; in[i] = hk.ist[i]; }
    if (tail_only) {
        w[8] = (tag << 24) | 0x00800000u;
        SBV_UNROLL
        for (int i = 9; i < 15; ++i) w[i] = 0;
        w[15] = (64 + 33) * 8;
        sha256_compress_call(in, w);
    } else {
        // the 65 bytes tag | x | h start at word 8, shifted by one byte against the word grid
        w[8] = (tag << 24) | (x[0] >> 8);
        SBV_UNROLL
        for (int j = 1; j < 8; ++j) w[8 + j] = (x[j - 1] << 24) | (x[j] >> 8);
        sha256_compress_call(in, w);
        w[0] = (x[7] << 24) | (h[0] >> 8);
        SBV_UNROLL
        for (int j = 1; j < 8; ++j) w[j] = (h[j - 1] << 24) | (h[j] >> 8);
        w[8] = (h[7] << 24) | 0x00800000u;
        SBV_UNROLL
        for (int i = 9; i < 15; ++i) w[i] = 0;
        w[15] = (64 + 97) * 8;
        sha256_compress_call(in, w);
    }
    hmac_outer(hk, in, out);
}

// big-endian words (w[0] most significant) <-> u256 (v[0] least significant)
SBV_HD void u256_from_be_words(u256& r, const u32 w[8]) {
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = w[7 - i];
}
SBV_HD void u256_to_be_words(u32 w[8], const u256& a) {
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = a.v[7 - i];
}

}  // namespace sbv
