// ed25519_sign.h — Ed25519 signing (RFC 8032 §5.1.6, pure Ed25519), one signature per lane.  The batch form of api.Signer.Sign for
// the Ed25519 variant (BASELINE.json configs[4]), byte-identical to the host Signer of consensus_amd/host (ed25519_host.cc:
// ed25519_sign), to Go's crypto/ed25519.Sign and to the RFC 8032 §7.1 vectors: the signature is deterministic, so every byte of it
// is checked (tests/test_ed25519_sign_cpu.py, tests/test_gpu_ed25519_sign.py).
//
// Two steps, so that the key expansion is paid once per key and not once per signature:
//   ed_sign_expand_lane   seed (32 bytes) -> the 96-byte expanded record  a mod L | prefix | A_enc  (24 little-endian dwords):
//                         one SHA-512 block, the clamp, a mod L, A = [a mod L]B through the 16-bit comb of B, one inversion.
//   ed_sign_lane          record + message -> R | S:  r = H(prefix | M) mod L, R = [r]B (16 mixed additions, ed_add_sB), one inversion
//                         for R_enc, k = H(R_enc | A_enc | M) mod L (sha512_ram as the verifier's front end has it), S = r + k a mod L.
// Per lane and signature: ceil((32 + len + 17) / 128) + ceil((64 + len + 17) / 128) SHA-512 compressions (2 for messages up to 47
// bytes, 3 up to 79, 4 up to 175), 16 mixed additions, one fe25_inv_gcd, two reductions mod L and one 8 x 8-limb product.
//
// The record holds a mod L and not the clamped a: ed_add_sB takes scalars below 2^253 and a clamped scalar reaches 2^255 - 8.  B has
// order L, so [a mod L]B = [a]B, and S = r + k (a mod L) mod L is the same S.
//
// NOT constant-time: the comb lookups are indexed by digits of the secret scalars a and r and the table lives in HBM; SHA-512 runs
// block by block with a trip count that depends on the message length only.  This is for test traffic and load generation and for a
// trusted, single-tenant host that already holds the seeds in memory; a deployment that shares the GPU with untrusted work keeps
// signing on the CPU.
#pragma once
#include "ed25519_core.h"
#include "sha512_dev.h"

namespace sbv {

#define SBV_ED_SIGN_REC_WORDS 24   // a mod L (8) | prefix (8) | A_enc (8)

SBV_HD void sha512_iv(u64 st[8]) {
    const u64 iv[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                       0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) st[i] = iv[i];
}

// SHA-512 of head[0 .. head_len) | msg[0 .. mlen), head_len = 32 or 64: digest as 8 big-endian-valued 64-bit words.  The sibling of
// sha512_ram for a head in one piece (the nonce hash: head = the 32-byte prefix of the expanded record); block by block per lane,
// lanes of a wavefront finish at different block counts.  head and msg are read byte-wise, wherever they live.
SBV_HD void sha512_head_msg(const uint8_t* head, size_t head_len, const uint8_t* msg, size_t mlen, u64 out[8]) {
    u64 st[8];
    sha512_iv(st);
    const size_t len = head_len + mlen;
    const size_t total_blocks = (len + 17 + 127) / 128;
    for (size_t blk = 0; blk < total_blocks; ++blk) {
        u64 w[16];
        SBV_NOUNROLL
        for (int i = 0; i < 16; ++i) {
            u64 word = 0;
            SBV_NOUNROLL
            for (int k = 0; k < 8; ++k) {
                const size_t pos = blk * 128 + (size_t)i * 8 + k;
                u64 byte = 0;
                if (pos < head_len) byte = head[pos];
                else if (pos < len) byte = msg[pos - head_len];
                else if (pos == len) byte = 0x80u;
                word = (word << 8) | byte;
            }
            w[i] = word;
        }
        if (blk == total_blocks - 1) {
            w[14] = 0;                               // lengths here are far below 2^61 bytes
            w[15] = (u64)len * 8;
        }
        sha512_compress(st, w);
    }
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) out[i] = st[i];
}

// a digest (8 big-endian-valued words) as the 512-bit little-endian integer RFC 8032 reads it: limb j = digest bytes 4j .. 4j+3
SBV_HD void sc25519_digest_limbs(u32 x[16], const u64 h[8]) {
    SBV_UNROLL
    for (int j = 0; j < 16; ++j) {
        const u64 word = h[j >> 1];
        x[j] = bswap32((j & 1) ? (u32)word : (u32)(word >> 32));
    }
}
SBV_HD void sc25519_from_digest(u256& out, const u64 h[8]) {
    u32 x[16];
    sc25519_digest_limbs(x, h);
    mod_l_512(x, out.v);
}

// any 256-bit value mod L (a clamped secret scalar reaches 2^255 - 8; ed_add_sB wants less than 2^253)
SBV_HD void sc25519_reduce256(u256& out, const u256& a) {
    u32 x[16];
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) x[i] = i < 8 ? a.v[i] : 0u;
    mod_l_512(x, out.v);
}

// S = (k a + r) mod L for k, a, r < L (< 2^253)
//   p = k a        < L^2 < 2^506: 16 limbs hold it.  Row i adds k[i] * a (< 2^32 * 2^256) to the running limbs: every step is
//                  t = k[i] a[j] + p[i+j] + carry <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1, so t never overflows 64 bits and the
//                  carry stays below 2^32
//   t = p mod L    < L  (mod_l_512: three folds, its own bounds in sha512_dev.h)
//   s = t + r      < 2L < 2^254: no carry out of 256 bits
//   S = s - L if s >= L, else s: one conditional subtraction, S < L
SBV_HD void sc25519_muladd(u256& S, const u256& k, const u256& a, const u256& r) {
    u32 p[16];
    SBV_UNROLL
    for (int i = 0; i < 16; ++i) p[i] = 0;
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) {
        u64 carry = 0;
        SBV_UNROLL
        for (int j = 0; j < 8; ++j) {
            const u64 t = (u64)k.v[i] * a.v[j] + p[i + j] + carry;
            p[i + j] = (u32)t;
            carry = t >> 32;
        }
        p[i + 8] = (u32)carry;
    }
    u256 t, s, d;
    mod_l_512(p, t.v);
    (void)add256(s, t, r);
    const u32 borrow = sub256(d, s, ed_L());
    select256(S, borrow == 0, d, s);
}

// encode(P): the affine y, little-endian, with the sign (parity) of the affine x in bit 255 — what ed_encoding_matches compares
// against, written out.  One inversion by division steps, two multiplications, one freeze (a second inside fe25_is_negative).
SBV_HD void ed_encode(u32 out[8], const ept& P) {
    fe25 zi, x, y;
    fe25_inv_gcd(zi, P.Z);
    fe25_mul(x, P.X, zi);
    fe25_mul(y, P.Y, zi);
    u256 yw;
    fe25_freeze(yw, y);
    yw.v[7] |= (fe25_is_negative(x) ? 1u : 0u) << 31;
    SBV_UNROLL
    for (int j = 0; j < 8; ++j) out[j] = yw.v[j];
}

// encode([s]B) for s < 2^253 through the 16-bit comb of B
SBV_HD void ed_encode_sB(u32 out[8], const u256& s, const aniels* b16) {
    ept R;
    ed_set_ident(R);
    ed_add_sB(R, s, b16);
    ed_encode(out, R);
}

// seed (8 little-endian dwords) -> the expanded record: rec[0..8) = a mod L, rec[8..16) = prefix, rec[16..24) = A_enc
SBV_HD void ed_sign_expand_lane(const u32 seed[8], const aniels* b16, u32 rec[SBV_ED_SIGN_REC_WORDS]) {
    u64 st[8], w[16];
    sha512_iv(st);
    SBV_UNROLL
    for (int i = 0; i < 4; ++i) w[i] = ((u64)bswap32(seed[2 * i]) << 32) | bswap32(seed[2 * i + 1]);
    w[4] = 0x8000000000000000ULL;
    SBV_UNROLL
    for (int i = 5; i < 15; ++i) w[i] = 0;
    w[15] = 32 * 8;
    sha512_compress(st, w);
    u32 x[16];
    sc25519_digest_limbs(x, st);
    u256 a, am;
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) a.v[i] = x[i];
    a.v[0] &= 0xFFFFFFF8u;                           // the clamp of RFC 8032 §5.1.5
    a.v[7] = (a.v[7] & 0x7FFFFFFFu) | 0x40000000u;
    sc25519_reduce256(am, a);
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) { rec[i] = am.v[i]; rec[8 + i] = x[8 + i]; }
    ed_encode_sB(rec + 16, am, b16);
}

// One signature.  rec: the expanded record, read as dwords and, for the two hashes, as bytes (prefix = bytes 32..63, A_enc = bytes
// 64..95).  sig: the 16 dwords of R | S — MEMORY THE LANE OWNS, not a register array: R_enc is written there first and the challenge
// hash reads it back byte-wise through sha512_ram, which takes its three inputs as byte strings (on the device this keeps a byte-indexed
// private copy of R_enc, which would live in scratch, out of the kernel).
SBV_HD void ed_sign_lane(const u32* rec, const uint8_t* msg, size_t mlen, const aniels* b16, u32* sig) {
    const uint8_t* recb = reinterpret_cast<const uint8_t*>(rec);
    u64 h[8];
    u256 r, k, a, S;
    sha512_head_msg(recb + 32, 32, msg, mlen, h);                   // 1. r = H(prefix | M) mod L
    sc25519_from_digest(r, h);
    u32 renc[8];
    ed_encode_sB(renc, r, b16);                                     // 2, 3. R = [r]B, R_enc
    SBV_UNROLL
    for (int j = 0; j < 8; ++j) sig[j] = renc[j];
    sha512_ram(reinterpret_cast<const uint8_t*>(sig), recb + 64, msg, mlen, h);      // 4. k = H(R_enc | A_enc | M) mod L
    sc25519_from_digest(k, h);
    SBV_UNROLL
    for (int j = 0; j < 8; ++j) a.v[j] = rec[j];
    sc25519_muladd(S, k, a, r);                                     // 5. S = r + k a mod L
    SBV_UNROLL
    for (int j = 0; j < 8; ++j) sig[8 + j] = S.v[j];
}

}  // namespace sbv
