// keccak256_dev.h — Keccak-256 (the original padding, as Ethereum uses it; FIPS 202's SHA3-256 differs only in the domain byte) as
// per-lane code: the permutation Keccak-f[1600], the sponge at rate 136, and the two fixed-size forms that follow a secp256k1 public-key
// recovery: the hash of a 64-byte key and the 20-byte address Keccak-256(Qx | Qy)[12:].
//
// One hash per lane, the whole state in the lane's registers: 25 lanes of 64 bits = 50 dwords.  Every state index below is a constant
// after unrolling (a state indexed at run time would go to scratch); only the round loop and the block loop stay loops (DESIGN.md
// "Keccak-256 and Ethereum addresses" has the instruction mix and why the 24 rounds are not unrolled).
//
// Digests are eight big-endian word values, out[0] = bytes 0..3 of the digest as a number, like sha256_dev.h and the records of
// k256_sign.h / k256_recover.h: a kernel stores bswap32(out[i]) and the bytes are on the wire.
//
// Shared host/device source (tests/emul/keccak_emul.cc compiles it with g++; consensus_amd/host/k256_host.cc builds the CPU forms).
#pragma once
#include "sbv_common.h"

#define SBV_KECCAK_RATE 136             // bytes per block at capacity 512
#define SBV_KECCAK_DOMAIN 0x01u         // Keccak-256; 0x06 is SHA3-256

namespace sbv {

// The three bit operations of a round, on the 32-bit halves a lane's registers hold.  On gfx950 the five-way xor of theta is two
// three-input operations and chi's a ^ (~b & c) is one (v_bitop3_b32: 0x96 = a ^ b ^ c, 0xd2 = a ^ (~b & c) for a = 0xf0, b = 0xcc, c = 0xaa);
// the compiler finds neither from the 64-bit expressions, so the device build names them.  A rotate by a constant is two funnel shifts
// (v_alignbit_b32), which it does find from the halves.
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
SBV_HD u32 keccak_xor3_32(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
SBV_HD u32 keccak_chi_32(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xd2); }
#else
SBV_HD u32 keccak_xor3_32(u32 a, u32 b, u32 c) { return a ^ b ^ c; }
SBV_HD u32 keccak_chi_32(u32 a, u32 b, u32 c) { return a ^ (~b & c); }
#endif
SBV_HD u64 keccak_join(u32 lo, u32 hi) { return (u64)lo | ((u64)hi << 32); }
SBV_HD u64 keccak_xor5(u64 a, u64 b, u64 c, u64 d, u64 e) {
    return keccak_join(keccak_xor3_32(keccak_xor3_32((u32)a, (u32)b, (u32)c), (u32)d, (u32)e),
                       keccak_xor3_32(keccak_xor3_32((u32)(a >> 32), (u32)(b >> 32), (u32)(c >> 32)), (u32)(d >> 32), (u32)(e >> 32)));
}
SBV_HD u64 keccak_chi(u64 a, u64 b, u64 c) {
    return keccak_join(keccak_chi_32((u32)a, (u32)b, (u32)c), keccak_chi_32((u32)(a >> 32), (u32)(b >> 32), (u32)(c >> 32)));
}
// n is a constant in 1..63 at every call
SBV_HD u64 keccak_rotl(u64 x, int n) {
    const u32 lo = n < 32 ? (u32)x : (u32)(x >> 32), hi = n < 32 ? (u32)(x >> 32) : (u32)x;
    const int m = n & 31;
    if (m == 0) return keccak_join(lo, hi);
    return keccak_join((lo << m) | (hi >> (32 - m)), (hi << m) | (lo >> (32 - m)));
}

// 24 rounds of theta, rho, pi, chi, iota on A[x + 5 y]
SBV_HD void keccak_f1600(u64 A[25]) {
    const u64 RC[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
        0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
        0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
        0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    SBV_NOUNROLL
    for (int round = 0; round < 24; ++round) {
        // theta: column parities, D[x] = C[x - 1] ^ rotl(C[x + 1], 1)
        const u64 C0 = keccak_xor5(A[0], A[5], A[10], A[15], A[20]);
        const u64 C1 = keccak_xor5(A[1], A[6], A[11], A[16], A[21]);
        const u64 C2 = keccak_xor5(A[2], A[7], A[12], A[17], A[22]);
        const u64 C3 = keccak_xor5(A[3], A[8], A[13], A[18], A[23]);
        const u64 C4 = keccak_xor5(A[4], A[9], A[14], A[19], A[24]);
        const u64 D0 = C4 ^ keccak_rotl(C1, 1);
        const u64 D1 = C0 ^ keccak_rotl(C2, 1);
        const u64 D2 = C1 ^ keccak_rotl(C3, 1);
        const u64 D3 = C2 ^ keccak_rotl(C4, 1);
        const u64 D4 = C3 ^ keccak_rotl(C0, 1);
        // rho and pi with theta's xor folded in: B[y + 5 (2 x + 3 y)] = rotl(A[x + 5 y] ^ D[x], rho[x][y]), written out lane by lane
        const u64 B0 = A[0] ^ D0;
        const u64 B1 = keccak_rotl(A[6] ^ D1, 44);
        const u64 B2 = keccak_rotl(A[12] ^ D2, 43);
        const u64 B3 = keccak_rotl(A[18] ^ D3, 21);
        const u64 B4 = keccak_rotl(A[24] ^ D4, 14);
        const u64 B5 = keccak_rotl(A[3] ^ D3, 28);
        const u64 B6 = keccak_rotl(A[9] ^ D4, 20);
        const u64 B7 = keccak_rotl(A[10] ^ D0, 3);
        const u64 B8 = keccak_rotl(A[16] ^ D1, 45);
        const u64 B9 = keccak_rotl(A[22] ^ D2, 61);
        const u64 B10 = keccak_rotl(A[1] ^ D1, 1);
        const u64 B11 = keccak_rotl(A[7] ^ D2, 6);
        const u64 B12 = keccak_rotl(A[13] ^ D3, 25);
        const u64 B13 = keccak_rotl(A[19] ^ D4, 8);
        const u64 B14 = keccak_rotl(A[20] ^ D0, 18);
        const u64 B15 = keccak_rotl(A[4] ^ D4, 27);
        const u64 B16 = keccak_rotl(A[5] ^ D0, 36);
        const u64 B17 = keccak_rotl(A[11] ^ D1, 10);
        const u64 B18 = keccak_rotl(A[17] ^ D2, 15);
        const u64 B19 = keccak_rotl(A[23] ^ D3, 56);
        const u64 B20 = keccak_rotl(A[2] ^ D2, 62);
        const u64 B21 = keccak_rotl(A[8] ^ D3, 55);
        const u64 B22 = keccak_rotl(A[14] ^ D4, 39);
        const u64 B23 = keccak_rotl(A[15] ^ D0, 41);
        const u64 B24 = keccak_rotl(A[21] ^ D1, 2);
        // chi row by row, iota on lane 0
        A[0] = keccak_chi(B0, B1, B2) ^ RC[round];
        A[1] = keccak_chi(B1, B2, B3);
        A[2] = keccak_chi(B2, B3, B4);
        A[3] = keccak_chi(B3, B4, B0);
        A[4] = keccak_chi(B4, B0, B1);
        A[5] = keccak_chi(B5, B6, B7);
        A[6] = keccak_chi(B6, B7, B8);
        A[7] = keccak_chi(B7, B8, B9);
        A[8] = keccak_chi(B8, B9, B5);
        A[9] = keccak_chi(B9, B5, B6);
        A[10] = keccak_chi(B10, B11, B12);
        A[11] = keccak_chi(B11, B12, B13);
        A[12] = keccak_chi(B12, B13, B14);
        A[13] = keccak_chi(B13, B14, B10);
        A[14] = keccak_chi(B14, B10, B11);
        A[15] = keccak_chi(B15, B16, B17);
        A[16] = keccak_chi(B16, B17, B18);
        A[17] = keccak_chi(B17, B18, B19);
        A[18] = keccak_chi(B18, B19, B15);
        A[19] = keccak_chi(B19, B15, B16);
        A[20] = keccak_chi(B20, B21, B22);
        A[21] = keccak_chi(B21, B22, B23);
        A[22] = keccak_chi(B22, B23, B24);
        A[23] = keccak_chi(B23, B24, B20);
        A[24] = keccak_chi(B24, B20, B21);
    }
}

// the first 32 bytes of the state as eight big-endian word values
SBV_HD void keccak_squeeze256(const u64 A[25], u32 out[8]) {
    SBV_UNROLL
    for (int i = 0; i < 4; ++i) {
        out[2 * i] = bswap32((u32)A[i]);
        out[2 * i + 1] = bswap32((u32)(A[i] >> 32));
    }
}

// The sponge with the domain byte as a parameter: rate 136, bytes into lanes little-endian, `domain` after the message and 0x80 into
// byte 135 of the last block (one byte takes both when len % 136 == 135).  Reads msg[0 .. len) byte by byte and nothing else, whatever
// the alignment of msg; msg may be null when len == 0.
SBV_HD void keccak_sponge256(const uint8_t* msg, size_t len, u32 domain, u32 out[8]) {
    u64 A[25];
    SBV_UNROLL
    for (int i = 0; i < 25; ++i) A[i] = 0;
    const size_t blocks = len / SBV_KECCAK_RATE + 1;            // the padding always finds room: a full last block adds one more
    SBV_NOUNROLL
    for (size_t blk = 0; blk < blocks; ++blk) {
        const size_t base = blk * SBV_KECCAK_RATE;
        if (base + SBV_KECCAK_RATE <= len) {                    // a whole block of message
            SBV_UNROLL
            for (int j = 0; j < SBV_KECCAK_RATE / 8; ++j) {
                const uint8_t* p = msg + base + (size_t)j * 8;
                u64 w = 0;
                SBV_UNROLL
                for (int k = 0; k < 8; ++k) w |= (u64)p[k] << (8 * k);
                A[j] ^= w;
            }
        } else {                                                // the last block: whole lanes, the lane the message ends in, zeros
            const size_t rem = len - base;                      // 0..135
            SBV_UNROLL
            for (int j = 0; j < SBV_KECCAK_RATE / 8; ++j) {
                const uint8_t* p = msg + base + (size_t)j * 8;
                u64 w = 0;
                if ((size_t)j * 8 + 8 <= rem) {
                    SBV_UNROLL
                    for (int k = 0; k < 8; ++k) w |= (u64)p[k] << (8 * k);
                } else if ((size_t)j * 8 <= rem) {              // 0..7 bytes of message, then the domain byte
                    const int t = (int)(rem - (size_t)j * 8);
                    SBV_NOUNROLL
                    for (int k = 0; k < t; ++k) w |= (u64)p[k] << (8 * k);
                    w |= (u64)domain << (8 * t);
                }
                A[j] ^= w;
            }
            A[SBV_KECCAK_RATE / 8 - 1] ^= 0x8000000000000000ull;
        }
        keccak_f1600(A);
    }
    keccak_squeeze256(A, out);
}

SBV_HD void keccak256(const uint8_t* msg, size_t len, u32 out[8]) { keccak_sponge256(msg, len, SBV_KECCAK_DOMAIN, out); }

// Keccak-256 of a 64-byte key given as the 16 big-endian words k256_recover_finish produces: one block, one permutation
SBV_HD void keccak256_64(const u32 q[16], u32 out[8]) {
    u64 A[25];
    SBV_UNROLL
    for (int i = 0; i < 8; ++i) A[i] = (u64)bswap32(q[2 * i]) | ((u64)bswap32(q[2 * i + 1]) << 32);
    SBV_UNROLL
    for (int i = 8; i < 25; ++i) A[i] = 0;
    A[8] = SBV_KECCAK_DOMAIN;                                    // byte 64
    A[16] = 0x8000000000000000ull;                              // byte 135
    keccak_f1600(A);
    keccak_squeeze256(A, out);
}

// the address of a key: the last 20 bytes of keccak256_64, as five big-endian word values
SBV_HD void k256_address(const u32 q[16], u32 addr[5]) {
    u32 h[8];
    keccak256_64(q, h);
    SBV_UNROLL
    for (int i = 0; i < 5; ++i) addr[i] = h[3 + i];
}

// ---- test only: one case of a unit operation (include/sbv.h: sbv_debug_keccak_op) ---------------------------------------------------
#define SBV_KECCAK_OPS 1
// op 0: one keccak_f1600 on a state of 25 little-endian lanes, as 50 dwords in memory order (dword 2 j = the low half of lane j)
SBV_HD void keccak_op_lane(int op, const u32 in[50], u32 out[50]) {
    (void)op;
    u64 A[25];
    SBV_UNROLL
    for (int i = 0; i < 25; ++i) A[i] = (u64)in[2 * i] | ((u64)in[2 * i + 1] << 32);
    keccak_f1600(A);
    SBV_UNROLL
    for (int i = 0; i < 25; ++i) { out[2 * i] = (u32)A[i]; out[2 * i + 1] = (u32)(A[i] >> 32); }
}

}  // namespace sbv
