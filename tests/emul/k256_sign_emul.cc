// k256_sign_emul.cc — CPU TEST TIER ONLY: the secp256k1 batch signer (consensus_amd/csrc/k256_sign.h, k256_sign_kernels.hip), lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them as the kernels do: k_k256_sign (key selection, the
// rejected lanes, k256_sign_lane), k_k256_pubkeys, the four unit operations of sbv_debug_secp256k1_sign_op, and k256_sign_with_nonce
// on its own.  The 16-bit comb of G is the host builder's (k256_build_g_window: 17 x 32768 entries, 36 MB, a fraction of a second on
// 17 threads).  Not part of libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     k256_sign_emul CASES
// CASES holds one case per line, seven hex fields separated by blanks: private key, digest, r | s and recid with flags = 0, r | s and
// recid with SBV_K256_SIGN_LOW_S, public key ("-" for sig and public key when the key is rejected: the lane must then answer zeros).
// Every case is signed under both flag settings and its public key derived, and the four unit operations run once over inputs made
// from the cases (ops 0 and 2 are compared with the signature's r; ops 1 and 3 run for the sanitizers' sake).
// Exit status 0 = every byte matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_sign.h"

using namespace sbv;

namespace {

const kapt* gtab() {
    static kapt* tab = nullptr;
    if (!tab) {
        tab = (kapt*)aligned_alloc(64, sizeof(kapt) * SBV_K256_G_ENTRIES);
        std::vector<std::thread> th;
        for (int j = 0; j < SBV_K256_G_WINDOWS; ++j)
            th.emplace_back([j] { k256_build_g_window(j, tab + (size_t)j * SBV_K256_G_PER_WINDOW, SBV_K256_G_PER_WINDOW); });
        for (auto& t : th) t.join();
    }
    return tab;
}

template <class F>
void parallel(size_t n, F f) {
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(32u, std::thread::hardware_concurrency()), n));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([=] { for (size_t i = t; i < n; i += nt) f(i); });
    for (auto& t : th) t.join();
}

// the kernels' loads and stores: big-endian bytes <-> words
void load_be(u32* w, const uint8_t* b, int words) {
    for (int k = 0; k < words; ++k) w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
void store_be(uint8_t* b, const u32* w, int words) {
    for (int k = 0; k < words; ++k) { b[4 * k] = (uint8_t)(w[k] >> 24); b[4 * k + 1] = (uint8_t)(w[k] >> 16); b[4 * k + 2] = (uint8_t)(w[k] >> 8); b[4 * k + 3] = (uint8_t)w[k]; }
}

}  // namespace

extern "C" {

// k_k256_sign
void sbvk256sign_sign(const uint8_t* keys, uint32_t n_keys, const uint32_t* key_index, const uint8_t* digests, size_t n, uint32_t flags,
                      uint8_t* sigs, uint8_t* recid, uint8_t* ok) {
    const kapt* tab = gtab();
    parallel(n, [=](size_t i) {
        u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
        const bool known = kidx < n_keys;
        if (!known) kidx = 0;
        u32 d[8], h[8], rs[16], rid;
        load_be(d, keys + 32 * (size_t)kidx, 8);
        load_be(h, digests + 32 * i, 8);
        const bool good = k256_sign_lane(d, h, tab, flags, rs, rid) && known;
        if (!good) memset(rs, 0, sizeof rs);
        store_be(sigs + 64 * i, rs, 16);
        if (recid) recid[i] = good ? (uint8_t)rid : 0;
        ok[i] = good ? 1 : 0;
    });
}

// k_k256_pubkeys
void sbvk256sign_pubkeys(const uint8_t* keys, size_t m, uint8_t* pubs, uint8_t* ok) {
    const kapt* tab = gtab();
    parallel(m, [=](size_t i) {
        u32 d[8], q[16];
        load_be(d, keys + 32 * i, 8);
        ok[i] = k256_pubkey_lane(d, tab, q) ? 1 : 0;
        store_be(pubs + 64 * i, q, 16);
    });
}

// k_k256_sign_op: 192 bytes in, 128 bytes out per case
int sbvk256sign_op(int op, const uint8_t* in, uint8_t* out, size_t n) {
    if (op < 0 || op >= SBV_K256_SIGN_OPS) return -1;
    const kapt* tab = gtab();
    parallel(n, [=](size_t i) {
        u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
        load_be(a, in + 192 * i, SBV_K256_SIGN_OP_IN_WORDS);
        k256_sign_op_lane(op, a, tab, r);
        store_be(out + 128 * i, r, SBV_K256_SIGN_OP_OUT_WORDS);
    });
    return 0;
}

// k256_sign_with_nonce on big-endian d, k, e (d in [1, n - 1], e < n): 1 and r | s, recid, or 0 and nothing written
int sbvk256sign_with_nonce(const uint8_t d_be[32], const uint8_t k_be[32], const uint8_t e_be[32], uint32_t flags, uint8_t rs[64], uint8_t* recid) {
    u256 d, k, e, r, s;
    u32 rid = 0, w[16];
    from_be32(d, d_be); from_be32(k, k_be); from_be32(e, e_be);
    if (!k256_sign_with_nonce(d, k, e, gtab(), flags, r, s, rid)) return 0;
    u256_to_be_words(w, r);
    u256_to_be_words(w + 8, s);
    store_be(rs, w, 16);
    *recid = (uint8_t)rid;
    return 1;
}

}  // extern "C"

#ifdef SBV_EMUL_MAIN
static bool unhex(const std::string& s, std::vector<uint8_t>& out, size_t want) {
    out.clear();
    if (s == "-") { out.assign(want, 0); return true; }
    if (s.size() != 2 * want) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        unsigned v;
        if (sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
        out.push_back((uint8_t)v);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> keys, digs, sig[2], rid[2], pubs, want_ok;
    static char a[70], b[70], c[140], d[8], e[140], g[8], h[140];
    size_t n = 0;
    while (fscanf(f, "%69s %69s %139s %7s %139s %7s %139s", a, b, c, d, e, g, h) == 7) {
        std::vector<uint8_t> key, dig, s0, r0, s1, r1, pub;
        if (!unhex(a, key, 32) || !unhex(b, dig, 32) || !unhex(c, s0, 64) || !unhex(d, r0, 1) || !unhex(e, s1, 64) || !unhex(g, r1, 1) || !unhex(h, pub, 64)) {
            fprintf(stderr, "case %zu is malformed\n", n);
            return 2;
        }
        keys.insert(keys.end(), key.begin(), key.end());
        digs.insert(digs.end(), dig.begin(), dig.end());
        sig[0].insert(sig[0].end(), s0.begin(), s0.end());
        sig[1].insert(sig[1].end(), s1.begin(), s1.end());
        rid[0].push_back(r0[0]);
        rid[1].push_back(r1[0]);
        pubs.insert(pubs.end(), pub.begin(), pub.end());
        want_ok.push_back(strcmp(c, "-") != 0);
        ++n;
    }
    fclose(f);
    if (n == 0) { fprintf(stderr, "no cases\n"); return 2; }
    size_t bad = 0;
    std::vector<uint8_t> gsig(64 * n), grid(n), gok(n), gpub(64 * n);
    for (uint32_t flags = 0; flags < 2; ++flags) {                 // case i signs with key i
        sbvk256sign_sign(keys.data(), (uint32_t)n, nullptr, digs.data(), n, flags, gsig.data(), grid.data(), gok.data());
        for (size_t i = 0; i < n; ++i)
            if (gok[i] != want_ok[i] || grid[i] != rid[flags][i] || memcmp(&gsig[64 * i], &sig[flags][64 * i], 64)) {
                if (bad++ < 8) fprintf(stderr, "case %zu, flags %u: the signature differs\n", i, flags);
            }
    }
    sbvk256sign_pubkeys(keys.data(), n, gpub.data(), gok.data());
    for (size_t i = 0; i < n; ++i)
        if (gok[i] != want_ok[i] || memcmp(&gpub[64 * i], &pubs[64 * i], 64)) {
            if (bad++ < 8) fprintf(stderr, "case %zu: the public key differs\n", i);
        }
    // the unit operations: op 0 on d | digest, op 1 on the state op 0 returns, op 2 on op 0's k (its x mod n is r: these r are below
    // n), op 3 on digest-derived integers
    std::vector<uint8_t> in(192 * n), o0(128 * n), o1(128 * n), o2(128 * n), o3(128 * n);
    for (size_t i = 0; i < n; ++i) { memcpy(&in[192 * i], &keys[32 * i], 32); memcpy(&in[192 * i + 32], &digs[32 * i], 32); }
    sbvk256sign_op(0, in.data(), o0.data(), n);
    std::fill(in.begin(), in.end(), 0);
    for (size_t i = 0; i < n; ++i) memcpy(&in[192 * i], &o0[128 * i + 32], 64);
    sbvk256sign_op(1, in.data(), o1.data(), n);
    std::fill(in.begin(), in.end(), 0);
    for (size_t i = 0; i < n; ++i) memcpy(&in[192 * i], &o0[128 * i], 32);
    sbvk256sign_op(2, in.data(), o2.data(), n);
    for (size_t i = 0; i < n; ++i)
        if (want_ok[i] && (o0[128 * i + 127] != 1 || o2[128 * i + 127] != 1 || memcmp(&o2[128 * i], &sig[0][64 * i], 32))) {
            if (bad++ < 8) fprintf(stderr, "case %zu: the x of op 0's nonce times G is not r\n", i);
        }
    std::fill(in.begin(), in.end(), 0);
    for (size_t i = 0; i < n; ++i) {
        uint8_t* r = &in[192 * i];
        memcpy(r, &digs[32 * i], 32);                              // x
        r[63] = (uint8_t)(i & 1);                                  // y_odd
        memcpy(r + 64, &keys[32 * i], 32);                         // d
        memcpy(r + 96, &o0[128 * i], 32);                          // k
        memcpy(r + 128, &sig[0][64 * i], 32);                      // e: any integer below n
        r[191] = (uint8_t)((i >> 1) & 1);                          // flags
    }
    sbvk256sign_op(3, in.data(), o3.data(), n);
    printf("%zu cases, %zu differ\n", n, bad);
    free(const_cast<kapt*>(gtab()));
    return bad ? 1 : 0;
}
#endif
