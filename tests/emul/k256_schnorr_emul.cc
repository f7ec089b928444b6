// k256_schnorr_emul.cc — CPU TEST TIER ONLY: the BIP-340 Schnorr entries over secp256k1 (consensus_amd/csrc/k256_schnorr.h,
// k256_schnorr_kernels.hip), lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them as the kernels do: k_k256_schnorr_verify with its capped
// grid (lane L handles items L, L + lanes, ... on its own strip; `lanes` is a parameter here so that a small value reuses every strip
// many times), k_k256_schnorr_expand and k_k256_schnorr_sign with the signer's index rule and the null aux, the four unit operations
// of sbv_debug_secp256k1_schnorr_op, and op 2 of the recovery (the double-scalar walk).  The strips are allocated exactly, min(n,
// lanes) of them, so that a sanitizer build sees any access outside a lane's strip.  The 16-bit comb of G is the host builder's.  Not
// part of libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     k256_schnorr_emul CASES
// CASES holds one case per line, blank-separated hex fields:
//     V pk msg sig ok                  a verification case and its verdict (0 or 1)
//     S key msg aux record sig         a signing case: the private key, and the expected record and signature ("-": refused, zeros)
// Every V case is verified twice, with 5 lanes and with more lanes than cases; every S case is expanded and signed (with its aux, and
// the all-zero aux once more through the null pointer), and every produced signature is verified.  Exit status 0 = every byte matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_schnorr.h"

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

u32* alloc_strips(size_t count) { return (u32*)aligned_alloc(16, count * SBV_K256_QTAB_WORDS * sizeof(u32)); }

}  // namespace

extern "C" {

// k_k256_schnorr_verify on a grid capped at `lanes` lanes
void sbvk256sch_verify(const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs, size_t n, size_t lanes, uint8_t* ok) {
    if (n == 0 || lanes == 0) return;
    const kapt* tab = gtab();
    const size_t active = std::min(n, lanes);
    u32* work = alloc_strips(active);
    parallel(active, [=](size_t L) {
        u32* strip = work + L * (size_t)SBV_K256_QTAB_WORDS;
        for (size_t i = L; i < n; i += lanes) {
            u32 pk[8], m[8], rs[16];
            load_be(pk, pks + 32 * i, 8);
            load_be(m, msgs + 32 * i, 8);
            load_be(rs, sigs + 64 * i, 16);
            ok[i] = k256_schnorr_verify_lane(pk, m, rs, strip, tab) ? 1 : 0;
        }
    });
    free(work);
}

// k_k256_schnorr_expand; pks may be null
void sbvk256sch_expand(const uint8_t* keys, size_t m, uint8_t* expanded, uint8_t* pks, uint8_t* ok) {
    const kapt* tab = gtab();
    parallel(m, [=](size_t i) {
        u32 d[8], rec[16];
        load_be(d, keys + 32 * i, 8);
        const bool good = k256_schnorr_expand_lane(d, tab, rec);
        store_be(expanded + 64 * i, rec, 16);
        if (pks) store_be(pks + 32 * i, rec + 8, 8);
        ok[i] = good ? 1 : 0;
    });
}

// k_k256_schnorr_sign; key_index and aux may be null
void sbvk256sch_sign(const uint8_t* expanded, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs, const uint8_t* aux, size_t n,
                     uint8_t* sigs, uint8_t* ok) {
    const kapt* tab = gtab();
    parallel(n, [=](size_t i) {
        u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
        const bool known = kidx < n_keys;
        if (!known) kidx = 0;
        u32 rec[16], m[8], a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rs[16];
        load_be(rec, expanded + 64 * (size_t)kidx, 16);
        load_be(m, msgs + 32 * i, 8);
        if (aux) load_be(a, aux + 32 * i, 8);
        const bool good = k256_schnorr_sign_lane(rec, m, a, tab, rs) && known;
        if (!good) memset(rs, 0, sizeof rs);
        store_be(sigs + 64 * i, rs, 16);
        ok[i] = good ? 1 : 0;
    });
}

// k_k256_schnorr_op (recovery = 0) or k_k256_recover_op (recovery = 1): 192 bytes in, 128 bytes out per case
int sbvk256sch_op(int recovery, int op, const uint8_t* in, uint8_t* out, size_t n) {
    if (op < 0 || op >= (recovery ? SBV_K256_RECOVER_OPS : SBV_K256_SCHNORR_OPS)) return -1;
    if (n == 0) return 0;
    const kapt* tab = gtab();
    u32* work = alloc_strips(n);
    parallel(n, [=](size_t i) {
        u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
        load_be(a, in + 192 * i, SBV_K256_SIGN_OP_IN_WORDS);
        if (recovery) k256_recover_op_lane(op, a, work + i * (size_t)SBV_K256_QTAB_WORDS, tab, r);
        else k256_schnorr_op_lane(op, a, work + i * (size_t)SBV_K256_QTAB_WORDS, tab, r);
        store_be(out + 128 * i, r, SBV_K256_SIGN_OP_OUT_WORDS);
    });
    free(work);
    return 0;
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
static void append(std::vector<uint8_t>& dst, const std::vector<uint8_t>& src) { dst.insert(dst.end(), src.begin(), src.end()); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> vpk, vmsg, vsig, vok, skey, smsg, saux, srec, ssig, sok;
    static char k[4], a[140], b[140], c[140], d[140], e[140];
    size_t line = 0;
    while (fscanf(f, "%3s", k) == 1) {
        std::vector<uint8_t> x, y, z, u, v;
        if (!strcmp(k, "V")) {
            if (fscanf(f, "%139s %139s %139s %139s", a, b, c, d) != 4 || !unhex(a, x, 32) || !unhex(b, y, 32) || !unhex(c, z, 64) || !unhex(d, u, 1) ||
                u[0] > 1) {
                fprintf(stderr, "case %zu is malformed\n", line);
                return 2;
            }
            append(vpk, x); append(vmsg, y); append(vsig, z); vok.push_back(u[0]);
        } else if (!strcmp(k, "S")) {
            if (fscanf(f, "%139s %139s %139s %139s %139s", a, b, c, d, e) != 5 || !unhex(a, x, 32) || !unhex(b, y, 32) || !unhex(c, z, 32) ||
                !unhex(d, u, 64) || !unhex(e, v, 64)) {
                fprintf(stderr, "case %zu is malformed\n", line);
                return 2;
            }
            append(skey, x); append(smsg, y); append(saux, z); append(srec, u); append(ssig, v); sok.push_back(strcmp(e, "-") != 0);
        } else {
            fprintf(stderr, "case %zu is malformed\n", line);
            return 2;
        }
        ++line;
    }
    fclose(f);
    if (vok.empty() || sok.empty()) { fprintf(stderr, "no cases\n"); return 2; }
    size_t bad = 0;
    const size_t n = vok.size(), m = sok.size();
    for (size_t lanes : {(size_t)5, n + 3}) {
        std::vector<uint8_t> got(n, 0xA5);
        sbvk256sch_verify(vpk.data(), vmsg.data(), vsig.data(), n, lanes, got.data());
        for (size_t i = 0; i < n; ++i)
            if (got[i] != vok[i] && bad++ < 8) fprintf(stderr, "verify case %zu, %zu lanes: the verdict differs\n", i, lanes);
    }
    std::vector<uint8_t> rec(64 * m, 0xA5), pk(32 * m, 0xA5), eok(m, 0xA5), sig(64 * m, 0xA5), gok(m, 0xA5), sig0(64 * m), sig1(64 * m), zero(32 * m, 0);
    sbvk256sch_expand(skey.data(), m, rec.data(), pk.data(), eok.data());
    sbvk256sch_sign(rec.data(), (uint32_t)m, nullptr, smsg.data(), saux.data(), m, sig.data(), gok.data());
    for (size_t i = 0; i < m; ++i) {
        if ((memcmp(&rec[64 * i], &srec[64 * i], 64) || memcmp(&pk[32 * i], &srec[64 * i + 32], 32) || eok[i] != sok[i]) && bad++ < 8)
            fprintf(stderr, "sign case %zu: the record differs\n", i);
        if ((memcmp(&sig[64 * i], &ssig[64 * i], 64) || gok[i] != sok[i]) && bad++ < 8) fprintf(stderr, "sign case %zu: the signature differs\n", i);
    }
    // aux = NULL is 32 zero bytes
    sbvk256sch_sign(rec.data(), (uint32_t)m, nullptr, smsg.data(), nullptr, m, sig0.data(), gok.data());
    sbvk256sch_sign(rec.data(), (uint32_t)m, nullptr, smsg.data(), zero.data(), m, sig1.data(), gok.data());
    if (sig0 != sig1) { ++bad; fprintf(stderr, "a null aux is not the zero aux\n"); }
    // every produced signature verifies under its key, on 3 lanes
    std::vector<uint8_t> back(m, 0xA5);
    sbvk256sch_verify(pk.data(), smsg.data(), sig.data(), m, 3, back.data());
    for (size_t i = 0; i < m; ++i)
        if (back[i] != sok[i] && bad++ < 8) fprintf(stderr, "sign case %zu: the signature does not verify\n", i);
    printf("%zu cases, %zu verify, %zu sign, %zu differ\n", line, n, m, bad);
    free(const_cast<kapt*>(gtab()));
    return bad ? 1 : 0;
}
#endif
