// ecdsa_sign_msgs_emul.cc — CPU TEST TIER ONLY: the lanes of the raw-message ECDSA signers (consensus_amd/csrc/ecdsa_sign_msgs.h,
// ecdsa_sign_msgs_kernels.hip), lane by lane, with the contract assertions of the header turned on.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them as the kernels do: k_sha256_msgs (the slice check and
// either loader), the signing lane of each curve as k_p256_sign / k_k256_sign run it, and k_ecdsa_sig_finish.  The combs of G are the
// host builders' (P-256: an 8-bit comb, the signature does not depend on the width; secp256k1: the 16-bit comb).  Not part of
// libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     ecdsa_sign_msgs_emul CASES
// CASES holds one case per line:
//     H <message hex or -> <digest hex>                      both loaders, the message in a heap block of exactly its length, and copies
//                                                            at offsets 1, 2 and 3 of a block of len + offset bytes
//     D <curve> <flags> <r|s hex> <record hex> <recid in> <recid out>     k_ecdsa_sig_finish's lane: the record must be the one given, zero
//                                                            behind it, and parse back (der_parse_sig) to the r | s it encodes
// Exit status 0 = every byte matched.  The program builds no comb and signs nothing.
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#define SBV_ECDSA_CONTRACT(cond) assert(cond)
#include "../../consensus_amd/csrc/ecdsa_sign_msgs.h"
#ifndef SBV_EMUL_MAIN
#include "../../consensus_amd/csrc/p256_core.h"
#include "../../consensus_amd/csrc/p256_sign.h"
#include "../../consensus_amd/csrc/k256_sign.h"
#endif

using namespace sbv;

namespace {

void load_mem(u32* w, const uint8_t* b, int words) { memcpy(w, b, 4 * (size_t)words); }      // a kernel's dword loads: memory order
void load_be(u32* w, const uint8_t* b, int words) {
    for (int k = 0; k < words; ++k) w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
void store_be(uint8_t* b, const u32* w, int words) {
    for (int k = 0; k < words; ++k) { b[4 * k] = (uint8_t)(w[k] >> 24); b[4 * k + 1] = (uint8_t)(w[k] >> 16); b[4 * k + 2] = (uint8_t)(w[k] >> 8); b[4 * k + 3] = (uint8_t)w[k]; }
}

}  // namespace

extern "C" {

// sha256_msg_words (words != 0) or sha256_msg on one message where it lies; out: the 32 digest bytes
void sbvesm_sha256(int words, const uint8_t* msg, size_t len, uint8_t out[32]) {
    u32 h[8];
    if (words) sha256_msg_words(msg, len, h);
    else sha256_msg(msg, len, h);
    store_be(out, h, 8);
}

// k_sha256_msgs over a packed batch
void sbvesm_sha256_msgs(const uint8_t* msgs, const uint64_t* moff, size_t n, uint64_t mbytes, int words, uint8_t* digests) {
    for (size_t i = 0; i < n; ++i) {
        u32 h[8];
        (void)sha256_msgs_lane(msgs, moff[i], moff[i + 1], mbytes, words != 0, h);
        memcpy(digests + 32 * i, h, 32);
    }
}

// ecdsa_low_s on a big-endian s: 1 when negated
int sbvesm_low_s(int curve, uint8_t s_be[32]) {
    u256 s;
    from_be32(s, s_be);
    const bool neg = ecdsa_low_s(curve, s);
    u32 w[8];
    for (int i = 0; i < 8; ++i) w[i] = s.v[7 - i];
    store_be(s_be, w, 8);
    return neg ? 1 : 0;
}

// k_ecdsa_sig_finish's lane: rs as the signer stores it, record as the kernel stores it.  recid in / out.
void sbvesm_finish(int curve, const uint8_t rs[64], int ok, int low_s, uint8_t record[72], uint8_t* len, uint8_t* recid) {
    u32 in[16], rec[SBV_ECDSA_DER_WORDS], l, rid = *recid;
    load_mem(in, rs, 16);
    ecdsa_sig_finish_lane(curve, in, ok != 0, low_s != 0, rec, l, rid);
    memcpy(record, rec, 72);
    *len = (uint8_t)l;
    *recid = (uint8_t)rid;
}

// the device parser on the bytes of a record: 1 and r | s, or 0
int sbvesm_der_parse(const uint8_t* der, size_t len, uint8_t rs[64]) {
    u32 r[8], s[8];
    const bool good = der_parse_sig(der, len, r, s);
    store_be(rs, r, 8);
    store_be(rs + 32, s, 8);
    return good ? 1 : 0;
}

// msg_frontend_tuple_lane: what k_msg_frontend_tuples makes of (message, DER signature, key)
void sbvesm_frontend_tuple(const uint8_t* msg, size_t mlen, const uint8_t* der, size_t dlen, const uint8_t key[64], uint8_t tuple[160]) {
    u32 k[16], t[40];
    load_mem(k, key, 16);
    msg_frontend_tuple_lane(msg, mlen, der, dlen, k, t);
    memcpy(tuple, t, 160);
}

#ifndef SBV_EMUL_MAIN
static gcomb p256_comb() {
    static apt* tab = nullptr;
    const int bits = 8;
    if (!tab) {
        const size_t count = gcomb_entries(bits);
        apt* tmp = (apt*)aligned_alloc(64, sizeof(apt) * count);
        tab = (apt*)aligned_alloc(64, sizeof(apt) * count);
        for (int j = 0; j < (257 + bits - 1) / bits; ++j) build_gcomb_window(bits, j, tmp + ((size_t)j << (bits - 1)));
        for (size_t k = 0; k < count; ++k) apt_to_r261(tab[k], tmp[k]);
        free(tmp);
    }
    return gcomb_make(tab, bits);
}
static const kapt* k256_comb() {
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

// the secp256k1 signing lane alone, under its own flag: 1 and r | s, recid
int sbvesm_k256_sign(const uint8_t d_be[32], const uint8_t digest[32], uint32_t flags, uint8_t rs[64], uint8_t* recid) {
    u32 d[8], h[8], w[16], rid;
    load_be(d, d_be, 8);
    load_be(h, digest, 8);
    const bool good = k256_sign_lane(d, h, k256_comb(), flags, w, rid);
    store_be(rs, w, 16);
    *recid = (uint8_t)rid;
    return good ? 1 : 0;
}

// The three kernels of one call, as enqueue_sign_msgs (sbv_api.hip) launches them: k_sha256_msgs into the workspace, the curve's signing
// kernel, k_ecdsa_sig_finish; the refusal marks of the first travel to the last in lens.  curve 0 = P-256, 1 = secp256k1.  recid may be null.
void sbvesm_sign_msgs(int curve, const uint8_t* keys, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs, const uint64_t* moff,
                      uint64_t mbytes, size_t n, uint32_t flags, int words, uint8_t* records, uint8_t* lens, uint8_t* recid, uint8_t* ok) {
    const gcomb gc = p256_comb();
    const kapt* kt = k256_comb();
    std::vector<uint8_t> work(96 * n);
    uint8_t* dig = work.data();
    uint8_t* rs = work.data() + 32 * n;
    for (size_t i = 0; i < n; ++i) {                 // k_sha256_msgs with a mark array: the call's length array
        u32 h[8];
        lens[i] = sha256_msgs_lane(msgs, moff[i], moff[i + 1], mbytes, words != 0, h) ? 0 : 1;
        memcpy(dig + 32 * i, h, 32);
    }
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([=] {
            for (size_t i = t; i < n; i += nt) {
                u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
                const bool known = kidx < n_keys;
                if (!known) kidx = 0;
                u32 d[8], h[8], w[16], rid = 0;
                load_be(d, keys + 32 * (size_t)kidx, 8);
                load_be(h, dig + 32 * i, 8);
                const bool good = (curve == SBV_ECDSA_CURVE_P256 ? sign29_lane(d, h, gc, w) : k256_sign_lane(d, h, kt, flags, w, rid)) && known;
                if (!good) memset(w, 0, sizeof w);
                store_be(rs + 64 * i, w, 16);
                if (recid) recid[i] = good ? (uint8_t)rid : 0;
                ok[i] = good ? 1 : 0;
            }
        });
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n; ++i) {
        const bool good = ok[i] != 0 && lens[i] == 0;          // k_ecdsa_sig_finish reads the mark before it stores the length
        uint8_t rid = recid ? recid[i] : 0;
        sbvesm_finish(curve, rs + 64 * i, good, curve == SBV_ECDSA_CURVE_P256 && (flags & 1u), records + 72 * i, lens + i, &rid);
        if (recid) recid[i] = rid;
        ok[i] = good ? 1 : 0;
    }
}
#endif

}  // extern "C"

#ifdef SBV_EMUL_MAIN
static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    out.clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
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
    static char kind[4], a[16384], b[16384], c[256], d[256], e[16], g[16];
    size_t hashes = 0, ders = 0, bad = 0;
    while (fscanf(f, "%3s", kind) == 1) {
        if (kind[0] == 'H') {
            if (fscanf(f, "%16383s %16383s", a, b) != 2) return 2;
            std::vector<uint8_t> msg, want;
            if (!unhex(a, msg) || !unhex(b, want) || want.size() != 32) { fprintf(stderr, "malformed hash case\n"); return 2; }
            for (size_t off = 0; off < 4; ++off) {
                // malloc returns blocks aligned to 16: the message starts at address = off mod 4 and ends with the block
                uint8_t* block = (uint8_t*)malloc(msg.size() + off ? msg.size() + off : 1);
                if (!msg.empty()) memcpy(block + off, msg.data(), msg.size());
                for (int words = 0; words < 2; ++words) {
                    uint8_t got[32];
                    sbvesm_sha256(words, msg.empty() && off == 0 ? nullptr : block + off, msg.size(), got);
                    if (memcmp(got, want.data(), 32)) { if (bad++ < 8) fprintf(stderr, "hash of %zu bytes at offset %zu, loader %d differs\n", msg.size(), off, words); }
                }
                // and through the kernel's lane, as a slice of a packed batch
                const uint64_t moff[2] = {off, off + msg.size()};
                uint8_t got[32];
                sbvesm_sha256_msgs(block, moff, 1, off + msg.size(), 1, got);
                if (memcmp(got, want.data(), 32)) { if (bad++ < 8) fprintf(stderr, "lane hash of %zu bytes at offset %zu differs\n", msg.size(), off); }
                free(block);
            }
            ++hashes;
        } else if (kind[0] == 'D') {
            int curve, flags, rid_in, rid_out;
            if (fscanf(f, "%d %d %255s %255s %d %d", &curve, &flags, c, d, &rid_in, &rid_out) != 6) return 2;
            (void)e; (void)g;
            std::vector<uint8_t> rs, want;
            if (!unhex(c, rs) || !unhex(d, want) || rs.size() != 64 || want.size() > 72) { fprintf(stderr, "malformed DER case\n"); return 2; }
            uint8_t* in = (uint8_t*)malloc(64);
            uint8_t* rec = (uint8_t*)malloc(72);
            memcpy(in, rs.data(), 64);
            uint8_t len = 0, rid = (uint8_t)rid_in, back[64];
            sbvesm_finish(curve, in, 1, flags & 1, rec, &len, &rid);
            bool good = len == want.size() && !memcmp(rec, want.data(), len) && rid == rid_out;
            for (size_t k = len; k < 72; ++k) good = good && rec[k] == 0;
            uint8_t* exact = (uint8_t*)malloc(len ? len : 1);
            memcpy(exact, rec, len);
            good = good && sbvesm_der_parse(exact, len, back) == 1;
            if (!good) { if (bad++ < 8) fprintf(stderr, "DER case %zu differs\n", ders); }
            sbvesm_finish(curve, in, 0, flags & 1, rec, &len, &rid);
            for (size_t k = 0; k < 72; ++k) good = good && rec[k] == 0;
            if (len != 0 || rid != 0) { if (bad++ < 8) fprintf(stderr, "DER case %zu: a refused lane is not empty\n", ders); }
            free(exact); free(rec); free(in);
            ++ders;
        } else {
            fprintf(stderr, "unknown case kind %s\n", kind);
            return 2;
        }
    }
    fclose(f);
    printf("%zu hash cases, %zu DER cases, %zu mismatches\n", hashes, ders, bad);
    return bad || hashes + ders == 0 ? 1 : 0;
}
#endif
