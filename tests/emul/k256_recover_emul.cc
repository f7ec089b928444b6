// k256_recover_emul.cc — CPU TEST TIER ONLY: the secp256k1 public-key recovery (consensus_amd/csrc/k256_recover.h,
// k256_recover_kernels.hip), lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them as the kernels do: k_k256_recover with its capped grid
// (lane L handles items L, L + lanes, ... on its own strip; `lanes` is a parameter here so that a small value reuses every strip many
// times) and the three unit operations of sbv_debug_secp256k1_recover_op.  The strips are allocated exactly, min(n, lanes) of them,
// so that a sanitizer build sees any access outside a lane's strip.  The 16-bit comb of G is the host builder's.  Not part of
// libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     k256_recover_emul CASES
// CASES holds one case per line, five hex fields separated by blanks: r | s, recid, digest, flags, Qx | Qy ("-" for a refused case:
// the lane must then answer zeros).  Every case is recovered twice, with 5 lanes and with more lanes than cases, and the unit
// operations run once over inputs made from the cases (op 1's point, walked by op 2 with u1 = 0 and u2 = 1, must come back).
// Exit status 0 = every byte matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_recover.h"

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

// k_k256_recover on a grid capped at `lanes` lanes
void sbvk256rec_recover(const uint8_t* sigs, const uint8_t* recid, const uint8_t* digests, size_t n, uint32_t flags, size_t lanes, uint8_t* pubs,
                        uint8_t* ok) {
    if (n == 0 || lanes == 0) return;
    const kapt* tab = gtab();
    const size_t active = std::min(n, lanes);
    u32* work = alloc_strips(active);
    parallel(active, [=](size_t L) {
        u32* strip = work + L * (size_t)SBV_K256_QTAB_WORDS;
        for (size_t i = L; i < n; i += lanes) {
            u32 rs[16], h[8], q[16];
            load_be(rs, sigs + 64 * i, 16);
            load_be(h, digests + 32 * i, 8);
            const bool good = k256_recover_lane(rs, recid[i], h, flags, strip, tab, q);
            store_be(pubs + 64 * i, q, 16);
            ok[i] = good ? 1 : 0;
        }
    });
    free(work);
}

// k_k256_recover_op: 192 bytes in, 128 bytes out per case
int sbvk256rec_op(int op, const uint8_t* in, uint8_t* out, size_t n) {
    if (op < 0 || op >= SBV_K256_RECOVER_OPS) return -1;
    if (n == 0) return 0;
    const kapt* tab = gtab();
    u32* work = alloc_strips(n);
    parallel(n, [=](size_t i) {
        u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
        load_be(a, in + 192 * i, SBV_K256_SIGN_OP_IN_WORDS);
        k256_recover_op_lane(op, a, work + i * (size_t)SBV_K256_QTAB_WORDS, tab, r);
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

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> sigs[2], rids[2], digs[2], pubs[2], want_ok[2];
    static char a[140], b[8], c[70], d[8], e[140];
    size_t line = 0;
    while (fscanf(f, "%139s %7s %69s %7s %139s", a, b, c, d, e) == 5) {
        std::vector<uint8_t> rs, rid, dig, fl, pub;
        if (!unhex(a, rs, 64) || !unhex(b, rid, 1) || !unhex(c, dig, 32) || !unhex(d, fl, 1) || fl[0] > 1 || !unhex(e, pub, 64)) {
            fprintf(stderr, "case %zu is malformed\n", line);
            return 2;
        }
        const int k = fl[0];
        sigs[k].insert(sigs[k].end(), rs.begin(), rs.end());
        rids[k].push_back(rid[0]);
        digs[k].insert(digs[k].end(), dig.begin(), dig.end());
        pubs[k].insert(pubs[k].end(), pub.begin(), pub.end());
        want_ok[k].push_back(strcmp(e, "-") != 0);
        ++line;
    }
    fclose(f);
    if (line == 0) { fprintf(stderr, "no cases\n"); return 2; }
    size_t bad = 0;
    for (uint32_t flags = 0; flags < 2; ++flags) {
        const size_t n = rids[flags].size();
        for (size_t lanes : {(size_t)5, n + 3}) {
            std::vector<uint8_t> gpub(64 * n, 0xA5), gok(n, 0xA5);
            sbvk256rec_recover(sigs[flags].data(), rids[flags].data(), digs[flags].data(), n, flags, lanes, gpub.data(), gok.data());
            for (size_t i = 0; i < n; ++i)
                if (gok[i] != want_ok[flags][i] || memcmp(&gpub[64 * i], &pubs[flags][64 * i], 64)) {
                    if (bad++ < 8) fprintf(stderr, "flags %u, case %zu, %zu lanes: the key differs\n", flags, i, lanes);
                }
        }
    }
    // the unit operations on the flags = 0 cases: op 0 on the digest, op 1 on r | recid, op 2 on op 1's point with u1 = 0, u2 = 1
    const size_t n = rids[0].size();
    std::vector<uint8_t> in(192 * n, 0), o0(128 * n), o1(128 * n), o2(128 * n);
    for (size_t i = 0; i < n; ++i) memcpy(&in[192 * i], &digs[0][32 * i], 32);
    sbvk256rec_op(0, in.data(), o0.data(), n);
    std::fill(in.begin(), in.end(), 0);
    for (size_t i = 0; i < n; ++i) { memcpy(&in[192 * i], &sigs[0][64 * i], 32); in[192 * i + 63] = rids[0][i]; }
    sbvk256rec_op(1, in.data(), o1.data(), n);
    std::fill(in.begin(), in.end(), 0);
    size_t lifted = 0;
    for (size_t i = 0; i < n; ++i) {
        if (o1[128 * i + 127] != 1) { memcpy(&in[192 * i], &o1[0], 64); in[192 * i + 127] = 1; continue; }      // any point
        memcpy(&in[192 * i], &o1[128 * i], 64);
        in[192 * i + 127] = 1;
        ++lifted;
    }
    if (o1[127] != 1) { fprintf(stderr, "the first case must have a point\n"); return 2; }
    sbvk256rec_op(2, in.data(), o2.data(), n);
    for (size_t i = 0; i < n; ++i)
        if (o2[128 * i + 127] != 1 || memcmp(&o2[128 * i], &in[192 * i], 64)) {
            if (bad++ < 8) fprintf(stderr, "case %zu: 1 * R' + 0 * G is not R'\n", i);
        }
    printf("%zu cases, %zu lifted, %zu differ\n", line, lifted, bad);
    free(const_cast<kapt*>(gtab()));
    return bad ? 1 : 0;
}
#endif
