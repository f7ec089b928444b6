// keccak_emul.cc — CPU TEST TIER ONLY: Keccak-256 and the address kernels (consensus_amd/csrc/keccak256_dev.h, keccak_kernels.hip),
// lane by lane.
//
// Compiles the lane code the gfx950 kernels are built from with g++ and runs it as the kernels do: one message per lane from an offset
// table, one key per lane, the fused recovery lane on a grid capped at `lanes` lanes (lane L handles items L, L + lanes, ... on its own
// strip), and the unit operation of sbv_debug_keccak_op.  Every message is hashed from a heap buffer of exactly its length (no buffer
// at all for an empty one), addresses go into n x 20 bytes exactly and strips are allocated exactly, so that a sanitizer build sees any
// byte read outside msg[0 .. len), a sixth dword of an address and any access outside a lane's strip.  Not part of libsbv.so, never
// shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     keccak_emul CASES
// CASES holds one case per line, a letter and hex fields separated by blanks ("-" is the empty string, or zeros where a size is fixed):
//     M domain message digest          the sponge under the domain byte
//     S state state'                   one Keccak-f[1600] on 200 bytes
//     K key digest address             keccak256_64 and k256_address of 64 bytes
//     R r|s recid digest flags address the fused recovery lane ("-": a refused case, the lane must answer 20 zero bytes and ok = 0)
// The recovery cases run with 5 lanes and with more lanes than cases.  Exit status 0 = every byte matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_recover.h"
#include "../../consensus_amd/csrc/keccak256_dev.h"

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

// k_keccak256_msgs under any domain byte: a decreasing offset pair writes zeros and reads nothing
void sbvkk_msgs(const uint8_t* msgs, const uint64_t* moff, size_t n, uint32_t domain, uint8_t* digests) {
    parallel(n, [=](size_t i) {
        u32 h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint64_t m0 = moff[i], m1 = moff[i + 1];
        if (m1 >= m0) {
            const size_t len = (size_t)(m1 - m0);
            uint8_t* own = len ? (uint8_t*)malloc(len) : nullptr;           // exactly the message: a read past it is a finding
            if (len) memcpy(own, msgs + m0, len);
            keccak_sponge256(own, len, domain, h);
            free(own);
        }
        store_be(digests + 32 * i, h, 8);
    });
}

// k_keccak_op: 200 bytes in, 200 bytes out per case
int sbvkk_op(int op, const uint8_t* in, uint8_t* out, size_t n) {
    if (op < 0 || op >= SBV_KECCAK_OPS) return -1;
    parallel(n, [=](size_t i) {
        u32 a[50], r[50];
        memcpy(a, in + 200 * i, 200);                                       // the kernel's plain dword loads (little-endian host)
        keccak_op_lane(op, a, r);
        memcpy(out + 200 * i, r, 200);
    });
    return 0;
}

// keccak256_64 on its own: pubs n x 64 -> digests n x 32
void sbvkk_hash64(const uint8_t* pubs, size_t n, uint8_t* digests) {
    parallel(n, [=](size_t i) {
        u32 q[16], h[8];
        load_be(q, pubs + 64 * i, 16);
        keccak256_64(q, h);
        store_be(digests + 32 * i, h, 8);
    });
}

// k_k256_addresses: pubs n x 64 -> addrs n x 20, five dwords per lane
void sbvkk_addresses(const uint8_t* pubs, size_t n, uint8_t* addrs) {
    parallel(n, [=](size_t i) {
        u32 q[16], a[5];
        load_be(q, pubs + 64 * i, 16);
        k256_address(q, a);
        store_be(addrs + 20 * i, a, 5);
    });
}

// k_k256_recover_addr on a grid capped at `lanes` lanes
void sbvkk_recover_addr(const uint8_t* sigs, const uint8_t* recid, const uint8_t* digests, size_t n, uint32_t flags, size_t lanes, uint8_t* addrs,
                        uint8_t* ok) {
    if (n == 0 || lanes == 0) return;
    const kapt* tab = gtab();
    const size_t active = std::min(n, lanes);
    u32* work = (u32*)aligned_alloc(16, active * SBV_K256_QTAB_WORDS * sizeof(u32));
    parallel(active, [=](size_t L) {
        u32* strip = work + L * (size_t)SBV_K256_QTAB_WORDS;
        for (size_t i = L; i < n; i += lanes) {
            u32 rs[16], h[8], q[16], a[5];
            load_be(rs, sigs + 64 * i, 16);
            load_be(h, digests + 32 * i, 8);
            const bool good = k256_recover_lane(rs, recid[i], h, flags, strip, tab, q);
            k256_address(q, a);
            for (int k = 0; k < 5; ++k) a[k] = good ? a[k] : 0u;
            store_be(addrs + 20 * i, a, 5);
            ok[i] = good ? 1 : 0;
        }
    });
    free(work);
}

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
    size_t lines = 0, bad = 0;
    std::vector<uint8_t> sigs[2], rids[2], digs[2], addrs[2], want_ok[2];
    static char buf[4096];
    while (fgets(buf, sizeof buf, f)) {
        std::vector<std::string> tok;
        for (char* p = strtok(buf, " \n"); p; p = strtok(nullptr, " \n")) tok.push_back(p);
        if (tok.empty()) continue;
        std::vector<std::vector<uint8_t>> v(tok.size());
        bool fine = tok[0].size() == 1;
        for (size_t k = 1; fine && k < tok.size(); ++k) fine = unhex(tok[k], v[k]);
        const char kind = tok[0][0];
        if (fine && kind == 'M' && tok.size() == 4 && v[1].size() == 1 && v[3].size() == 32) {
            // through the kernel's form: the message alone in a heap buffer of its own length, the offsets 0 and len
            std::vector<uint8_t> got(32, 0xA5);
            const uint64_t moff[2] = {0, v[2].size()};
            uint8_t* own = v[2].empty() ? nullptr : (uint8_t*)malloc(v[2].size());
            if (own) memcpy(own, v[2].data(), v[2].size());
            sbvkk_msgs(own, moff, 1, v[1][0], got.data());
            free(own);
            if (got != v[3] && bad++ < 8) fprintf(stderr, "line %zu: the digest of a %zu-byte message differs\n", lines, v[2].size());
        } else if (fine && kind == 'S' && tok.size() == 3 && v[1].size() == 200 && v[2].size() == 200) {
            std::vector<uint8_t> got(200, 0xA5);
            if ((sbvkk_op(0, v[1].data(), got.data(), 1) != 0 || got != v[2]) && bad++ < 8) fprintf(stderr, "line %zu: the state differs\n", lines);
        } else if (fine && kind == 'K' && tok.size() == 4 && v[1].size() == 64 && v[2].size() == 32 && v[3].size() == 20) {
            uint8_t* d = (uint8_t*)malloc(32);
            uint8_t* a = (uint8_t*)malloc(20);                              // exactly 20 bytes: a sixth dword is a finding
            sbvkk_hash64(v[1].data(), 1, d);
            sbvkk_addresses(v[1].data(), 1, a);
            if ((memcmp(d, v[2].data(), 32) || memcmp(a, v[3].data(), 20)) && bad++ < 8) fprintf(stderr, "line %zu: the key's hash differs\n", lines);
            free(d);
            free(a);
        } else if (fine && kind == 'R' && tok.size() == 6 && v[1].size() == 64 && v[2].size() == 1 && v[3].size() == 32 && v[4].size() == 1 &&
                   v[4][0] <= 1 && (v[5].size() == 20 || tok[5] == "-")) {
            const int k = v[4][0];
            sigs[k].insert(sigs[k].end(), v[1].begin(), v[1].end());
            rids[k].push_back(v[2][0]);
            digs[k].insert(digs[k].end(), v[3].begin(), v[3].end());
            v[5].resize(20, 0);
            addrs[k].insert(addrs[k].end(), v[5].begin(), v[5].end());
            want_ok[k].push_back(tok[5] != "-");
        } else {
            fprintf(stderr, "line %zu is malformed\n", lines);
            return 2;
        }
        ++lines;
    }
    fclose(f);
    if (lines == 0) { fprintf(stderr, "no cases\n"); return 2; }
    for (uint32_t flags = 0; flags < 2; ++flags) {
        const size_t n = rids[flags].size();
        for (size_t lanes : {(size_t)5, n + 3}) {
            if (n == 0) continue;
            uint8_t* ga = (uint8_t*)malloc(20 * n);
            uint8_t* gok = (uint8_t*)malloc(n);
            memset(ga, 0xA5, 20 * n);
            memset(gok, 0xA5, n);
            sbvkk_recover_addr(sigs[flags].data(), rids[flags].data(), digs[flags].data(), n, flags, lanes, ga, gok);
            for (size_t i = 0; i < n; ++i)
                if (gok[i] != want_ok[flags][i] || memcmp(ga + 20 * i, &addrs[flags][20 * i], 20)) {
                    if (bad++ < 8) fprintf(stderr, "flags %u, recovery case %zu, %zu lanes: the address differs\n", flags, i, lanes);
                }
            free(ga);
            free(gok);
        }
    }
    printf("%zu cases, %zu differ\n", lines, bad);
    if (!rids[0].empty() || !rids[1].empty()) free(const_cast<kapt*>(gtab()));
    return bad ? 1 : 0;
}
#endif
