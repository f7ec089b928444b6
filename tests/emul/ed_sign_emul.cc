// ed_sign_emul.cc — CPU TEST TIER ONLY: the Ed25519 batch signer (consensus_amd/csrc/ed25519_sign.h, ed25519_sign_kernels.hip), lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them as the kernels do: k_ed_sign_expand (seed -> the 96-byte
// expanded record), k_ed_sign (key selection, the rejected lanes, ed_sign_lane), the three unit operations of sbv_debug_ed25519_sign_op
// and sha512_head_msg on its own.  The 16-bit comb of B is the host builder's (build_ed_b16_window: 50 MB, ~0.2 s on 16 threads).
// Not part of libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     ed_sign_emul CASES
// CASES holds one case per line, four hex fields separated by blanks: seed, public key, message ("-" when empty), signature.
// Every case is expanded and signed; exit status 0 = every public key and every signature matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/ed25519_sign.h"

using namespace sbv;

namespace {

const aniels* b16() {
    static aniels* tab = nullptr;
    if (!tab) {
        tab = (aniels*)aligned_alloc(64, sizeof(aniels) * SBV_ED_B16_ENTRIES);
        std::vector<std::thread> th;
        for (int j = 0; j < SBV_ED_B16_WINDOWS; ++j) th.emplace_back([j] { build_ed_b16_window(j, tab + (size_t)j * SBV_ED_B16_PER_WINDOW); });
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

}  // namespace

extern "C" {

// k_ed_sign_expand
void sbvedsign_expand(const uint8_t* seeds, size_t m, uint8_t* expanded, uint8_t* pks) {
    const aniels* tab = b16();
    parallel(m, [=](size_t i) {
        u32 seed[8], rec[SBV_ED_SIGN_REC_WORDS];
        memcpy(seed, seeds + 32 * i, 32);
        ed_sign_expand_lane(seed, tab, rec);
        memcpy(expanded + 96 * i, rec, 96);
        if (pks) memcpy(pks + 32 * i, rec + 16, 32);
    });
}

// k_ed_sign
void sbvedsign_sign(const uint8_t* expanded, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs, const uint64_t* moff, size_t n,
                    uint8_t* sigs, uint8_t* ok) {
    const aniels* tab = b16();
    parallel(n, [=](size_t i) {
        const u32 kidx = key_index ? key_index[i] : (u32)(i % n_keys);
        const u64 m0 = moff[i], m1 = moff[i + 1];
        u32 rec[SBV_ED_SIGN_REC_WORDS], sig[16];
        if (kidx >= n_keys || m1 < m0) {
            memset(sigs + 64 * i, 0, 64);
            ok[i] = 0;
            return;
        }
        memcpy(rec, expanded + 96 * (size_t)kidx, 96);
        ed_sign_lane(rec, msgs + m0, (size_t)(m1 - m0), tab, sig);
        memcpy(sigs + 64 * i, sig, 64);
        ok[i] = 1;
    });
}

// k_ed_sign_op: 0 = sc25519_muladd (k | a | r -> S), 1 = sc25519_reduce256, 2 = encode([s]B)
int sbvedsign_op(int op, const uint8_t* in, uint8_t* out, size_t n) {
    if (op < 0 || op > 2) return -1;
    const aniels* tab = op == 2 ? b16() : nullptr;
    parallel(n, [=](size_t i) {
        u256 res;
        if (op == 0) {
            u256 k, a, r;
            memcpy(k.v, in + 96 * i, 32); memcpy(a.v, in + 96 * i + 32, 32); memcpy(r.v, in + 96 * i + 64, 32);
            sc25519_muladd(res, k, a, r);
        } else {
            u256 s;
            memcpy(s.v, in + 32 * i, 32);
            if (op == 1) sc25519_reduce256(res, s);
            else ed_encode_sB(res.v, s, tab);
        }
        memcpy(out + 32 * i, res.v, 32);
    });
    return 0;
}

// the digest as its 64 bytes
void sbvedsign_sha512_head_msg(const uint8_t* head, size_t head_len, const uint8_t* msg, size_t mlen, uint8_t out[64]) {
    u64 h[8];
    sha512_head_msg(head, head_len, msg, mlen, h);
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(h[i] >> (56 - 8 * b));
}

}  // extern "C"

#ifdef SBV_EMUL_MAIN
static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    out.clear();
    if (s == "-") return true;
    if (s.size() & 1) return false;
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
    std::vector<uint8_t> seeds, pks, msgs, sigs;
    std::vector<uint64_t> moff(1, 0);
    static char a[70], b[70], c[20000], d[140];
    while (fscanf(f, "%69s %69s %19999s %139s", a, b, c, d) == 4) {
        std::vector<uint8_t> seed, pk, msg, sig;
        if (!unhex(a, seed) || !unhex(b, pk) || !unhex(c, msg) || !unhex(d, sig) || seed.size() != 32 || pk.size() != 32 || sig.size() != 64) {
            fprintf(stderr, "case %zu is malformed\n", moff.size() - 1);
            return 2;
        }
        seeds.insert(seeds.end(), seed.begin(), seed.end());
        pks.insert(pks.end(), pk.begin(), pk.end());
        msgs.insert(msgs.end(), msg.begin(), msg.end());
        sigs.insert(sigs.end(), sig.begin(), sig.end());
        moff.push_back(msgs.size());
    }
    fclose(f);
    const size_t n = moff.size() - 1;
    if (n == 0) { fprintf(stderr, "no cases\n"); return 2; }
    msgs.push_back(0);                                   // a payload pointer for an all-empty list
    std::vector<uint8_t> exp(96 * n), gpk(32 * n), gsig(64 * n), ok(n);
    sbvedsign_expand(seeds.data(), n, exp.data(), gpk.data());
    sbvedsign_sign(exp.data(), (uint32_t)n, nullptr, msgs.data(), moff.data(), n, gsig.data(), ok.data());   // case i signs with key i
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i)
        if (!ok[i] || memcmp(&gpk[32 * i], &pks[32 * i], 32) || memcmp(&gsig[64 * i], &sigs[64 * i], 64)) {
            if (bad++ < 8) fprintf(stderr, "case %zu (message of %zu bytes) differs\n", i, (size_t)(moff[i + 1] - moff[i]));
        }
    printf("%zu cases, %zu differ\n", n, bad);
    free(const_cast<aniels*>(b16()));
    return bad ? 1 : 0;
}
#endif
