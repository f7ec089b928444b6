// sec1_emul.cc — CPU TEST TIER ONLY: the SEC1 key decoders (consensus_amd/csrc/sec1_keys.h, sec1_keys_kernels.hip), lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++, the contract assertions of both fields on (-DSBV_F29_CHECK,
// -DSBV_K256_CHECK), and runs them as the kernels do: k_sec1_decode_keys with its per-lane offset rule (null table = the 33-byte
// stride; a pair that is not monotone or not inside key_bytes is an empty key) and the two unit operations of sbv_debug_sec1_op.
// Not part of libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     sec1_emul CASES
// CASES holds one case per line, three fields separated by blanks: the curve (0 / 1), the key in hex ("-" for the empty key) and
// X | Y in hex ("-" for a refused key: the lane must then answer zeros).  Every key is copied into a heap block of EXACTLY its
// length before the lane sees it, so that AddressSanitizer reports any read outside key[0 .. len).  Then the cases of a curve run once
// more through the kernel's loop, packed back to back in a block of exactly their total size.  Exit status 0 = every byte matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/sec1_keys.h"

using namespace sbv;

namespace {

template <class F>
void parallel(size_t n, F f) {
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(32u, std::thread::hardware_concurrency()), n));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([=] { for (size_t i = t; i < n; i += nt) f(i); });
    for (auto& t : th) t.join();
}

void load_be(u32* w, const uint8_t* b, int words) {
    for (int k = 0; k < words; ++k) w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
void store_be(uint8_t* b, const u32* w, int words) {
    for (int k = 0; k < words; ++k) { b[4 * k] = (uint8_t)(w[k] >> 24); b[4 * k + 1] = (uint8_t)(w[k] >> 16); b[4 * k + 2] = (uint8_t)(w[k] >> 8); b[4 * k + 3] = (uint8_t)w[k]; }
}

bool decode_one(int curve, const uint8_t* key, size_t len, uint8_t* key64) {
    u32 out[16];
    const bool good = curve == SBV_SEC1_P256 ? sec1_decode_lane<SBV_SEC1_P256>(key, len, out) : sec1_decode_lane<SBV_SEC1_K256>(key, len, out);
    store_be(key64, out, 16);
    return good;
}

}  // namespace

extern "C" {

// one key on its own: the lane
int sbvsec1_decode_one(int curve, const uint8_t* key, size_t len, uint8_t* key64) {
    if (curve != SBV_SEC1_P256 && curve != SBV_SEC1_K256) return -1;
    return decode_one(curve, key, len, key64) ? 1 : 0;
}

// k_sec1_decode_keys; koff and ok may be null
int sbvsec1_decode(int curve, const uint8_t* keys, const uint64_t* koff, uint64_t key_bytes, size_t m, uint8_t* keys64, uint8_t* ok) {
    if (curve != SBV_SEC1_P256 && curve != SBV_SEC1_K256) return -1;
    parallel(m, [=](size_t i) {
        u64 k0, k1;
        if (koff) { k0 = koff[i]; k1 = koff[i + 1]; }
        else      { k0 = (u64)i * 33; k1 = k0 + 33; }
        if (!(k0 <= k1 && k1 <= key_bytes)) k0 = k1 = 0;
        const bool good = decode_one(curve, keys + k0, (size_t)(k1 - k0), keys64 + 64 * i);
        if (ok) ok[i] = good ? 1 : 0;
    });
    return 0;
}

// k_sec1_op: 192 bytes in, 128 bytes out per case
int sbvsec1_op(int curve, int op, const uint8_t* in, uint8_t* out, size_t n) {
    if ((curve != SBV_SEC1_P256 && curve != SBV_SEC1_K256) || op < 0 || op >= SBV_SEC1_OPS) return -1;
    parallel(n, [=](size_t i) {
        u32 a[SBV_K256_SIGN_OP_IN_WORDS], r[SBV_K256_SIGN_OP_OUT_WORDS];
        load_be(a, in + 192 * i, SBV_K256_SIGN_OP_IN_WORDS);
        if (curve == SBV_SEC1_P256) sec1_op_lane<SBV_SEC1_P256>(op, a, r);
        else sec1_op_lane<SBV_SEC1_K256>(op, a, r);
        store_be(out + 128 * i, r, SBV_K256_SIGN_OP_OUT_WORDS);
    });
    return 0;
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
    struct Case { int curve; std::vector<uint8_t> key, want; bool ok; };
    std::vector<Case> cs;
    static char a[8], b[400], c[140];
    while (fscanf(f, "%7s %399s %139s", a, b, c) == 3) {
        Case k;
        k.curve = atoi(a);
        k.ok = strcmp(c, "-") != 0;
        if ((k.curve != 0 && k.curve != 1) || !unhex(b, k.key) || !unhex(c, k.want) || (k.ok && k.want.size() != 64)) {
            fprintf(stderr, "case %zu is malformed\n", cs.size());
            return 2;
        }
        k.want.resize(64, 0);
        cs.push_back(k);
    }
    fclose(f);
    if (cs.empty()) { fprintf(stderr, "no cases\n"); return 2; }
    size_t bad = 0, accepted = 0;
    // every key in a heap block of exactly its length
    for (size_t i = 0; i < cs.size(); ++i) {
        const size_t len = cs[i].key.size();
        uint8_t* blk = (uint8_t*)malloc(len);                  // len 0: a block no byte of which may be read
        if (len) memcpy(blk, cs[i].key.data(), len);
        uint8_t got[64];
        memset(got, 0xA5, 64);
        const int good = sbvsec1_decode_one(cs[i].curve, blk, len, got);
        free(blk);
        accepted += good == 1;
        if (good != (cs[i].ok ? 1 : 0) || memcmp(got, cs[i].want.data(), 64)) {
            if (bad++ < 8) fprintf(stderr, "case %zu (curve %d, %zu bytes): the key differs\n", i, cs[i].curve, len);
        }
    }
    // the kernel's loop over the cases of each curve, packed in a block of exactly their total size
    for (int curve = 0; curve < 2; ++curve) {
        std::vector<uint64_t> off(1, 0);
        std::vector<size_t> idx;
        size_t total = 0;
        for (size_t i = 0; i < cs.size(); ++i)
            if (cs[i].curve == curve) { total += cs[i].key.size(); off.push_back(total); idx.push_back(i); }
        uint8_t* blk = (uint8_t*)malloc(total);
        for (size_t k = 0; k < idx.size(); ++k)
            if (!cs[idx[k]].key.empty()) memcpy(blk + off[k], cs[idx[k]].key.data(), cs[idx[k]].key.size());
        std::vector<uint8_t> got(64 * idx.size() + 1, 0xA5), gok(idx.size() + 1, 0xA5);
        sbvsec1_decode(curve, blk, off.data(), total, idx.size(), got.data(), gok.data());
        free(blk);
        for (size_t k = 0; k < idx.size(); ++k)
            if (gok[k] != (cs[idx[k]].ok ? 1 : 0) || memcmp(&got[64 * k], cs[idx[k]].want.data(), 64)) {
                if (bad++ < 8) fprintf(stderr, "curve %d, packed case %zu: the key differs\n", curve, k);
            }
        if (got[64 * idx.size()] != 0xA5 || gok[idx.size()] != 0xA5) { ++bad; fprintf(stderr, "curve %d: a byte behind the outputs was written\n", curve); }
    }
    printf("%zu cases, %zu accepted, %zu differ\n", cs.size(), accepted, bad);
    return bad ? 1 : 0;
}
#endif
