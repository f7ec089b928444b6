// k256_schnorr_keyed_emul.cc — CPU TEST TIER ONLY: BIP-340 Schnorr against registered secp256k1 keys
// (consensus_amd/csrc/k256_schnorr_keyed.h, k256_schnorr_keyed_kernels.hip), lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them as the kernels do: 64-lane groups, the two ballots over
// each group (k256_keyed_slot_wide per lane, a live lane and no live narrow lane = wide: what k256_keyed_wave_wide computes with
// __ballot on the device), the lanes behind the batch's end left out, one byte per verdict.  The registry comes from the host
// builders (k256_keyed_host_comb, k256_keyed_host_wide_window), the reference of the device builders; its arrays — key bytes, valid
// bytes, 8-bit combs, the pool of 16-bit combs — are allocated exactly, so that a sanitizer build sees any access outside them.  The
// comb of G is 16 bits wide here (the device walks a 20-bit one with the same walker).  Not part of libsbv.so, never shipped, not a
// fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     k256_schnorr_keyed_emul CASES
// CASES holds one record per line, blank-separated hex fields:
//     K key64 widen                    a registry slot, in slot order; widen = 01: the slot gets a 16-bit comb
//     L pk key64 ok                    a lifting case
//     V msg sig slot ok                a verification item (slot: 8 hex digits), in batch order
//     W in192 slot out128              a walk case of the debug op
// The items and walk cases run twice: with no slot wide and with the widened slots.  Exit status 0 = every byte matched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_schnorr_keyed.h"

using namespace sbv;

namespace {
constexpr int kGBits = 16;

template <class F>
void parallel(size_t n, F f) {
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(32u, std::thread::hardware_concurrency()), n));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([=] { for (size_t i = t; i < n; i += nt) f(i); });
    for (auto& t : th) t.join();
}

const kapt* g_comb16() {
    static kapt* tab = nullptr;
    if (!tab) {
        const int windows = (257 + kGBits - 1) / kGBits;
        tab = (kapt*)aligned_alloc(64, sizeof(kapt) * ((size_t)windows << (kGBits - 1)));
        parallel(windows, [&](size_t j) { k256_build_g_window_bits(kGBits, (int)j, tab + (j << (kGBits - 1)), 1 << (kGBits - 1)); });
    }
    return tab;
}

void load_be(u32* w, const uint8_t* b, int words) {
    for (int k = 0; k < words; ++k) w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
void store_be(uint8_t* b, const u32* w, int words) {
    for (int k = 0; k < words; ++k) { b[4 * k] = (uint8_t)(w[k] >> 24); b[4 * k + 1] = (uint8_t)(w[k] >> 16); b[4 * k + 2] = (uint8_t)(w[k] >> 8); b[4 * k + 3] = (uint8_t)w[k]; }
}

// the registry as the library holds it on the device: exact allocations
struct Registry {
    uint8_t* kkeys = nullptr;
    kapt* ktab = nullptr;
    kapt* wtab = nullptr;
    uint8_t* kvalid = nullptr;
    u32* kwidx = nullptr;
    u32 nkeys = 0, nwide = 0;
    ~Registry() { free(kkeys); free(ktab); free(wtab); free(kvalid); free(kwidx); }
    K256KeyedRegistry view(bool with_wide) const {
        K256KeyedRegistry r;
        r.ktab = ktab; r.kvalid = kvalid; r.wtab = wtab; r.kwidx = with_wide && nwide ? kwidx : nullptr; r.nkeys = nkeys;
        return r;
    }
};

Registry* build_registry(const uint8_t* keys, size_t nkeys, const uint8_t* widen) {
    Registry* r = new Registry;
    r->nkeys = (u32)nkeys;
    if (nkeys == 0) return r;
    r->kkeys = (uint8_t*)malloc(nkeys * SBV_K256_KEY_BYTES);
    memcpy(r->kkeys, keys, nkeys * SBV_K256_KEY_BYTES);
    r->ktab = (kapt*)aligned_alloc(64, nkeys * SBV_K256_KEYTAB_ENTRIES * sizeof(kapt));
    r->kvalid = (uint8_t*)malloc(nkeys);
    r->kwidx = (u32*)malloc(nkeys * sizeof(u32));
    parallel(nkeys, [&](size_t s) {
        r->kvalid[s] = k256_keyed_host_comb(keys + s * SBV_K256_KEY_BYTES, r->ktab + s * SBV_K256_KEYTAB_ENTRIES) ? 1 : 0;
        r->kwidx[s] = SBV_K256_WIDE_NONE;
    });
    for (size_t s = 0; s < nkeys; ++s) if (widen && widen[s] && r->kvalid[s]) ++r->nwide;      // the library widens points only
    if (r->nwide) r->wtab = (kapt*)aligned_alloc(64, (size_t)r->nwide * SBV_K256_WIDE_COMB_BYTES);
    u32 w = 0;
    for (size_t s = 0; s < nkeys; ++s) {
        if (!(widen && widen[s] && r->kvalid[s])) continue;
        u32 kw[16];
        memcpy(kw, keys + s * SBV_K256_KEY_BYTES, sizeof(kw));
        kfe x, y;
        (void)k256_key_load_words(kw, x, y);
        kapt* comb = r->wtab + (size_t)w * SBV_K256_WIDE_ENTRIES;
        memset((void*)comb, 0, SBV_K256_WIDE_COMB_BYTES);
        parallel(SBV_K256_WIDE_WINDOWS, [&](size_t j) { k256_keyed_host_wide_window(x, y, SBV_K256_WIDE_BITS, (int)j, comb + j * SBV_K256_WIDE_PER_WINDOW); });
        r->kwidx[s] = w++;
    }
    return r;
}

// one 64-lane group of a kernel: live(i) per lane, then the wave rule, then lane(i, live, wide); returns the lanes of a wide group
template <class Live, class Lane>
unsigned long run_waves(const K256KeyedRegistry& reg, const u32* slots, size_t n, Live live_of, Lane lane) {
    const size_t waves = (n + 63) / 64;
    std::vector<unsigned long> wl(waves, 0);
    parallel(waves, [&](size_t wv) {
        const size_t w0 = wv * 64, w1 = std::min(n, w0 + 64);
        bool any_live = false, any_live_narrow = false;        // the two ballots
        for (size_t i = w0; i < w1; ++i) {
            const bool live = live_of(i);
            any_live = any_live || live;
            any_live_narrow = any_live_narrow || (live && !k256_keyed_slot_wide(slots[i], reg));
        }
        const bool wide = k256_wave_is_wide(any_live, any_live_narrow);
        for (size_t i = w0; i < w1; ++i) lane(i, live_of(i), wide);
        if (wide) wl[wv] = w1 - w0;
    });
    unsigned long total = 0;
    for (unsigned long v : wl) total += v;
    return total;
}

}  // namespace

extern "C" {

// keys: nkeys x 64 bytes in slot order; widen (may be null): widen[s] != 0 gives slot s a 16-bit comb if its key is a point
void* sbvk256sk_registry_new(const uint8_t* keys, size_t nkeys, const uint8_t* widen) { return build_registry(keys, nkeys, widen); }
void sbvk256sk_registry_free(void* h) { delete (Registry*)h; }
void sbvk256sk_registry_valid(void* h, uint8_t* out) { const Registry* r = (const Registry*)h; if (r->nkeys) memcpy(out, r->kvalid, r->nkeys); }

// k_k256_schnorr_verify_keyed behind the entry's rule for an empty registry; with_wide = 0 hides the 16-bit combs (no slot is wide).
// Returns the lanes that took the 16-bit walk.
unsigned long sbvk256sk_verify(void* h, int with_wide, const uint8_t* msgs, const uint8_t* sigs, const u32* slots, size_t n, uint8_t* ok) {
    const Registry* r = (const Registry*)h;
    if (n == 0) return 0;
    if (r->nkeys == 0) { memset(ok, 0, n); return 0; }
    const K256KeyedRegistry reg = r->view(with_wide != 0);
    const kgcomb gc = kgcomb_make(g_comb16(), kGBits);
    auto live_of = [&](size_t i) {
        u32 rs[16];
        load_be(rs, sigs + 64 * i, 16);
        return k256_schnorr_keyed_live(rs, slots[i], reg);
    };
    return run_waves(reg, slots, n, live_of, [&](size_t i, bool live, bool wide) {
        u32 m[8], rs[16];
        load_be(m, msgs + 32 * i, 8);
        load_be(rs, sigs + 64 * i, 16);
        ok[i] = k256_schnorr_keyed_lane(m, rs, slots[i], live, reg, r->kkeys, gc, wide) ? 1 : 0;
    });
}

// k_k256_schnorr_lift; ok may be null
void sbvk256sk_lift(const uint8_t* pks, size_t m, uint8_t* keys64, uint8_t* ok) {
    parallel(m, [=](size_t i) {
        u32 pk[8], key[16];
        load_be(pk, pks + 32 * i, 8);
        const bool good = k256_schnorr_lift_lane(pk, key);
        store_be(keys64 + 64 * i, key, 16);
        if (ok) ok[i] = good ? 1 : 0;
    });
}

// k_k256_schnorr_keyed_op: 192 bytes in, a slot, 128 bytes out per case.  Returns the lanes that took the 16-bit walk, -1 for another op.
long sbvk256sk_op(void* h, int with_wide, int op, const uint8_t* in, const u32* slots, uint8_t* out, size_t n) {
    const Registry* r = (const Registry*)h;
    if (op < 0 || op >= SBV_K256_SCHNORR_KEYED_OPS) return -1;
    if (n == 0) return 0;
    if (r->nkeys == 0) { memset(out, 0, 128 * n); return 0; }
    const K256KeyedRegistry reg = r->view(with_wide != 0);
    const kgcomb gc = kgcomb_make(g_comb16(), kGBits);
    return (long)run_waves(reg, slots, n, [&](size_t i) { return k256_schnorr_keyed_op_live(slots[i], reg); }, [&](size_t i, bool live, bool wide) {
        u32 a[SBV_K256_SIGN_OP_IN_WORDS], res[SBV_K256_SIGN_OP_OUT_WORDS];
        load_be(a, in + 192 * i, SBV_K256_SIGN_OP_IN_WORDS);
        k256_schnorr_keyed_op_lane(a, slots[i], live, reg, gc, wide, res);
        store_be(out + 128 * i, res, SBV_K256_SIGN_OP_OUT_WORDS);
    });
}

}  // extern "C"

#ifdef SBV_EMUL_MAIN
static bool unhex(const char* s, std::vector<uint8_t>& out, size_t want) {
    out.clear();
    if (strlen(s) != 2 * want) return false;
    for (size_t i = 0; i < 2 * want; i += 2) {
        unsigned v;
        if (sscanf(s + i, "%2x", &v) != 1) return false;
        out.push_back((uint8_t)v);
    }
    return true;
}
static void append(std::vector<uint8_t>& dst, const std::vector<uint8_t>& src) { dst.insert(dst.end(), src.begin(), src.end()); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> keys, widen, lpk, lkey, lok, vmsg, vsig, vok, win, wout;
    std::vector<u32> vslot, wslot;
    static char k[4], a[400], b[400], c[400], d[400];
    size_t line = 0;
    auto bad_line = [&] { fprintf(stderr, "record %zu is malformed\n", line); return 2; };
    while (fscanf(f, "%3s", k) == 1) {
        std::vector<uint8_t> x, y, z, u;
        if (!strcmp(k, "K")) {
            if (fscanf(f, "%399s %399s", a, b) != 2 || !unhex(a, x, 64) || !unhex(b, y, 1)) return bad_line();
            append(keys, x); widen.push_back(y[0]);
        } else if (!strcmp(k, "L")) {
            if (fscanf(f, "%399s %399s %399s", a, b, c) != 3 || !unhex(a, x, 32) || !unhex(b, y, 64) || !unhex(c, z, 1)) return bad_line();
            append(lpk, x); append(lkey, y); lok.push_back(z[0]);
        } else if (!strcmp(k, "V")) {
            if (fscanf(f, "%399s %399s %399s %399s", a, b, c, d) != 4 || !unhex(a, x, 32) || !unhex(b, y, 64) || !unhex(c, z, 4) || !unhex(d, u, 1)) return bad_line();
            append(vmsg, x); append(vsig, y); vok.push_back(u[0]);
            vslot.push_back(((u32)z[0] << 24) | ((u32)z[1] << 16) | ((u32)z[2] << 8) | z[3]);
        } else if (!strcmp(k, "W")) {
            if (fscanf(f, "%399s %399s %399s", a, b, c) != 3 || !unhex(a, x, 192) || !unhex(b, z, 4) || !unhex(c, y, 128)) return bad_line();
            append(win, x); append(wout, y);
            wslot.push_back(((u32)z[0] << 24) | ((u32)z[1] << 16) | ((u32)z[2] << 8) | z[3]);
        } else {
            return bad_line();
        }
        ++line;
    }
    fclose(f);
    if (widen.empty() || lok.empty() || vok.empty() || wslot.empty()) { fprintf(stderr, "no cases\n"); return 2; }
    size_t bad = 0;
    const size_t m = lok.size(), n = vok.size(), nw = wslot.size();
    std::vector<uint8_t> gkey(64 * m, 0xA5), gok(m, 0xA5);
    sbvk256sk_lift(lpk.data(), m, gkey.data(), gok.data());
    for (size_t i = 0; i < m; ++i)
        if ((memcmp(&gkey[64 * i], &lkey[64 * i], 64) || gok[i] != lok[i]) && bad++ < 8) fprintf(stderr, "lift case %zu differs\n", i);
    void* reg = sbvk256sk_registry_new(keys.data(), widen.size(), widen.data());
    unsigned long wide_lanes = 0;
    for (int with_wide : {0, 1}) {
        std::vector<uint8_t> got(n, 0xA5), out(128 * nw, 0xA5);
        const unsigned long wl = sbvk256sk_verify(reg, with_wide, vmsg.data(), vsig.data(), vslot.data(), n, got.data());
        if (with_wide) wide_lanes = wl;
        else if (wl) { ++bad; fprintf(stderr, "a wide walk without wide slots\n"); }
        for (size_t i = 0; i < n; ++i)
            if (got[i] != vok[i] && bad++ < 8) fprintf(stderr, "item %zu, wide %d: the verdict differs\n", i, with_wide);
        if (sbvk256sk_op(reg, with_wide, 0, win.data(), wslot.data(), out.data(), nw) < 0) ++bad;
        for (size_t i = 0; i < nw; ++i)
            if (memcmp(&out[128 * i], &wout[128 * i], 128) && bad++ < 8) fprintf(stderr, "walk case %zu, wide %d differs\n", i, with_wide);
    }
    sbvk256sk_registry_free(reg);
    printf("%zu records, %zu lift, %zu items, %zu walk, %lu wide lanes, %zu differ\n", line, m, n, nw, wide_lanes, bad);
    free(const_cast<kapt*>(g_comb16()));
    return bad ? 1 : 0;
}
#endif
