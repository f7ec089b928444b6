// k256_keyed_emul.cc — CPU TEST TIER ONLY: the registered-key secp256k1 step (consensus_amd/csrc/k256_keyed.h) lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them in launch order — the registry's chain / rows / fill
// lanes over the registered keys, the wide-comb builder lanes, stage A on records in workgroups of 64 lanes, then stage B with the
// wavefront ballot of k_k256_keyed_verify — so the build container can diff the keyed step against the oracle without a GPU.
// Not part of libsbv.so, never shipped, not a fallback.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_keyed.h"
#include "../../consensus_amd/csrc/sha256_dev.h"

using namespace sbv;

namespace {
constexpr int kGBits = 16;              // the emulator's comb of G (the device walks a 20-bit one with the same walker)

unsigned threads() { return std::max(1u, std::min(32u, std::thread::hardware_concurrency())); }
template <class F>
void parallel(size_t n, F f) {
    const unsigned nt = (unsigned)std::min<size_t>(threads(), n ? n : 1);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([=] { for (size_t i = t; i < n; i += nt) f(i); });
    for (auto& t : th) t.join();
}

const kapt* gcomb() {
    static kapt* tab = nullptr;
    if (!tab) {
        const int windows = (257 + kGBits - 1) / kGBits;
        tab = (kapt*)aligned_alloc(64, sizeof(kapt) * ((size_t)windows << (kGBits - 1)));
        parallel(windows, [&](size_t j) { k256_build_g_window_bits(kGBits, (int)j, tab + (j << (kGBits - 1)), 1 << (kGBits - 1)); });
    }
    return tab;
}

struct Registry {
    kapt* ktab = nullptr;
    kapt* wtab = nullptr;
    std::vector<uint8_t> kvalid;
    std::vector<u32> kwidx;
    u32 nkeys = 0, nwide = 0;
    ~Registry() { free(ktab); free(wtab); }
    K256KeyedRegistry view() const {
        K256KeyedRegistry r;
        r.ktab = ktab; r.kvalid = kvalid.data(); r.wtab = wtab; r.kwidx = nwide ? kwidx.data() : nullptr; r.nkeys = nkeys;
        return r;
    }
};

// launch_k256_reg_build in launch order: the table zeroed, then chain (one quad per key), rows and fill over slots [0, nkeys)
void build_slot_combs(const uint8_t* kkeys, u32 nkeys, kapt* ktab, uint8_t* kvalid) {
    memset((void*)ktab, 0, (size_t)nkeys * SBV_K256_KEYTAB_ENTRIES * sizeof(kapt));
    parallel(nkeys, [&](size_t k) {
        // scratch indexed by the chain's number as on the device; one key per pass here (slot0 = k, count = 1)
        std::vector<u32> jstate(SBV_K256_STATE_WORDS), bases((size_t)SBV_GTAB_WINDOWS * SBV_K256_BASES_STRIDE), tmp((size_t)SBV_GTAB_WINDOWS * SBV_K256_WINDOW_TMP);
        k256_quad_host q;
        k256_reg_chain_run(q, kkeys, (u32)k, 0, jstate.data(), bases.data(), kvalid);
        for (u32 lane = 0; lane < SBV_GTAB_WINDOWS * 2; ++lane) k256_reg_rows_lane(lane, 1, (u32)k, bases.data(), tmp.data(), ktab);
        for (u32 lane = 0; lane < SBV_GTAB_WINDOWS * 7; ++lane) k256_reg_fill_lane(lane, 1, (u32)k, tmp.data(), ktab);
    });
}

// launch_k256_widetab: window 16 zeroed, then one lane per run
void build_wide(const kapt* qtab, kapt* wide) {
    memset((void*)(wide + (size_t)(SBV_K256_WIDE_WINDOWS - 1) * SBV_K256_WIDE_PER_WINDOW), 0, (size_t)SBV_K256_WIDE_PER_WINDOW * sizeof(kapt));
    parallel(SBV_K256_WIDE_WINDOWS, [&](size_t j) {
        std::vector<u32> tmp(SBV_K256_WIDE_TMP_WORDS);
        if (j == SBV_K256_WIDE_WINDOWS - 1) { k256_widetab_lane(qtab, SBV_K256_WIDE_LANES - 1, tmp.data(), wide); return; }
        for (u32 q = 0; q < SBV_K256_WIDE_RUNS_PER_WINDOW; ++q) k256_widetab_lane(qtab, (u32)j * SBV_K256_WIDE_RUNS_PER_WINDOW + q, tmp.data(), wide);
    });
}

void build_registry(Registry& r, const uint8_t* keys, size_t nkeys, const uint8_t* widen) {
    r.nkeys = (u32)nkeys;
    r.ktab = (kapt*)aligned_alloc(64, std::max<size_t>(1, nkeys) * SBV_K256_KEYTAB_ENTRIES * sizeof(kapt));
    r.kvalid.assign(nkeys, 0);
    r.kwidx.assign(nkeys, SBV_K256_WIDE_NONE);
    uint8_t* kk = (uint8_t*)aligned_alloc(64, std::max<size_t>(64, nkeys * SBV_K256_KEY_BYTES));
    memcpy(kk, keys, nkeys * SBV_K256_KEY_BYTES);
    build_slot_combs(kk, r.nkeys, r.ktab, r.kvalid.data());
    free(kk);
    for (size_t s = 0; s < nkeys; ++s) if (widen && widen[s] && r.kvalid[s]) ++r.nwide;      // the library widens points only
    if (r.nwide) r.wtab = (kapt*)aligned_alloc(64, (size_t)r.nwide * SBV_K256_WIDE_COMB_BYTES);
    u32 w = 0;
    for (size_t s = 0; s < nkeys; ++s)
        if (widen && widen[s] && r.kvalid[s]) {
            build_wide(r.ktab + s * SBV_K256_KEYTAB_ENTRIES, r.wtab + (size_t)w * SBV_K256_WIDE_ENTRIES);
            r.kwidx[s] = w++;
        }
}

// stage A (k_k256_keyed_prep) + stage B (k_k256_keyed_verify) over n records; returns the lanes that took the wide walk
unsigned long keyed_step(const Registry& r, const uint8_t* recs, const u32* slots, size_t n, uint8_t* bitmap) {
    memset(bitmap, 0, (n + 7) / 8);
    if (n == 0 || r.nkeys == 0) return 0;             // the library's rule: without a registry every record is a reject
    size_t cap = (n + 63) & ~(size_t)63;
    std::vector<u32> pr(8 * cap), u1(8 * cap), u2(8 * cap), qx(8 * cap), qy(8 * cap), sm(8 * cap);
    std::vector<uint8_t> ok(cap, 0);
    Scratch s{pr.data(), u1.data(), u2.data(), qx.data(), qy.data(), sm.data(), ok.data(), cap};
    const int T = k256_keyed_prep_T(n);
    const size_t per_block = (size_t)64 * T;
    for (size_t b = 0; b * per_block < n; ++b)
        for (int t = 0; t < 64; ++t) k256_keyed_prep_lane(recs, n, s, b * per_block + t, (size_t)64, T);
    const K256KeyedRegistry reg = r.view();
    const kgcomb gc = kgcomb_make(gcomb(), kGBits);
    const size_t waves = (n + 63) / 64;
    std::vector<unsigned long> wl(waves, 0);
    parallel(waves, [&](size_t wv) {
        const size_t w0 = wv * 64, w1 = std::min(n, w0 + 64);
        bool any_live = false, any_live_narrow = false;        // the two ballots
        for (size_t i = w0; i < w1; ++i) {
            const bool live = k256_keyed_live(s, i, slots[i], reg);
            any_live = any_live || live;
            any_live_narrow = any_live_narrow || (live && !k256_keyed_slot_wide(slots[i], reg));
        }
        const bool wide = any_live && !any_live_narrow;
        uint8_t bits[8] = {0};
        for (size_t i = w0; i < w1; ++i) {
            const bool live = k256_keyed_live(s, i, slots[i], reg);
            if (k256_keyed_verify_lane(s, i, slots[i], live, reg, gc, wide)) bits[(i - w0) >> 3] |= (uint8_t)(1u << (i & 7));
        }
        memcpy(bitmap + (w0 >> 3), bits, (w1 - w0 + 7) / 8);
        if (wide) wl[wv] = w1 - w0;
    });
    unsigned long total = 0;
    for (unsigned long v : wl) total += v;
    return total;
}
}  // namespace

extern "C" {

// records n x 96 (r | s | hash) + slots against the registry of `nkeys` keys (64 bytes each); widen[s] != 0: slot s gets a 16-bit comb
// if its key is a point (widen may be null).  valid_out (may be null): the slots' valid bytes.  Returns the lanes that took the wide walk.
unsigned long sbvk256_verify_keyed(const uint8_t* recs_in, const u32* slots, size_t n, const uint8_t* keys, size_t nkeys, const uint8_t* widen,
                                   uint8_t* bitmap, uint8_t* valid_out) {
    Registry r;
    build_registry(r, keys, nkeys, widen);
    if (valid_out) memcpy(valid_out, r.kvalid.data(), nkeys);
    uint8_t* recs = (uint8_t*)aligned_alloc(64, std::max<size_t>(64, (n * SBV_K256_REC_BYTES + 63) & ~(size_t)63));
    memcpy(recs, recs_in, n * SBV_K256_REC_BYTES);
    const unsigned long wide = keyed_step(r, recs, slots, n, bitmap);
    free(recs);
    return wide;
}

// the _msgs_keyed form: the front end lane (SHA-256 + strict DER, sha256_dev.h) writes the records, then the same step.  The offset
// tables are checked as the entry checks them (start at 0, never decrease): -2 = refused.
int sbvk256_verify_msgs_keyed(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const u32* slots, size_t n,
                              const uint8_t* keys, size_t nkeys, uint8_t* bitmap) {
    for (const uint64_t* o : {moff, soff}) {
        if (o[0] != 0) return -2;
        for (size_t i = 0; i < n; ++i) if (o[i + 1] < o[i]) return -2;
    }
    Registry r;
    build_registry(r, keys, nkeys, nullptr);
    u32* recs = (u32*)aligned_alloc(64, std::max<size_t>(64, (n * SBV_K256_REC_BYTES + 63) & ~(size_t)63));
    for (size_t i = 0; i < n; ++i)
        msg_frontend_lane(msgs + moff[i], (size_t)(moff[i + 1] - moff[i]), sigs + soff[i], (size_t)(soff[i + 1] - soff[i]), recs + 24 * i);
    keyed_step(r, reinterpret_cast<const uint8_t*>(recs), slots, n, bitmap);
    free(recs);
    return 0;
}

// Three builds of the 8-bit comb of one key (33 x 128 entries of 64 bytes each, unwritten entries zero): the registry's lanes
// (k256_reg_chain_run / rows / fill, the key from a registry key array at slot 1), the host builder, and the grouped step's lanes
// (k256_chain_run with the key read from a batch's tuples through GroupState::group_rep, in two chunks of windows as the step runs
// them).  Returns the valid flags: bit 0 registry, bit 1 host, bit 2 grouped.
int sbvk256_tables(const uint8_t key[64], uint8_t* out_reg, uint8_t* out_host, uint8_t* out_grouped) {
    const size_t per_key = SBV_K256_KEYTAB_ENTRIES;
    int flags = 0;
    {   // registry: two slots, the key in the second (slot0 and the scratch index differ)
        alignas(64) uint8_t kk[2 * SBV_K256_KEY_BYTES] = {0};
        memcpy(kk + SBV_K256_KEY_BYTES, key, SBV_K256_KEY_BYTES);
        std::vector<kapt> tab(2 * per_key);
        uint8_t valid[2] = {9, 9};
        build_slot_combs(kk, 2, tab.data(), valid);
        memcpy(out_reg, tab.data() + per_key, per_key * sizeof(kapt));
        if (valid[0] != 0) return -1;                  // (0, 0) is no point
        flags |= valid[1] ? 1 : 0;
    }
    {
        std::vector<kapt> tab(per_key);
        flags |= k256_keyed_host_comb(key, tab.data()) ? 2 : 0;
        memcpy(out_host, tab.data(), per_key * sizeof(kapt));
    }
    {   // grouped: group 0's representative is tuple 1 of a two-tuple batch
        uint8_t* tuples = (uint8_t*)aligned_alloc(64, 320);
        memset(tuples, 0, 320);
        memcpy(tuples + 160 + 96, key, 64);
        u32 group_rep[1] = {1};
        GroupState g = {};
        g.group_rep = group_rep;
        std::vector<u32> jstate(SBV_K256_STATE_WORDS), bases((size_t)SBV_GTAB_WINDOWS * SBV_K256_BASES_STRIDE), tmp(SBV_K256_WINDOW_TMP);
        std::vector<kapt> tab(per_key);
        memset((void*)tab.data(), 0, per_key * sizeof(kapt));
        uint8_t valid = 9;
        const int chunks = 2;
        for (int c = 0; c < chunks; ++c) {
            const int j_first = SBV_GTAB_WINDOWS * c / chunks, j_end = SBV_GTAB_WINDOWS * (c + 1) / chunks;
            k256_quad_host q;
            k256_chain_run(q, tuples, 0, g, jstate.data(), bases.data(), &valid, j_first, j_end - 1);
            for (int j = j_first; j < j_end; ++j) {
                kapt* row = tab.data() + (size_t)j * SBV_GTAB_PER_WINDOW;
                for (int which = 0; which < 2; ++which) {
                    if (which == 1 && j == SBV_GTAB_WINDOWS - 1) continue;
                    k256_rows_lane(bases.data() + (size_t)j * SBV_K256_BASES_STRIDE, which, j == SBV_GTAB_WINDOWS - 1, tmp.data(), row);
                }
                if (j != SBV_GTAB_WINDOWS - 1)
                    for (int a = 1; a <= 7; ++a) k256_fill_lane(a, tmp.data(), row);
            }
        }
        flags |= valid ? 4 : 0;
        memcpy(out_grouped, tab.data(), per_key * sizeof(kapt));
        free(tuples);
    }
    return flags;
}

// entries of the 16-bit comb the device builder lanes make from the registry comb of `key` that differ from the host reference
// builder's (k256_keyed_host_wide_window: windows 0..15 whole, window 16 its first entry, the rest zero); -1 = not a point
long sbvk256_wide_mismatches(const uint8_t key[64]) {
    Registry r;
    const uint8_t one = 1;
    build_registry(r, key, 1, &one);
    if (!r.kvalid[0]) return -1;
    u32 w[16];
    memcpy(w, key, 64);
    kfe x, y;
    k256_key_load_words(w, x, y);
    std::vector<kapt> want(SBV_K256_WIDE_ENTRIES);
    memset((void*)want.data(), 0, SBV_K256_WIDE_COMB_BYTES);
    parallel(SBV_K256_WIDE_WINDOWS, [&](size_t j) { k256_keyed_host_wide_window(x, y, SBV_K256_WIDE_BITS, (int)j, want.data() + j * SBV_K256_WIDE_PER_WINDOW); });
    long bad = 0;
    for (size_t e = 0; e < want.size(); ++e)
        if (memcmp(r.wtab + e, &want[e], sizeof(kapt)) != 0) ++bad;
    return bad;
}

}  // extern "C"
