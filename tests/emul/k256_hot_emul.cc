// k256_hot_emul.cc — CPU TEST TIER ONLY: the secp256k1 grouped step with its hot-key pool (consensus_amd/csrc/k256_group.h "hot keys",
// k256_group_kernels.hip), lane by lane on a persistent key-table cache.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs them in launch order: stage A with records, grouping by key in
// first-appearance order, the key-sorted list in group_sort_group_at order, the cold groups' 8-bit combs by the chain / rows / fill
// lanes, the G lane into gacc, the class lane, the wave rule over each 64 consecutive list positions (k256_wave_is_wide: the function
// both Q kernels call), the wide lane or k256_qphase_lane_sorted in two chunks, and the tail — decay on its tick, select, evict,
// k256_widetab_lane, publish.  Every key is grouped here (the library leaves rare keys to the one-lane kernel: same verdicts).
// Not part of libsbv.so, never shipped, not a fallback.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/k256_keyed.h"

using namespace sbv;

namespace {
// The emulator walks u1 * G on a 16-bit comb of G (as k256_keyed_emul.cc does; a 20-bit one is 436 MB and minutes of host work): the same
// walker, k256_gphase_point, at another width.  The `g20` scalar cases therefore meet the window boundaries of 16 bits here, not those
// they were chosen for; only the GPU tier (tests/test_gpu_k256_hot.py) walks them at the device's 20 bits.
constexpr int kGBits = 16;
constexpr size_t kPerKey = SBV_K256_KEYTAB_ENTRIES;
constexpr u32 kNone = 0xFFFFFFFFu;

unsigned threads() { return std::max(1u, std::min(32u, std::thread::hardware_concurrency())); }
template <class F>
void parallel(size_t n, F f) {
    const unsigned nt = (unsigned)std::min<size_t>(threads(), n ? n : 1);
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

struct TupleWords {
    const uint8_t* p;
    u32 operator[](int i) const { u32 v; memcpy(&v, p + 4 * i, 4); return v; }
};

// what outlives a batch: the key-table cache (slots by first appearance) and the pool
struct State {
    u32 K = 0, W = 0, min_hits = 4096, tick = 0;
    bool cache_on = true;
    std::map<std::string, u32> index;
    std::vector<std::string> slot_key;
    kapt* ktab = nullptr;
    kapt* wtab = nullptr;
    std::vector<uint8_t> kvalid;
    std::vector<u32> kwide, khits, wowner, plist, elist;
    u32 hot[4] = {0, 0, 0, 0};
    std::vector<uint8_t> last_classes;      // per wavefront of the last batch: SBV_Q_WIDE, SBV_Q_FULL, SBV_Q_NONE
    u32 evictions = 0;
    void forget() {
        index.clear(); slot_key.clear();
        std::fill(kvalid.begin(), kvalid.end(), 0);
        std::fill(kwide.begin(), kwide.end(), kNone);
        std::fill(khits.begin(), khits.end(), 0);
        std::fill(wowner.begin(), wowner.end(), kNone);
        hot[0] = hot[1] = hot[2] = hot[3] = 0;
    }
    void release() { free(ktab); free(wtab); ktab = wtab = nullptr; }
} S;

// the chain / rows / fill lanes of one cold group, in the launcher's two chunks (the scratch is indexed by the group as on the device:
// one group per call here, so its index is 0)
void build_comb(const uint8_t* tuples, const GroupState& gin, u32 kin, kapt* tab, uint8_t* valid) {
    u32 rep1[1] = {gin.group_rep[kin]};
    GroupState g{};
    g.group_rep = rep1;
    const u32 k = 0;
    std::vector<u32> jstate(SBV_K256_STATE_WORDS), tmp(SBV_K256_WINDOW_TMP);
    std::vector<u32> bases((size_t)SBV_GTAB_WINDOWS * SBV_K256_BASES_STRIDE);
    memset((void*)tab, 0, kPerKey * sizeof(kapt));
    const int chunks = 2;
    for (int c = 0; c < chunks; ++c) {
        const int j_first = SBV_GTAB_WINDOWS * c / chunks, j_end = SBV_GTAB_WINDOWS * (c + 1) / chunks;
        k256_quad_host q;
        k256_chain_run(q, tuples, k, g, jstate.data(), bases.data(), valid, j_first, j_end - 1);
        for (int j = j_first; j < j_end; ++j) {
            kapt* row = tab + (size_t)j * SBV_GTAB_PER_WINDOW;
            const u32* b2 = bases.data() + ((size_t)k * SBV_GTAB_WINDOWS + j) * SBV_K256_BASES_STRIDE;
            for (int which = 0; which < 2; ++which) {
                if (which == 1 && j == SBV_GTAB_WINDOWS - 1) continue;
                k256_rows_lane(b2, which, j == SBV_GTAB_WINDOWS - 1, tmp.data(), row);
            }
            if (j != SBV_GTAB_WINDOWS - 1)
                for (int a = 1; a <= 7; ++a) k256_fill_lane(a, tmp.data(), row);
        }
    }
}

// the host builder's 16-bit comb of a key (k256_keyed.h: k256_keyed_host_wide_window); false = not a point
bool host_wide(const uint8_t key[64], std::vector<kapt>& want) {
    u32 w[16];
    memcpy(w, key, 64);
    kfe x, y;
    if (!k256_key_load_words(w, x, y)) return false;
    want.resize(SBV_K256_WIDE_ENTRIES);
    memset((void*)want.data(), 0, SBV_K256_WIDE_COMB_BYTES);
    parallel(SBV_K256_WIDE_WINDOWS, [&](size_t j) { k256_keyed_host_wide_window(x, y, SBV_K256_WIDE_BITS, (int)j, want.data() + j * SBV_K256_WIDE_PER_WINDOW); });
    return true;
}
}  // namespace

extern "C" {

// a fresh cache of `cache_cap` slots and a pool of `pool_cap` combs (0 = the feature is off, as the library's default)
void sbvk256hot_reset(u32 cache_cap, u32 pool_cap, u32 min_hits) {
    S.release();
    S = State();
    S.K = cache_cap; S.W = pool_cap;
    if (min_hits) S.min_hits = min_hits;
    S.ktab = (kapt*)aligned_alloc(64, std::max<size_t>(1, cache_cap) * kPerKey * sizeof(kapt));
    if (pool_cap) {
        S.wtab = (kapt*)aligned_alloc(64, (size_t)pool_cap * SBV_K256_WIDE_COMB_BYTES);
        memset((void*)S.wtab, 0, (size_t)pool_cap * SBV_K256_WIDE_COMB_BYTES);      // a comb's top window holds one entry; the builder writes no other of it
    }
    S.kvalid.assign(cache_cap, 0);
    S.kwide.assign(cache_cap, kNone); S.khits.assign(cache_cap, 0); S.wowner.assign(pool_cap, kNone);
    S.plist.assign(2 * SBV_PROMOTE_MAX, kNone); S.elist.assign(SBV_PROMOTE_MAX, kNone);
}
// sbv_key_cache(SBV_SCHEME_SECP256K1, on): switching the cache off forgets it, and with it the promotions
void sbvk256hot_key_cache(int on) {
    S.cache_on = on != 0;
    if (!on) S.forget();
}
void sbvk256hot_min_hits(u32 min_hits) { if (min_hits) S.min_hits = min_hits; }

// One grouped batch.  stats (may be null): [0] groups, [1] lanes of the key-sorted list, [2] live lanes the wide pass served (hot[2]),
// [3] promoted keys, [4] wavefronts of the wide pass, [5] wavefronts of the 8-bit kernel with a live lane, [6] wavefronts without a live
// lane, [7] evictions so far.
void sbvk256hot_verify(const uint8_t* tuples_in, size_t n, uint8_t* bitmap, u32* stats) {
    memset(bitmap, 0, (n + 7) / 8);
    if (stats) memset(stats, 0, 8 * sizeof(u32));
    S.last_classes.clear();
    if (n == 0) return;
    uint8_t* tuples = (uint8_t*)aligned_alloc(64, (n * 160 + 63) & ~(size_t)63);
    memcpy(tuples, tuples_in, n * 160);
    const size_t cap = (n + 63) & ~(size_t)63;
    std::vector<u32> pr(8 * cap), u1(8 * cap), u2(8 * cap), qx(8 * cap), qy(8 * cap), sm(8 * cap);
    std::vector<uint8_t> ok(cap, 0);
    u32* rec = (u32*)aligned_alloc(64, cap * SBV_REC_WORDS * sizeof(u32));
    Scratch s{pr.data(), u1.data(), u2.data(), qx.data(), qy.data(), sm.data(), ok.data(), cap};
    s.rec = rec;
    parallel(n, [&](size_t i) { k256_prep_lane(TupleWords{tuples + 160 * i}, i, s); });
    // 1. groups by key, in first-appearance order
    std::map<std::string, u32> gidx;
    std::vector<u32> group_rep, grp_of_tuple(n), gcount;
    for (size_t i = 0; i < n; ++i) {
        const std::string key((const char*)tuples + 160 * i + 96, 64);
        auto it = gidx.find(key);
        if (it == gidx.end()) { it = gidx.emplace(key, (u32)group_rep.size()).first; group_rep.push_back((u32)i); gcount.push_back(0); }
        grp_of_tuple[i] = it->second;
        ++gcount[it->second];
    }
    const u32 groups = (u32)group_rep.size();
    std::vector<u32> counters(SBV_GROUP_COUNTERS, 0);
    GroupState g{};
    g.group_rep = group_rep.data(); g.gcount = gcount.data(); g.counters = counters.data(); g.max_groups = groups; g.sorted = 1;
    counters[0] = groups;
    // 2. the key-sorted list: the runs in group_sort_group_at order
    std::vector<std::vector<u32>> members(groups);
    for (size_t i = 0; i < n; ++i) members[grp_of_tuple[i]].push_back((u32)i);
    std::vector<u32> grp_idx, grp_of;
    const u32 rows = group_sort_rows(groups), P = group_sort_positions(groups);
    for (u32 p = 0; p < P; ++p) {
        const u32 k = group_sort_group_at(p, rows);
        if (k >= groups) continue;
        for (u32 t : members[k]) { grp_idx.push_back(t); grp_of.push_back(k); }
    }
    const u32 lanes = (u32)grp_idx.size();
    counters[1] = lanes;
    // the cache's lookup and insert: a key the cache knows keeps its slot; a new one takes the next slot, or a slot of the per-batch area
    std::vector<u32> tslot(groups);
    std::vector<uint8_t> cold(groups, 1);
    u32 overflow = 0;
    for (u32 k = 0; k < groups; ++k) {
        const std::string key((const char*)tuples + 160 * (size_t)group_rep[k] + 96, 64);
        auto it = S.cache_on ? S.index.find(key) : S.index.end();
        if (it != S.index.end()) { tslot[k] = it->second; cold[k] = 0; }
        else if (S.cache_on && S.slot_key.size() < S.K) { tslot[k] = (u32)S.slot_key.size(); S.index.emplace(key, tslot[k]); S.slot_key.push_back(key); }
        else tslot[k] = S.K + overflow++;
    }
    const u32 nslots = S.K + overflow;
    kapt* btab = (kapt*)aligned_alloc(64, std::max<size_t>(1, overflow) * kPerKey * sizeof(kapt));
    std::vector<uint8_t> kvalid(nslots, 0);
    memcpy(kvalid.data(), S.kvalid.data(), S.K);
    auto table_of = [&](u32 slot) -> kapt* { return slot < S.K ? S.ktab + (size_t)slot * kPerKey : btab + (size_t)(slot - S.K) * kPerKey; };
    // 3. the 8-bit combs of the cold groups
    parallel(groups, [&](size_t k) { if (cold[k]) build_comb(tuples, g, (u32)k, table_of(tslot[k]), &kvalid[tslot[k]]); });
    memcpy(S.kvalid.data(), kvalid.data(), S.K);
    // 4. the G lane
    std::vector<u32> gacc((size_t)SBV_K256_GACC_WORDS * cap);
    const kgcomb gc = kgcomb_make(g_comb16(), kGBits);
    parallel(lanes, [&](size_t L) { k256_gphase_lane_sorted(s, grp_idx[L], L, gc, gacc.data()); });
    // 5. the class lane (the launcher's hot_on: a pool, the cache on, the key-sorted list)
    const bool hot_on = S.W != 0 && S.cache_on;
    std::vector<uint8_t> wide(groups, 0);
    if (hot_on) {
        ++S.tick;
        S.hot[1] = S.hot[2] = S.hot[3] = 0;
        for (u32 k = 0; k < groups; ++k) {
            group_hot_class_lane(k, g, tslot.data(), cold.data(), S.K, S.kwide.data(), S.khits.data(), wide.data());
            if (wide[k]) ++counters[8];
        }
    }
    // 6. + 7. the wave rule, then the wide lane or the 8-bit lanes in two chunks
    const size_t waves = (lanes + 63) / 64;
    S.last_classes.assign(waves, SBV_Q_FULL);
    std::vector<u32> wlive(waves, 0);
    std::vector<uint8_t> acc(n, 0);
    parallel(waves, [&](size_t wv) {
        const size_t w0 = wv * 64, w1 = std::min<size_t>(lanes, w0 + 64);
        bool any_live = false, any_live_not_wide = false;
        for (size_t L = w0; L < w1; ++L) {
            const bool live = k256_lane_live(grp_of[L], groups, tslot.data(), nslots, kvalid.data());
            any_live = any_live || live;
            any_live_not_wide = any_live_not_wide || (live && !(hot_on && k256_lane_wide(grp_of[L], groups, wide.data())));
        }
        const bool is_wide = hot_on && counters[8] != 0 && k256_wave_is_wide(any_live, any_live_not_wide);
        S.last_classes[wv] = is_wide ? SBV_Q_WIDE : any_live ? SBV_Q_FULL : SBV_Q_NONE;
        for (size_t L = w0; L < w1; ++L) {
            const u32 t = grp_idx[L], grp = grp_of[L];
            const u32 slot = tslot[grp];
            bool v;
            if (is_wide) {
                bool live = k256_lane_live(grp, groups, tslot.data(), nslots, kvalid.data());
                if (live) ++wlive[wv];
                u32 w = live ? S.kwide[slot] : 0u;
                if (w >= S.W) { w = 0; live = false; }
                const kgcomb wc = {S.wtab + (size_t)w * SBV_K256_WIDE_ENTRIES, SBV_K256_WIDE_BITS, SBV_K256_WIDE_WINDOWS};
                v = k256_qphase_wide_lane(s, t, L, live, wc, gacc.data());
            } else {
                const int mid = SBV_GTAB_WINDOWS / 2;
                (void)k256_qphase_lane_sorted(s, t, L, 0, 1, table_of(slot), &kvalid[slot], gacc.data(), 0, mid, false);
                v = k256_qphase_lane_sorted(s, t, L, 0, 1, table_of(slot), &kvalid[slot], gacc.data(), mid, SBV_GTAB_WINDOWS, true);
            }
            acc[t] = v ? 1 : 0;
        }
    });
    for (size_t i = 0; i < n; ++i) if (acc[i] == 1) bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
    u32 nw = 0, nf = 0, nn = 0;
    for (size_t wv = 0; wv < waves; ++wv) {
        S.hot[2] += wlive[wv];
        if (S.last_classes[wv] == SBV_Q_WIDE) ++nw; else if (S.last_classes[wv] == SBV_Q_FULL) ++nf; else ++nn;
    }
    // 8. the tail
    if (hot_on) {
        if (S.tick % SBV_HOT_DECAY_EVERY == SBV_HOT_DECAY_EVERY - 1)
            for (u32 slot = 0; slot < S.K; ++slot) hot_decay_lane(slot, S.khits.data());
        for (u32 k = 0; k < groups; ++k)
            group_promote_select_lane(k, tslot.data(), S.kvalid.data(), S.K, S.kwide.data(), S.khits.data(), S.min_hits, S.W, S.hot, S.plist.data(), S.elist.data());
        {   // k_promote_evict, by one agent
            const u32 ncand = S.hot[3] < SBV_PROMOTE_MAX ? S.hot[3] : SBV_PROMOTE_MAX;
            if (ncand != 0) {
                std::vector<u32> taken((S.W + 31) / 32 + 1, 0);
                u32 entries = S.hot[1] < SBV_PROMOTE_MAX ? S.hot[1] : SBV_PROMOTE_MAX;
                u32 mc = 0, bh, bw;
                for (u32 c = 0; c < ncand; ++c) mc = std::max(mc, S.khits[S.elist[c]]);
                hot_evict_scan(S.khits.data(), S.wowner.data(), taken.data(), S.W, S.K, 0, 1, bh, bw);
                if (bh != kNone && hot_evict_ok(mc, bh)) {
                    for (u32 c = 0; c < ncand; ++c) {
                        hot_evict_scan(S.khits.data(), S.wowner.data(), taken.data(), S.W, S.K, 0, 1, bh, bw);
                        const u32 before = entries;
                        entries = hot_evict_commit(S.elist[c], bh, bw, S.khits.data(), S.kwide.data(), S.wowner.data(), taken.data(), entries, S.plist.data());
                        if (entries != before) ++S.evictions;
                    }
                    S.hot[1] = entries;
                }
            }
        }
        const u32 live_p = S.hot[1] < SBV_PROMOTE_MAX ? S.hot[1] : SBV_PROMOTE_MAX;
        for (u32 i = 0; i < live_p; ++i) {      // k_k256_promote_build
            const u32 slot = S.plist[2 * i], w = S.plist[2 * i + 1];
            if (slot >= S.K || w >= S.W) continue;
            const kapt* qtab = S.ktab + (size_t)slot * kPerKey;
            kapt* comb = S.wtab + (size_t)w * SBV_K256_WIDE_ENTRIES;
            parallel(SBV_K256_WIDE_WINDOWS, [&](size_t j) {
                std::vector<u32> tmp(SBV_K256_WIDE_TMP_WORDS);
                if (j == SBV_K256_WIDE_WINDOWS - 1) { k256_widetab_lane(qtab, SBV_K256_WIDE_LANES - 1, tmp.data(), comb); return; }
                for (u32 q = 0; q < SBV_K256_WIDE_RUNS_PER_WINDOW; ++q) k256_widetab_lane(qtab, (u32)j * SBV_K256_WIDE_RUNS_PER_WINDOW + q, tmp.data(), comb);
            });
        }
        for (u32 i = 0; i < live_p; ++i) {      // k_promote_publish
            const u32 slot = S.plist[2 * i];
            if (slot != kNone) { S.kwide[slot] = S.plist[2 * i + 1]; S.wowner[S.plist[2 * i + 1]] = slot; }
        }
    }
    if (stats) {
        stats[0] = groups; stats[1] = lanes; stats[2] = S.hot[2]; stats[3] = S.hot[0] < S.W ? S.hot[0] : S.W;
        stats[4] = nw; stats[5] = nf; stats[6] = nn; stats[7] = S.evictions;
    }
    free(tuples); free(rec); free(btab);
}

// per wavefront of the last batch's key-sorted list: 2 = the wide pass, 0 = the 8-bit kernel, 3 = no live lane (the 8-bit kernel writes
// its rejects; neither walk decides anything) — SBV_Q_WIDE / SBV_Q_FULL / SBV_Q_NONE
size_t sbvk256hot_wave_classes(uint8_t* out, size_t max) {
    const size_t m = std::min(max, S.last_classes.size());
    if (m) memcpy(out, S.last_classes.data(), m);
    return S.last_classes.size();
}
// the comb a key's cache slot owns (0xFFFFFFFF: none, 0xFFFFFFFE: the key is not cached) and the slot's hit count
u32 sbvk256hot_wide_of_key(const uint8_t key[64]) {
    auto it = S.index.find(std::string((const char*)key, 64));
    return it == S.index.end() ? 0xFFFFFFFEu : S.kwide[it->second];
}
u32 sbvk256hot_hits_of_key(const uint8_t key[64]) {
    auto it = S.index.find(std::string((const char*)key, 64));
    return it == S.index.end() ? 0xFFFFFFFFu : S.khits[it->second];
}
// the owner's key of comb `index`: 1 and the 64 bytes, or 0 when nobody owns it
int sbvk256hot_owner_key(u32 index, uint8_t out[64]) {
    if (index >= S.W || S.wowner[index] >= S.slot_key.size() || S.kwide[S.wowner[index]] != index) return 0;
    memcpy(out, S.slot_key[S.wowner[index]].data(), 64);
    return 1;
}
// entries of promoted comb `index` that differ from the host builder's comb of its owner's key; -1 = nobody owns it, -2 = no point
long sbvk256hot_comb_mismatches(u32 index) {
    uint8_t key[64];
    if (!sbvk256hot_owner_key(index, key)) return -1;
    std::vector<kapt> want;
    if (!host_wide(key, want)) return -2;
    const kapt* got = S.wtab + (size_t)index * SBV_K256_WIDE_ENTRIES;
    long bad = 0;
    for (size_t e = 0; e < want.size(); ++e)
        if (memcmp((const void*)(got + e), (const void*)&want[e], sizeof(kapt)) != 0) ++bad;
    return bad;
}

}  // extern "C"
