// ed_keyed_emul.cc — CPU TEST TIER ONLY: the registered-key Ed25519 step (consensus_amd/csrc/ed25519_keyed.h) lane by lane.
//
// Compiles the lanes the gfx950 kernels are built from with g++ and runs the four launches of the keyed step in launch order —
// expand, G phase, keyed Q phase (with the wavefront ballot that picks the 16-bit combs), finish — so the build container can diff
// the keyed step against the oracle without a GPU.  The registry combs come from the library's host builder (ed_keyed_host_comb), the
// 16-bit combs from the device builder lane (ed_widetab_lane).  Not part of libsbv.so, never shipped, not a fallback.
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../consensus_amd/csrc/ed25519_keyed.h"

using namespace sbv;

namespace {
constexpr int kBBits = 8;               // the emulator's comb of B: 32 windows of 128 entries (the device uses 20 bits; same walker)

struct Registry {
    std::vector<aniels> ktab;
    std::vector<uint8_t> kvalid, kenc;
    std::vector<uint8_t> wtab;          // 16-bit combs at SBV_ED_HOT_PITCH
    std::vector<u32> kwidx;
    u32 nkeys = 0;
};

void* aligned(size_t bytes) { return aligned_alloc(64, (bytes + 63) & ~(size_t)63); }

// the 16-bit comb of slot `slot` into comb `w`, by the device builder lane; one host thread per window
void build_wide(Registry& r, u32 slot, u32 w) {
    std::vector<std::thread> th;
    for (u32 j = 0; j < SBV_ED_HOT_WINDOWS; ++j)
        th.emplace_back([&, j] {
            std::vector<u32> tmp(SBV_ED_HOT_TMP_WORDS);
            for (u32 part = 0; part < SBV_ED_HOT_PARTS; ++part)
                ed_widetab_lane(r.ktab.data() + (size_t)slot * SBV_ED_KEYTAB_ENTRIES, j, part, tmp.data(), r.wtab.data() + (size_t)w * SBV_ED_HOT_COMB_BYTES);
        });
    for (auto& t : th) t.join();
}

void build_registry(Registry& r, const uint8_t* encs, size_t nkeys, const uint8_t* widen) {
    r.nkeys = (u32)nkeys;
    r.ktab.assign(nkeys * (size_t)SBV_ED_KEYTAB_ENTRIES, aniels());
    r.kvalid.assign(nkeys, 0);
    r.kenc.assign(encs, encs + 32 * nkeys);
    r.kwidx.assign(nkeys, SBV_ED_WIDE_NONE);
    std::vector<std::thread> th;
    for (size_t s = 0; s < nkeys; ++s)
        th.emplace_back([&, s] { r.kvalid[s] = ed_keyed_host_comb(encs + 32 * s, r.ktab.data() + s * SBV_ED_KEYTAB_ENTRIES) ? 1 : 0; });
    for (auto& t : th) t.join();
    u32 wide = 0;
    for (size_t s = 0; s < nkeys; ++s) if (widen && widen[s] && r.kvalid[s]) ++wide;
    r.wtab.assign((size_t)wide * SBV_ED_HOT_COMB_BYTES, 0);
    u32 w = 0;
    for (size_t s = 0; s < nkeys; ++s)
        if (widen && widen[s] && r.kvalid[s]) { build_wide(r, (u32)s, w); r.kwidx[s] = w++; }
}

const aniels* bcomb() {
    static aniels* tab = nullptr;
    if (!tab) {
        tab = new aniels[edcomb_entries(kBBits)];
        for (int j = 0; j < edcomb_windows(kBBits); ++j) build_ed_b_window(kBBits, j, tab + ((size_t)j << (kBBits - 1)));
    }
    return tab;
}

// G | keyed Q (64-lane wavefronts, the ballot of k_ed_keyed_qphase) | finish | pack over n expanded tuples
void verify_tuples(const Registry& r, const uint8_t* tuples, const u32* slots, size_t n, uint8_t* bitmap, unsigned long* wide_lanes) {
    u32* gacc = (u32*)aligned(n * SBV_ED_GACC_WORDS * sizeof(u32));
    std::vector<uint8_t> okb(n), acc(n);
    const edcomb bc = edcomb_make(bcomb(), kBBits);
    for (size_t i = 0; i < n; ++i) ed_gphase_lane(tuples, i, bc, gacc, n, okb.data(), true);
    const u32* kwidx = r.kwidx.empty() ? nullptr : r.kwidx.data();
    bool any_wide = false;
    for (size_t s = 0; s < r.nkeys; ++s) any_wide = any_wide || r.kwidx[s] != SBV_ED_WIDE_NONE;
    if (!any_wide) kwidx = nullptr;               // the library passes no index while no slot is wide
    for (size_t w0 = 0; w0 < n; w0 += 64) {
        const size_t w1 = w0 + 64 < n ? w0 + 64 : n;
        bool wide = true;
        for (size_t i = w0; i < w1; ++i) wide = wide && ed_keyed_slot_wide(slots[i], r.nkeys, kwidx);
        for (size_t i = w0; i < w1; ++i) {
            const bool v = ed_keyed_qphase_lane(tuples, i, slots[i], r.nkeys, r.ktab.data(), r.kvalid.data(), r.wtab.data(), kwidx, wide, gacc, okb.data());
            acc[i] = v ? SBV_ED_PENDING : 0;
        }
        if (wide && wide_lanes) *wide_lanes += w1 - w0;
    }
    for (size_t i0 = 0; i0 < n; i0 += SBV_ED_FINISH_T) ed_finish_lane(tuples, n, i0, gacc, n, acc.data(), true);
    memset(bitmap, 0, (n + 7) / 8);
    for (size_t i = 0; i < n; ++i) if (acc[i] == 1) bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
    free(gacc);
}
}  // namespace

extern "C" {

// records n x 96 (R | S | k) + slots against the registry of `nkeys` encodings; widen[s] != 0: slot s gets a 16-bit comb (widen may be
// null).  tuples_out (may be null): the expanded tuples.  Returns the lanes that ran the wide pass.
unsigned long sbvk_verify_keyed(const uint8_t* recs_in, const u32* slots_in, size_t n, const uint8_t* encs, size_t nkeys, const uint8_t* widen,
                                uint8_t* bitmap, uint8_t* tuples_out) {
    Registry r;
    build_registry(r, encs, nkeys, widen);
    uint8_t* recs = (uint8_t*)aligned(n * SBV_ED_REC_BYTES);
    uint8_t* tuples = (uint8_t*)aligned(n * 128);
    u32* slots = (u32*)aligned(n * sizeof(u32));
    memcpy(recs, recs_in, n * SBV_ED_REC_BYTES);
    memcpy(slots, slots_in, n * sizeof(u32));
    for (size_t i = 0; i < n; ++i) ed_keyed_expand_lane(recs, slots, i, r.nkeys, r.kenc.data(), tuples);
    unsigned long wide_lanes = 0;
    verify_tuples(r, tuples, slots, n, bitmap, &wide_lanes);
    if (tuples_out) memcpy(tuples_out, tuples, n * 128);
    free(recs); free(tuples); free(slots);
    return wide_lanes;
}

// the _msgs_keyed form: sigs n x 64, messages msgs[offs[i] .. offs[i+1]), slots -> tuples by the keyed front end lane, then the same step
void sbvk_verify_msgs_keyed(const uint8_t* sigs, const uint8_t* msgs, const uint64_t* offs, const u32* slots, size_t n, const uint8_t* encs,
                            size_t nkeys, uint8_t* bitmap) {
    Registry r;
    build_registry(r, encs, nkeys, nullptr);
    uint8_t* tuples = (uint8_t*)aligned(n * 128);
    for (size_t i = 0; i < n; ++i)
        ed_keyed_msg_frontend_lane(sigs + 64 * i, slots[i], r.nkeys, r.kenc.data(), msgs + offs[i], (size_t)(offs[i + 1] - offs[i]),
                                   reinterpret_cast<u32*>(tuples + 128 * i));
    verify_tuples(r, tuples, slots, n, bitmap, nullptr);
    free(tuples);
}

// the registry comb of `enc` (32 x 128 entries, 96 bytes each); returns the valid flag
int sbvk_host_comb(const uint8_t enc[32], uint8_t* out) {
    std::vector<aniels> tab(SBV_ED_KEYTAB_ENTRIES);
    const bool ok = ed_keyed_host_comb(enc, tab.data());
    memcpy(out, tab.data(), tab.size() * sizeof(aniels));
    return ok ? 1 : 0;
}

// entries of the 16-bit comb the device builder lane makes from the registry comb of `enc` that differ from the host reference
// builder's (build_ed_window_of on -A at 16 bits); -1 = not a point
long sbvk_wide_mismatches(const uint8_t enc[32]) {
    Registry r;
    const uint8_t one = 1;
    build_registry(r, enc, 1, &one);
    if (!r.kvalid[0]) return -1;
    u32 w[8];
    memcpy(w, enc, 32);
    ept A;
    ed_decompress(A, w);
    fe25_neg(A.X, A.X);
    fe25_neg(A.T, A.T);
    std::vector<aniels> want((size_t)SBV_ED_HOT_WINDOWS * SBV_ED_HOT_PER_WINDOW);
    std::vector<std::thread> th;
    for (int j = 0; j < SBV_ED_HOT_WINDOWS; ++j)
        th.emplace_back([&, j] { build_ed_window_of(A, SBV_ED_HOT_BITS, j, want.data() + (size_t)j * SBV_ED_HOT_PER_WINDOW); });
    for (auto& t : th) t.join();
    long bad = 0;
    for (size_t e = 0; e < want.size(); ++e)
        if (memcmp(r.wtab.data() + e * SBV_ED_HOT_PITCH, &want[e], sizeof(aniels)) != 0) ++bad;
    return bad;
}

}  // extern "C"
