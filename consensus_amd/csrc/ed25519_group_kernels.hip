// ed25519_group_kernels.hip — the grouped step of the Ed25519 variant (ed25519_group.h), same stream layout
// as the P-256 one (p256_group_kernels.hip):
//
//   stream: [S]B for every tuple ........ wait(split, tables c) Q-phase chunk c ... wait(generic) pack
//   side_a: insert assign | bases chunk 0 | bases chunk 1 | ... | wait(split) one-lane kernel over the ungrouped list
//   side_b:        wait(assign) split | wait(bases c) windows chunk c ...
//
// No stage A here (Ed25519 has no scalar inversion), so the G phase starts at once.  Unlike P-256 the ungrouped
// list is never empty on the headline-shaped batch (half of all corrupted keys still decompress), so its 2.5 ms
// chain runs on side_a where it gates only the final pack.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "ed25519_group.h"
#include "ed25519_keyed.h"
#include "ed25519_kernels.h"
#include "group_kernels_common.h"
#include "p256_kernels.h"

namespace sbv {

#ifndef SBV_ED_QPHASE_WAVES
#define SBV_ED_QPHASE_WAVES 3
#endif
#ifndef SBV_ED_GROUP_WAVES
#define SBV_ED_GROUP_WAVES 2      // waves/SIMD the comb kernels are compiled for: 234 VGPRs and no scratch at 2; 168 + 268 B of spills at 3, same speed (profiles/r02/ed25519_ab_r02.txt)
#endif

// The ungrouped list is a few hundred wavefronts of one long serial chain each (key check, then the one-lane kernel) beside the
// throughput kernels; once a scheme's combs are cached it is the step's critical path.  SBV_ED_CHAIN_PRIO > 0 raises those wavefronts'
// priority at their SIMD's arbiter (s_setprio).
#ifndef SBV_ED_CHAIN_PRIO
#define SBV_ED_CHAIN_PRIO 0
#endif
static __device__ __forceinline__ void ed_chain_prio() {
#if SBV_ED_CHAIN_PRIO > 0
    __builtin_amdgcn_s_setprio(SBV_ED_CHAIN_PRIO);
#endif
}

// Same result as ed_group_split_lane (compaction: group_split_emit)
__global__ __launch_bounds__(256) void k_ed_group_split(size_t n, GroupState g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    u32 s = SBV_GROUP_NONE;
    if (active) s = g.slot_of[g.rep[i]];
    group_split_emit(i, s, active && s == SBV_GROUP_NONE, active && s != SBV_GROUP_NONE, false, g);
}

// only the groups whose tables are built in this batch (cold: not found in the key-table cache).  Four lanes per key (ed25519_group.h:
// edchain_run, exchange policy edchain_quad_dev); a quad lives or exits as a whole.
__global__ __launch_bounds__(64) void k_ed_keytab_bases(const uint8_t* __restrict__ tuples, GroupState g, u32* __restrict__ jbases,
                                                        uint8_t* __restrict__ valid, const u32* __restrict__ tslot, const uint8_t* __restrict__ cold,
                                                        int j_first, int j_last) {
    const u32 lane = blockIdx.x * 64 + threadIdx.x;
    const u32 k = lane >> 2;
    if (k >= group_count(g) || !cold[k]) return;
    edchain_quad_dev q;
    q.r = (int)(lane & 3u);
    edchain_run(q, tuples, k, g, jbases, valid + tslot[k], j_first, j_last);
}

// lanes = groups x j_count x parts
__global__ __launch_bounds__(64) void k_ed_keytab_window(GroupState g, const u32* __restrict__ jbases, u32* __restrict__ tmp,
                                                         aniels* __restrict__ ktab, const u32* __restrict__ tslot, const uint8_t* __restrict__ cold,
                                                         int j_first, int j_count, int parts) {
    const u32 lane = blockIdx.x * 64 + threadIdx.x;
    const u32 part = lane % (u32)parts;
    const u32 kw = lane / (u32)parts;
    const u32 key = kw / (u32)j_count, j = (u32)j_first + kw % (u32)j_count;
    if (key >= group_count(g) || !cold[key]) return;
    const size_t w = (size_t)key * SBV_ED_KEY_WINDOWS + j;
    ed_keytab_window_lane(jbases + w * SBV_ED_JBASE_DWORDS, (int)part, parts,
                          tmp + w * (size_t)(SBV_ED_KEY_PER_WINDOW * SBV_ED_WINDOW_TMP_WORDS) + (size_t)part * (SBV_ED_KEY_PER_WINDOW / parts) * SBV_ED_WINDOW_TMP_WORDS,
                          ktab + ((size_t)tslot[key] * SBV_ED_KEY_WINDOWS + j) * SBV_ED_KEY_PER_WINDOW);
}

// The one-lane kernel (ed25519_verify_lane) over the ungrouped list, at the 3 waves/SIMD budget of the throughput
// kernels it runs beside.  A ~2.5 ms serial chain per lane: it goes on side_a behind the last bases so that it
// gates nothing but the final pack.
#ifndef SBV_ED_ONE_WAVES
#define SBV_ED_ONE_WAVES SBV_ED_GROUP_WAVES
#endif
// ungxy (may be null): the keys as the key check decompressed them (key-sorted step)
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_ONE_WAVES) void k_ed_generic_list(const uint8_t* __restrict__ tuples, GroupState g,
                                                                        u32* __restrict__ qtab, const aniels* __restrict__ btab,
                                                                        uint8_t* __restrict__ acc, const u32* __restrict__ ungxy) {
    const u32 L = blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (L >= g.counters[2]) return;
    ed_chain_prio();
    const u32 t = g.ung_idx[L];
    acc[t] = ed25519_verify_lane(EdGlobalTuple{ed_tuple_words(tuples, t)}, qtab + (size_t)L * (SBV_ED_QTAB_ENTRIES * SBV_ED_PT_WORDS), btab,
                                 ungxy ? ungxy + (size_t)L * SBV_ED_UNGXY_WORDS : nullptr) ? 1 : 0;
}

// key-sorted step, pass 2: the ungrouped candidates whose key is a point -> ung_idx (ed25519_group.h: ed_group_keycheck_lane)
__global__ __launch_bounds__(256) void k_ed_keycheck(const uint8_t* __restrict__ tuples, GroupState g, uint8_t* __restrict__ acc, u32* __restrict__ ungxy) {
    const u32 L = blockIdx.x * 256 + threadIdx.x;
    const u32 cands = g.counters[4];
    if (blockIdx.x * 256u >= cands) return;            // whole workgroup idle (uniform: the barriers below are not reached by anyone)
    ed_chain_prio();
    const bool active = L < cands;
    u32 i = 0;
    bool ok = false;
    ept A;
    if (active) {
        i = g.ung_cand[L];
        ok = ed_tuple_key_load(tuples, i, A);
        if (!ok) acc[i] = 0;
    }
    const unsigned long long mr = __ballot(active && !ok);
    if ((threadIdx.x & 63) == 0 && mr) atomicAdd(&g.counters[3], (u32)__popcll(mr));
    const u32 pos = group_compact_pos(active && ok, &g.counters[2]);
    if (active && ok) {
        g.ung_idx[pos] = i;
        if (ungxy) { fe25_store_raw(ungxy + (size_t)pos * SBV_ED_UNGXY_WORDS, A.X); fe25_store_raw(ungxy + (size_t)pos * SBV_ED_UNGXY_WORDS + 10, A.Y); }
    }
}
// The ungrouped list on four lanes per tuple (ed25519_group.h: ed25519_verify_quad): 4 x as many wavefronts, each a chain a third as long
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_GROUP_WAVES) void k_ed_generic_quad(const uint8_t* __restrict__ tuples, GroupState g, const u32* __restrict__ ungxy,
                                                                        u32* qtab, const aniels* __restrict__ btab, uint8_t* __restrict__ acc) {
    const u32 lane = blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    const u32 L = lane >> 2;
    if (L >= g.counters[2]) return;                   // a quad lives or leaves as a whole
    const u32 t = g.ung_idx[L];
    edchain_quad_dev q;
    q.r = (int)(lane & 3u);
    bool v[1];
    ed25519_verify_quad(q, EdGlobalTuple{ed_tuple_words(tuples, t)}, ungxy + (size_t)L * SBV_ED_UNGXY_WORDS, qtab + (size_t)L * (SBV_ED_QTAB_ENTRIES * SBV_ED_PT_WORDS), btab, v);
    if (q.r == 0) acc[t] = v[0] ? 1 : 0;
}

// [S]B for every tuple of the batch
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_GROUP_WAVES) void k_ed_gphase(const uint8_t* __restrict__ tuples, size_t n, edcomb btab,
                                                                  u32* __restrict__ gacc, size_t cap, uint8_t* __restrict__ okb, int tuple_major) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i < n) ed_gphase_lane(tuples, i, btab, gacc, cap, okb, tuple_major != 0);
}

// Round 6: the key-sorted form and the compaction-order form are kernels of their own, LAST is a template parameter (what the P-256 Q
// phase gained from the same split: each form alone needs far fewer registers than the kernel that held them all)
// hot keys: does every (active) lane of this wavefront belong to a group whose cache slot owns a 16-bit comb?
__device__ __forceinline__ bool ed_wave_is_wide(u32 grp, const GroupState& g, const uint8_t* __restrict__ wide) {
    const bool w = grp < group_count(g) && wide[grp] != 0;
    return __ballot(w) == __ballot(true);
}
template <bool LAST>
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_QPHASE_WAVES) void k_ed_qphase(const uint8_t* __restrict__ tuples, GroupState g,
                                                                  const aniels* __restrict__ ktab, const uint8_t* __restrict__ kvalid,
                                                                  const u32* __restrict__ tslot, u32 table_slots,
                                                                  u32* __restrict__ gacc, size_t cap, const uint8_t* __restrict__ okb,
                                                                  uint8_t* __restrict__ acc, int j0, int j1, const uint8_t* __restrict__ wide) {
    // key-sorted list, XCD-aware block order (see k_verify_keyed_q): block b takes logical block (b % 8) * per + b / 8
    const u32 lanes = g.counters[1];
    const u32 per = ((lanes + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK + 7) >> 3;
    const u32 local = blockIdx.x >> 3;
    if (local >= per) return;
    const u32 L = ((blockIdx.x & 7u) * per + local) * SBV_VERIFY_BLOCK + threadIdx.x;
    if (L >= lanes) return;
    const u32 t = g.grp_idx[L];
    const u32 grp = g.grp_of[L];
    if (wide && ed_wave_is_wide(grp, g, wide)) return;                // every lane's key owns a 16-bit comb: k_ed_qphase_wide's wavefront
    const bool v = ed_qphase_lane(tuples, t, grp < group_count(g) ? tslot[grp] : SBV_GROUP_NONE, table_slots, ktab, kvalid, gacc, cap, okb, j0, j1, LAST, true);
    if (LAST) acc[t] = v ? SBV_ED_PENDING : 0;
}
// The wide pass (ed25519_group.h: hot keys): the wavefronts of the key-sorted list whose lanes ALL belong to promoted cache slots —
// [k](-A) in 16 additions from the slot's comb, one launch that needs no table of this batch; it leaves the tuple pending for k_ed_finish
// as the last chunk's launch does for everybody else.  Same block order as k_ed_qphase: the two kernels split the same wavefronts.
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_GROUP_WAVES) void k_ed_qphase_wide(const uint8_t* __restrict__ tuples, GroupState g,
                                                                  const uint8_t* __restrict__ kvalid, const u32* __restrict__ tslot,
                                                                  const uint8_t* __restrict__ wide, const u32* __restrict__ kwide,
                                                                  const uint8_t* __restrict__ wtab, u32* __restrict__ wstat,
                                                                  u32* __restrict__ gacc, const uint8_t* __restrict__ okb, uint8_t* __restrict__ acc) {
    if (g.counters[8] == 0) return;                                   // no group of this batch owns a comb
    const u32 lanes = g.counters[1];
    const u32 per = ((lanes + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK + 7) >> 3;
    const u32 local = blockIdx.x >> 3;
    if (local >= per) return;
    const u32 L = ((blockIdx.x & 7u) * per + local) * SBV_VERIFY_BLOCK + threadIdx.x;
    if (L >= lanes) return;
    const u32 t = g.grp_idx[L];
    const u32 grp = g.grp_of[L];
    if (!ed_wave_is_wide(grp, g, wide)) return;
    const unsigned long long am = __ballot(true);
    if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)am) - 1u) atomicAdd(wstat, (u32)__popcll(am));     // statistics: lanes of the wide pass
    const u32 slot = tslot[grp];                                      // a cache slot: wide[grp] says so
    const bool v = ed_qphase_wide_lane(tuples, t, kvalid[slot] != 0, wtab + (size_t)kwide[slot] * SBV_ED_HOT_COMB_BYTES, gacc, okb);
    acc[t] = v ? SBV_ED_PENDING : 0;
}
// The builder of this batch's promotions: lane (promotion i, window j, part) writes 32 entries of comb plist[2 i + 1] from the base point
// the slot's 8-bit comb holds (ed25519_group.h: ed_widetab_lane).  A bounded grid walks the promotions' 16 x 1024 lanes each; scratch
// is per resident lane.
__global__ __launch_bounds__(64) void k_ed_promote_window(const u32* __restrict__ plist, const u32* __restrict__ hot, const aniels* __restrict__ ktab,
                                                          u32* __restrict__ tmp, uint8_t* __restrict__ wtab) {
    const u32 total = promote_live(hot) * (SBV_ED_HOT_WINDOWS * SBV_ED_HOT_PARTS);
    const u32 gid = blockIdx.x * 64 + threadIdx.x;
    u32* mine = tmp + (size_t)gid * SBV_ED_HOT_TMP_WORDS;
    for (u32 item = gid; item < total; item += gridDim.x * 64) {
        const u32 part = item % SBV_ED_HOT_PARTS, j = (item / SBV_ED_HOT_PARTS) % SBV_ED_HOT_WINDOWS, i = item / (SBV_ED_HOT_PARTS * SBV_ED_HOT_WINDOWS);
        const u32 slot = plist[2 * i];
        if (slot == 0xFFFFFFFFu) continue;
        ed_widetab_lane(ktab + (size_t)slot * SBV_ED_KEYTAB_ENTRIES, j, part, mine, wtab + (size_t)plist[2 * i + 1] * SBV_ED_HOT_COMB_BYTES);
    }
}
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_GROUP_WAVES) void k_ed_qphase_list(const uint8_t* __restrict__ tuples, GroupState g,
                                                                  const aniels* __restrict__ ktab, const uint8_t* __restrict__ kvalid,
                                                                  const u32* __restrict__ tslot, u32 table_slots,
                                                                  u32* __restrict__ gacc, size_t cap, const uint8_t* __restrict__ okb,
                                                                  uint8_t* __restrict__ acc, int j0, int j1, int last) {
    const u32 L = blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (L >= g.counters[1]) return;
    const u32 t = g.grp_idx[L];
    const u32 grp = g.slots[t];
    const bool v = ed_qphase_lane(tuples, t, grp < group_count(g) ? tslot[grp] : SBV_GROUP_NONE, table_slots, ktab, kvalid, gacc, cap, okb, j0, j1, last != 0);
    if (last) acc[t] = v ? SBV_ED_PENDING : 0;
}

// encode(R) == R_enc for the tuples the last Q chunk left pending: a lane takes SBV_ED_FINISH_T consecutive tuples and ONE
// inversion (ed25519_group.h: ed_finish_lane).  Few registers, 2^20 / 8 lanes: every wavefront of it is resident at once.
__global__ __launch_bounds__(256) void k_ed_finish(const uint8_t* __restrict__ tuples, size_t n, u32* __restrict__ gacc, size_t cap,
                                                   uint8_t* __restrict__ acc, int tuple_major) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * SBV_ED_FINISH_T;
    if (i0 < n) ed_finish_lane(tuples, n, i0, gacc, cap, acc, tuple_major != 0);
}

hipError_t launch_ed25519_verify_grouped(const uint8_t* d_tuples, size_t n, const GroupBuffers& b, const EdGroupBuffers& eb,
                                         u32* d_qtab, const aniels* d_btab, const edcomb& bcomb, uint8_t* d_bitmap, hipStream_t stream,
                                         const GroupSync& y, hipEvent_t* prof, int* prof_pairs) {
    if (n == 0) return hipSuccess;
    GroupState g = group_state_of(b);
    // key-sorted grouped list (p256_group.h): the Q phase walks runs of equal keys; the accumulator is tuple-major so that the
    // G phase can still start at once, in tuple order
    const size_t sort_lds = (size_t)b.max_groups * sizeof(u32);
    g.sorted = ed25519_group_step_sorted(y, b) ? 1u : 0u;
    group_set_threshold(g, b.min_count);
    // 2 chunks (the context's setting) also after the finish left the Q phase: 3 / 4 chunks 4.41-4.51 / 4.36-4.45 ms against 4.19-4.33 per cold 2^20
    // step, 3.33-3.35 / 3.38-3.42 against 3.20-3.23 warm (profiles/r04/ab_ed_chunks_r04o.jsonl)
    const int chunks = y.chunks < 1 ? 1 : (y.chunks > SBV_GROUP_MAX_CHUNKS ? SBV_GROUP_MAX_CHUNKS : y.chunks);
    const int parts = SBV_KEYTAB_PARTS_DEFAULT;     // lanes per (key, window) of the table kernel (2 / 4 / 8 / 16 measured in round 2)
    // this scheme's comb pool: slots of aniels combs of -A; hot keys (ed25519_group.h) only with the class bytes that exist with the pool
    const KeyPool& kp = eb.kp;
    aniels* const ktab = static_cast<aniels*>(kp.ktab);
    const u32 table_slots = kp.kc.cap + b.max_groups;
    const HotPool& hp = kp.hp;
    uint8_t* const wtab = static_cast<uint8_t*>(hp.wtab);
    const GroupHot hot = group_hot_of(hp, kp.kc, g, kp.wide != nullptr, kp.wide);
    const bool hot_on = hot.on;
    const uint8_t* wide = hot.wide;
    const unsigned gn = (unsigned)((n + 255) / 256);
    const unsigned gv = (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK);
    // side_a: the head; acc is cleared too: no stale "pending" marker can survive a batch that was cut short
    SBV_TRY((group_launch_head<128, 64, 8>(d_tuples, n, g, b, kp.kc, y, hot_on, b.acc)));
    // side_b: no key check in front of the sort (it sits on side_a, below)
    SBV_TRY(group_launch_split(n, g, b, hot, sort_lds, y, [] {}));
    if (!g.sorted) hipLaunchKernelGGL(k_ed_group_split, dim3(gn), dim3(256), 0, y.side_b, n, g);
    SBV_TRY(group_launch_hot_class(g, b, hot, y));
    SBV_TRY(hipEventRecord(y.ev_split, y.side_b));
    // stream: the G phase needs nothing but the tuples.  (Holding it back until the grouping's first kernels are through, so that the head
    // of the table pipeline does not share the CUs with it, was measured in round 6 and changes nothing: 3.84 against 3.81 ms cold.)
    hipLaunchKernelGGL(k_ed_gphase, dim3(gv), dim3(SBV_VERIFY_BLOCK), 0, stream, d_tuples, n, bcomb, b.gacc, b.gacc_cap, eb.okb, (int)g.sorted);
    if (hot_on) SBV_TRY(hipEventRecord(y.ev_class, stream));            // the G phase is enqueued: the wide pass (side_b) adds to its sums
    SBV_TRY(hipStreamWaitEvent(stream, y.ev_split, 0));
    // side_a: the doubling chains of every chunk, then the ungrouped list
    for (int c = 0; c < chunks; ++c) {
        const int j_first = SBV_ED_KEY_WINDOWS * c / chunks, j_end = SBV_ED_KEY_WINDOWS * (c + 1) / chunks;
        hipLaunchKernelGGL(k_ed_keytab_bases, dim3((b.max_groups * 4u + 63) / 64), dim3(64), 0, y.side_a, d_tuples, g, b.jbases, kp.kvalid,
                           b.tslot, b.cold, j_first, j_end - 1);
        SBV_TRY(hipEventRecord(y.ev_bases[c], y.side_a));
    }
    SBV_TRY(hipStreamWaitEvent(y.side_a, y.ev_split, 0));
    // the candidates whose key is a point -> ung_idx, right in front of the kernel that needs it: on side_b before the sort it held
    // up the first table windows (4.33 ms per cold 2^20 step against 4.08 here; without any key check 4.52: profiles/r04/ab_ed_keycheck_r04n.jsonl)
    // the ungrouped list on four lanes per tuple (the key check hands over the decompressed keys); SBV_ED_UNGROUPED_QUAD=0: the one-lane kernel
    static const bool quad_env = [] { const char* e = getenv("SBV_ED_UNGROUPED_QUAD"); return e && atoi(e) != 0; }();
    static const bool keep_keys = [] { const char* e = getenv("SBV_ED_UNGROUPED_KEYS"); return !e || atoi(e) != 0; }();
    const u32* ungxy = keep_keys && g.sorted ? eb.ungxy : nullptr;     // the key check keeps the keys it decompressed
    const bool quad = quad_env && ungxy;
    if (g.sorted) hipLaunchKernelGGL(k_ed_keycheck, dim3(gn), dim3(256), 0, y.side_a, d_tuples, g, b.acc, const_cast<u32*>(ungxy));
    // Once the combs are cached the one-lane kernel's chain (1.1 ms alone) is the step's critical path, and the key check in front of it
    // took 0.7 ms instead of 0.1 whenever its workgroups had to queue up behind those of the first Q launch (timeline_ed_hot_r06x.txt):
    // that launch now waits for the key check.  A cold step's first Q launch waits for tables anyway.
    static const bool keycheck_first = [] { const char* e = getenv("SBV_ED_KEYCHECK_FIRST"); return !e || atoi(e) != 0; }();
    if (g.sorted && keycheck_first) {
        SBV_TRY(hipEventRecord(y.ev_narrow, y.side_a));
        SBV_TRY(hipStreamWaitEvent(stream, y.ev_narrow, 0));
    }
    if (quad) hipLaunchKernelGGL(k_ed_generic_quad, dim3(4 * gv), dim3(SBV_VERIFY_BLOCK), 0, y.side_a, d_tuples, g, ungxy, d_qtab, d_btab, b.acc);
    else hipLaunchKernelGGL(k_ed_generic_list, dim3(gv), dim3(SBV_VERIFY_BLOCK), 0, y.side_a, d_tuples, g, d_qtab, d_btab, b.acc, ungxy);
    SBV_TRY(hipEventRecord(y.ev_generic, y.side_a));
    // (an uneven split — a first chunk of 6-12 windows so that the first Q launch starts earlier — was measured in round 5 and loses:
    // 4.11-4.46 ms per cold 2^20 step against 4.08-4.12, profiles/r05/ab_ed_chunk0_r05m.jsonl)
    for (int c = 0; c < chunks; ++c) {
        const int j_first = SBV_ED_KEY_WINDOWS * c / chunks, j_end = SBV_ED_KEY_WINDOWS * (c + 1) / chunks;
        const int j_count = j_end - j_first;
        hipStream_t tb = y.side_b;      // one table stream: the windows of the odd chunks on a second stream measured slower (round 4: 4.55 -> 4.67 ms)
        SBV_TRY(hipStreamWaitEvent(tb, y.ev_bases[c], 0));
        const size_t wl = (size_t)b.max_groups * j_count * parts;
        hipLaunchKernelGGL(k_ed_keytab_window, dim3((unsigned)((wl + 63) / 64)), dim3(64), 0, tb, g, b.jbases, b.tmp, ktab,
                           b.tslot, b.cold, j_first, j_count, parts);
        SBV_TRY(hipEventRecord(y.ev_tables[c], tb));
        SBV_TRY(hipStreamWaitEvent(stream, y.ev_tables[c], 0));
        if (prof) SBV_TRY(hipEventRecord(prof[2 * c], stream));
        if (!g.sorted) hipLaunchKernelGGL(k_ed_qphase_list, dim3(gv), dim3(SBV_VERIFY_BLOCK), 0, stream, d_tuples, g, ktab, kp.kvalid, b.tslot, table_slots, b.gacc, b.gacc_cap,
                                          eb.okb, b.acc, j_first, j_end, c + 1 == chunks ? 1 : 0);
        else if (c + 1 == chunks) hipLaunchKernelGGL(k_ed_qphase<true>, dim3((gv + 7u) & ~7u), dim3(SBV_VERIFY_BLOCK), 0, stream, d_tuples, g, ktab, kp.kvalid, b.tslot, table_slots,
                                                     b.gacc, b.gacc_cap, eb.okb, b.acc, j_first, j_end, wide);
        else hipLaunchKernelGGL(k_ed_qphase<false>, dim3((gv + 7u) & ~7u), dim3(SBV_VERIFY_BLOCK), 0, stream, d_tuples, g, ktab, kp.kvalid, b.tslot, table_slots,
                                b.gacc, b.gacc_cap, eb.okb, b.acc, j_first, j_end, wide);
        if (prof) SBV_TRY(hipEventRecord(prof[2 * c + 1], stream));
    }
    if (hot_on) {
        // The wide pass, on side_b behind this batch's table windows (none in a warm batch) and beside the chunks' launches: it needs the G
        // phase and the classes, no table.  On `stream` in front of the chunks' launches a batch with SOME hot signers ran three launches
        // in a row, each over a part of the lanes (half-hot 2^18: 1.45 ms against 1.31 from the 8-bit combs alone, ed_hot_sweep_r06al).
        // Like the first Q launch it lets the ungrouped list's key check go first.
        SBV_TRY(hipStreamWaitEvent(y.side_b, y.ev_class, 0));
        if (g.sorted && keycheck_first) SBV_TRY(hipStreamWaitEvent(y.side_b, y.ev_narrow, 0));
        hipLaunchKernelGGL(k_ed_qphase_wide, dim3((gv + 7u) & ~7u), dim3(SBV_VERIFY_BLOCK), 0, y.side_b, d_tuples, g, kp.kvalid, b.tslot, wide, hp.kwide, wtab,
                           hp.hot + 2, b.gacc, eb.okb, b.acc);
        SBV_TRY(hipEventRecord(y.ev_wide, y.side_b));
        SBV_TRY(hipStreamWaitEvent(stream, y.ev_wide, 0));
    }
    {   // the pending tuples' encodings: one inversion per SBV_ED_FINISH_T tuples
        const size_t fl = (n + SBV_ED_FINISH_T - 1) / SBV_ED_FINISH_T;
        hipLaunchKernelGGL(k_ed_finish, dim3((unsigned)((fl + 255) / 256)), dim3(256), 0, stream, d_tuples, n, b.gacc, b.gacc_cap, b.acc, (int)g.sorted);
    }
    // the tail on side_b: in stream order behind this batch's table windows and its wide pass
    SBV_TRY(group_launch_promote_select(g, b, kp.kvalid, hp, hot, y, false, [] {}));
    if (hot_on) {
        hipLaunchKernelGGL(k_ed_promote_window, dim3(SBV_ED_HOT_BUILD_BLOCKS), dim3(64), 0, y.side_b, hp.plist, hp.hot, ktab, hp.ptmp, wtab);
        group_launch_promote_publish(hp, y);
    }
    SBV_TRY(hipStreamWaitEvent(stream, y.ev_generic, 0));
    hipLaunchKernelGGL(k_pack_bitmap, dim3((unsigned)(((n + 7) / 8 + 255) / 256)), dim3(256), 0, stream, b.acc, n, d_bitmap);
    if (prof && prof_pairs) *prof_pairs = chunks;
    return hipGetLastError();
}

// ---- registered keys (ed25519_keyed.h): expand | G phase | keyed Q phase | finish ------------------------------------------------------
// records R | S | k + slots -> 128-byte tuples, A from the registry
__global__ __launch_bounds__(256) void k_ed_keyed_expand(const uint8_t* __restrict__ recs, const u32* __restrict__ slots, size_t n, u32 nkeys,
                                                         const uint8_t* __restrict__ kenc, uint8_t* __restrict__ tuples) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ed_keyed_expand_lane(recs, slots, i, nkeys, kenc, tuples);
}
// the keyed twin of k_ed_msg_frontend (ed25519_kernels.hip): signatures n x 64, messages msgs[moff[i] .. moff[i+1]), A from the registry
__global__ __launch_bounds__(256) void k_ed_keyed_msg_frontend(const uint8_t* __restrict__ sigs, const u32* __restrict__ slots, u32 nkeys,
                                                               const uint8_t* __restrict__ kenc, const uint8_t* __restrict__ msgs,
                                                               const u64* __restrict__ moff, size_t n, u32* __restrict__ tuples) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 m0 = moff[i], m1 = moff[i + 1];
    u32 rec[32];
    ed_keyed_msg_frontend_lane(sigs + i * 64, slots[i], nkeys, kenc, msgs + m0, (size_t)(m1 - m0), rec);
    ed_q4* t = reinterpret_cast<ed_q4*>(tuples + i * 32);
    SBV_UNROLL
    for (int q = 0; q < 8; ++q) { const ed_q4 v = {rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]}; t[q] = v; }
}
// [k](-A) for every tuple from its slot's registry comb, one launch: a wavefront whose lanes all own a 16-bit comb walks those (16
// additions), any other the 8-bit combs (32).  Leaves the survivors pending for k_ed_finish.
#ifndef SBV_ED_KEYED_WAVES
#define SBV_ED_KEYED_WAVES SBV_ED_GROUP_WAVES
#endif
__global__ __launch_bounds__(SBV_VERIFY_BLOCK, SBV_ED_KEYED_WAVES) void k_ed_keyed_qphase(const uint8_t* __restrict__ tuples, const u32* __restrict__ slots, size_t n,
                                                                  EdKeyedRegistry r, u32* __restrict__ gacc, const uint8_t* __restrict__ okb,
                                                                  uint8_t* __restrict__ acc) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 slot = slots[i];
    const bool w = ed_keyed_slot_wide(slot, r.nkeys, r.kwidx);
    const bool wide = __ballot(w) == __ballot(true);
    const bool v = ed_keyed_qphase_lane(tuples, i, slot, r.nkeys, r.ktab, r.kvalid, r.wtab, r.kwidx, wide, gacc, okb);
    acc[i] = v ? SBV_ED_PENDING : 0;
}
// the 16-bit combs of `count` widened slots: plist = (slot, comb) pairs; lane (key, window, part) writes 32 entries (ed_widetab_lane),
// a bounded grid walks the 16 x 1024 items per key; tmp = SBV_ED_HOT_TMP_WORDS per lane of the grid
__global__ __launch_bounds__(64) void k_ed_keyed_widen(const u32* __restrict__ plist, u32 count, const aniels* __restrict__ ktab,
                                                       u32* __restrict__ tmp, uint8_t* __restrict__ wtab) {
    const u32 total = count * (SBV_ED_HOT_WINDOWS * SBV_ED_HOT_PARTS);
    const u32 gid = blockIdx.x * 64 + threadIdx.x;
    u32* mine = tmp + (size_t)gid * SBV_ED_HOT_TMP_WORDS;
    for (u32 item = gid; item < total; item += gridDim.x * 64) {
        const u32 part = item % SBV_ED_HOT_PARTS, j = (item / SBV_ED_HOT_PARTS) % SBV_ED_HOT_WINDOWS, k = item / (SBV_ED_HOT_PARTS * SBV_ED_HOT_WINDOWS);
        ed_widetab_lane(ktab + (size_t)plist[2 * k] * SBV_ED_KEYTAB_ENTRIES, j, part, mine, wtab + (size_t)plist[2 * k + 1] * SBV_ED_HOT_COMB_BYTES);
    }
}

hipError_t launch_ed_keyed_expand(const uint8_t* d_recs, const u32* d_slots, size_t n, const EdKeyedRegistry& r, uint8_t* d_tuples, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed_keyed_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_recs, d_slots, n, r.nkeys, r.kenc, d_tuples);
    return hipGetLastError();
}
hipError_t launch_ed_keyed_msg_frontend(const uint8_t* d_sigs, const u32* d_slots, const EdKeyedRegistry& r, const uint8_t* d_msgs, const u64* d_moff,
                                        size_t n, uint8_t* d_tuples, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed_keyed_msg_frontend, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_sigs, d_slots, r.nkeys, r.kenc, d_msgs, d_moff, n,
                       reinterpret_cast<u32*>(d_tuples));
    return hipGetLastError();
}
hipError_t launch_ed25519_verify_keyed(const uint8_t* d_tuples, const u32* d_slots, size_t n, const EdKeyedRegistry& r, const edcomb& bcomb,
                                       u32* d_gacc, uint8_t* d_okb, uint8_t* d_acc, uint8_t* d_bitmap, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const unsigned gv = (unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK);
    hipLaunchKernelGGL(k_ed_gphase, dim3(gv), dim3(SBV_VERIFY_BLOCK), 0, stream, d_tuples, n, bcomb, d_gacc, n, d_okb, 1);
    hipLaunchKernelGGL(k_ed_keyed_qphase, dim3(gv), dim3(SBV_VERIFY_BLOCK), 0, stream, d_tuples, d_slots, n, r, d_gacc, d_okb, d_acc);
    const size_t fl = (n + SBV_ED_FINISH_T - 1) / SBV_ED_FINISH_T;
    hipLaunchKernelGGL(k_ed_finish, dim3((unsigned)((fl + 255) / 256)), dim3(256), 0, stream, d_tuples, n, d_gacc, n, d_acc, 1);
    hipLaunchKernelGGL(k_pack_bitmap, dim3((unsigned)(((n + 7) / 8 + 255) / 256)), dim3(256), 0, stream, d_acc, n, d_bitmap);
    return hipGetLastError();
}
hipError_t launch_ed_keyed_widen(const u32* d_plist, u32 count, const aniels* d_ktab, u32* d_tmp, u32 blocks, uint8_t* d_wtab, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ed_keyed_widen, dim3(blocks), dim3(64), 0, stream, d_plist, count, d_ktab, d_tmp, d_wtab);
    return hipGetLastError();
}

}  // namespace sbv
