// k256_keyed_kernels.hip — registered secp256k1 keys (k256_keyed.h): the keyed step and the comb builders of the registry.
//
//   the step     k_k256_keyed_prep    stage A on 96-byte records (T records per inversion, T by batch size)
//                k_k256_keyed_verify  one lane per signature: u1 * G from the comb of G, u2 * Q from the slot's comb — the 16-bit
//                                     comb when a ballot finds that every live lane of the wavefront owns one, else the 8-bit comb
//                                     every slot keeps — and the verdict bits packed by a ballot.  No grouping state, no side streams.
//   register     k_k256_reg_chain | k_k256_reg_rows | k_k256_reg_fill: the grouped step's table lanes over the fresh slots
//   widen        k_k256_widetab: the 16-bit comb of one slot from its 8-bit comb
//
// The kernels of the grouped step (k256_group_kernels.hip) and of the one-lane path (k256_kernels.hip) are not touched.
#include <hip/hip_runtime.h>

#include <thread>
#include <vector>

#include "k256_keyed.h"
#include "k256_keyed_kernels.h"

namespace sbv {

__global__ __launch_bounds__(64) void k_k256_keyed_prep(const uint8_t* __restrict__ recs, size_t n, Scratch s, int T) {
    const size_t first = (size_t)blockIdx.x * 64 * (size_t)T + threadIdx.x;
    k256_keyed_prep_lane(recs, n, s, first, (size_t)64, T);
}

__global__ __launch_bounds__(SBV_VERIFY_BLOCK, 2) void k_k256_keyed_verify(Scratch s, const u32* __restrict__ slots, size_t n, K256KeyedRegistry reg, kgcomb gc,
                                                                         uint8_t* __restrict__ bitmap) {
    const size_t i = (size_t)blockIdx.x * SBV_VERIFY_BLOCK + threadIdx.x;
    const bool in = i < n;
    const size_t ii = in ? i : n - 1;                   // the lanes behind the batch's end walk the last record's tables and report nothing
    const u32 slot = slots[ii];
    const bool live = in && k256_keyed_live(s, ii, slot, reg);
    // the ballot: dead lanes never decide their wavefront
    const bool lane_wide = k256_keyed_slot_wide(slot, reg);
    const bool wide = k256_keyed_wave_wide(live, lane_wide);
    const bool accept = k256_keyed_verify_lane(s, ii, slot, live, reg, gc, wide);
    const unsigned long long m = __ballot(accept);
    const int lane = threadIdx.x & 63;
    const size_t wave_first = i - (size_t)lane;
    if (lane < 8) {
        const size_t byte = (wave_first >> 3) + (size_t)lane;
        if (byte < ((n + 7) >> 3)) bitmap[byte] = (uint8_t)(m >> (8 * lane));
    }
}

hipError_t launch_k256_verify_keyed(const uint8_t* d_recs, const u32* d_slots, size_t n, const Scratch& s, const K256KeyedRegistry& reg,
                                    const kapt* d_gcomb, int gcomb_bits, uint8_t* d_bitmap, hipStream_t stream, hipEvent_t after_prep) {
    if (n == 0) return hipSuccess;
    const int T = k256_keyed_prep_T(n);
    const size_t per_block = (size_t)64 * T;
    hipLaunchKernelGGL(k_k256_keyed_prep, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(64), 0, stream, d_recs, n, s, T);
    if (after_prep) {
        const hipError_t e = hipEventRecord(after_prep, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_k256_keyed_verify, dim3((unsigned)((n + SBV_VERIFY_BLOCK - 1) / SBV_VERIFY_BLOCK)), dim3(SBV_VERIFY_BLOCK), 0, stream, s, d_slots, n,
                       reg, kgcomb_make(d_gcomb, gcomb_bits), d_bitmap);
    return hipGetLastError();
}

// ---- the registry's 8-bit combs ----------------------------------------------------------------------------------------------
// lanes = count x 4 (one quad per key, the DPP exchange of k256_quad_dev)
__global__ __launch_bounds__(64) void k_k256_reg_chain(const uint8_t* __restrict__ kkeys, u32 slot0, u32 count, u32* __restrict__ jstate, u32* __restrict__ bases,
                                                       uint8_t* __restrict__ kvalid) {
    const u32 lane = blockIdx.x * 64 + threadIdx.x;
    const u32 k = lane >> 2;
    if (k >= count) return;
    k256_quad_dev q;
    q.r = (int)(lane & 3u);
    k256_reg_chain_run(q, kkeys, slot0, k, jstate, bases, kvalid);
}
__global__ __launch_bounds__(64, 2) void k_k256_reg_rows(u32 slot0, u32 count, const u32* __restrict__ bases, u32* __restrict__ tmp, kapt* __restrict__ ktab) {
    k256_reg_rows_lane(blockIdx.x * 64 + threadIdx.x, count, slot0, bases, tmp, ktab);
}
__global__ __launch_bounds__(64) void k_k256_reg_fill(u32 slot0, u32 count, u32* __restrict__ tmp, kapt* __restrict__ ktab) {
    k256_reg_fill_lane(blockIdx.x * 64 + threadIdx.x, count, slot0, tmp, ktab);
}

size_t k256_reg_build_words(u32 count) {
    return (size_t)count * (SBV_K256_STATE_WORDS + (size_t)SBV_GTAB_WINDOWS * (SBV_K256_BASES_STRIDE + SBV_K256_WINDOW_TMP));
}
hipError_t launch_k256_reg_build(const uint8_t* d_kkeys, u32 slot0, u32 count, u32* d_work, kapt* d_ktab, uint8_t* d_kvalid, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    u32* jstate = d_work;
    u32* bases = jstate + (size_t)count * SBV_K256_STATE_WORDS;
    u32* tmp = bases + (size_t)count * SBV_GTAB_WINDOWS * SBV_K256_BASES_STRIDE;
    // window 32 holds one entry; the others of it are zero in every slot, as in the host builder's table
    hipError_t e = hipMemsetAsync(d_ktab + (size_t)slot0 * SBV_K256_KEYTAB_ENTRIES, 0, (size_t)count * SBV_K256_KEYTAB_ENTRIES * sizeof(kapt), stream);
    if (e != hipSuccess) return e;
    const size_t wl = (size_t)count * SBV_GTAB_WINDOWS * 2, fl = (size_t)count * SBV_GTAB_WINDOWS * 7;
    hipLaunchKernelGGL(k_k256_reg_chain, dim3((count * 4 + 63) / 64), dim3(64), 0, stream, d_kkeys, slot0, count, jstate, bases, d_kvalid);
    hipLaunchKernelGGL(k_k256_reg_rows, dim3((unsigned)((wl + 63) / 64)), dim3(64), 0, stream, slot0, count, bases, tmp, d_ktab);
    hipLaunchKernelGGL(k_k256_reg_fill, dim3((unsigned)((fl + 63) / 64)), dim3(64), 0, stream, slot0, count, tmp, d_ktab);
    return hipGetLastError();
}

// ---- the 16-bit combs --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_k256_widetab(const kapt* __restrict__ qtab, u32* __restrict__ tmp, kapt* __restrict__ wide) {
    const u32 lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= SBV_K256_WIDE_LANES) return;
    k256_widetab_lane(qtab, lane, tmp + (size_t)lane * SBV_K256_WIDE_TMP_WORDS, wide);
}
size_t k256_widetab_tmp_words() { return (size_t)SBV_K256_WIDE_LANES * SBV_K256_WIDE_TMP_WORDS; }
hipError_t launch_k256_widetab(const kapt* d_ktab, u32 slot, u32* d_tmp, kapt* d_wtab, u32 w, hipStream_t stream) {
    kapt* wide = d_wtab + (size_t)w * SBV_K256_WIDE_ENTRIES;
    const hipError_t e = hipMemsetAsync(wide + (size_t)(SBV_K256_WIDE_WINDOWS - 1) * SBV_K256_WIDE_PER_WINDOW, 0, (size_t)SBV_K256_WIDE_PER_WINDOW * sizeof(kapt), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_k256_widetab, dim3((SBV_K256_WIDE_LANES + 63) / 64), dim3(64), 0, stream, d_ktab + (size_t)slot * SBV_K256_KEYTAB_ENTRIES, d_tmp, wide);
    return hipGetLastError();
}

// the host reference of a slot's 16-bit comb (k256_keyed_host_wide_window), one thread per window; false = not a point
bool host_build_k256_wide_comb(const uint8_t key[64], kapt* out) {
    u32 w[16];
    memcpy(w, key, sizeof(w));
    kfe x, y;
    if (!k256_key_load_words(w, x, y)) return false;
    memset((void*)out, 0, SBV_K256_WIDE_COMB_BYTES);
    std::vector<std::thread> th;
    for (int j = 0; j < SBV_K256_WIDE_WINDOWS; ++j)
        th.emplace_back([=] { k256_keyed_host_wide_window(x, y, SBV_K256_WIDE_BITS, j, out + (size_t)j * SBV_K256_WIDE_PER_WINDOW); });
    for (auto& t : th) t.join();
    return true;
}

}  // namespace sbv
