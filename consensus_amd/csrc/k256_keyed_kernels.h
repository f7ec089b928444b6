// k256_keyed_kernels.h — launch interface between the C-ABI layer (sbv_api.hip) and the kernels of k256_keyed_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "k256_keyed.h"
#include "p256_kernels.h"

namespace sbv {

// The wave rule of the kernels that walk registered slots (k_k256_keyed_verify; k256_schnorr_keyed_kernels.hip): the wavefront takes the
// 16-bit combs when a lane of it is live and every live lane's slot owns one (lane_wide = k256_keyed_slot_wide); dead lanes never
// decide.  ONE function for every such kernel.
__device__ inline bool k256_keyed_wave_wide(bool live, bool lane_wide) { return __ballot(live) != 0 && __ballot(live && !lane_wide) == 0; }

// stage A + stage B of n keyed records (96 bytes, 16-byte aligned) on `stream`; s: the limb-major scratch planes, d_gcomb: the
// `gcomb_bits`-wide comb of G of the grouped step.  after_prep (optional) is recorded between the stages.
hipError_t launch_k256_verify_keyed(const uint8_t* d_recs, const u32* d_slots, size_t n, const Scratch& s, const K256KeyedRegistry& reg,
                                    const kapt* d_gcomb, int gcomb_bits, uint8_t* d_bitmap, hipStream_t stream, hipEvent_t after_prep = nullptr);
// the 8-bit combs and valid bytes of slots [slot0, slot0 + count) from d_kkeys (64 bytes per slot); d_work: k256_reg_build_words(count) words
size_t k256_reg_build_words(u32 count);
hipError_t launch_k256_reg_build(const uint8_t* d_kkeys, u32 slot0, u32 count, u32* d_work, kapt* d_ktab, uint8_t* d_kvalid, hipStream_t stream);
// comb w of d_wtab = the 16-bit comb of `slot`, from its 8-bit comb; d_tmp: k256_widetab_tmp_words() words
size_t k256_widetab_tmp_words();
hipError_t launch_k256_widetab(const kapt* d_ktab, u32 slot, u32* d_tmp, kapt* d_wtab, u32 w, hipStream_t stream);
bool host_build_k256_wide_comb(const uint8_t key[64], kapt* out);     // SBV_K256_WIDE_ENTRIES entries

}  // namespace sbv
