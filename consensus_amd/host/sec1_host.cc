// sec1_host.cc — the SEC1 key decoders as host code: sec1_decode_lane of consensus_amd/csrc/sec1_keys.h, the text the device kernels
// compile, so the two cannot drift apart.  One square root mod p per compressed key (~50 us on one core): what a caller without a
// device pays, and what Backend::decode_keys loops over by default.
#include "sec1_host.h"

#include "../csrc/sec1_keys.h"

namespace sbvhost {

using namespace sbv;

namespace {
template <int CURVE>
bool decode(const uint8_t* key, size_t len, uint8_t key64[64]) {
    u32 w[16];
    const bool ok = sec1_decode_lane<CURVE>(key, len, w);
    for (int k = 0; k < 16; ++k) {
        key64[4 * k] = (uint8_t)(w[k] >> 24); key64[4 * k + 1] = (uint8_t)(w[k] >> 16); key64[4 * k + 2] = (uint8_t)(w[k] >> 8); key64[4 * k + 3] = (uint8_t)w[k];
    }
    return ok;
}
}  // namespace

bool p256_sec1_decode(const uint8_t* key, size_t len, uint8_t key64[64]) { return decode<SBV_SEC1_P256>(key, len, key64); }
bool k256_sec1_decode(const uint8_t* key, size_t len, uint8_t key64[64]) { return decode<SBV_SEC1_K256>(key, len, key64); }

}  // namespace sbvhost
