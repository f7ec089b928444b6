// sec1_host.h — SEC1 public keys on the host: the CPU forms of sbv_p256_decode_keys / sbv_secp256k1_decode_keys (include/sbv.h),
// compiled from the lane code the device kernels run (csrc/sec1_keys.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sbvhost {

// key[0 .. len) (65 bytes 04 | X | Y, or 33 bytes 02/03 | X; nothing else is read) -> key64 = X | Y.  false, and key64 zeroed, for a
// refused key: any other length or prefix (the hybrid forms 06 / 07 included), a coordinate >= p, a point off the curve, an X without
// a point.  key may be null when len is 0.
bool p256_sec1_decode(const uint8_t* key, size_t len, uint8_t key64[64]);
bool k256_sec1_decode(const uint8_t* key, size_t len, uint8_t key64[64]);

}  // namespace sbvhost
