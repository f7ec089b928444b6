// k256_host.h — host-side secp256k1 key derivation and RFC 6979 signing for Scheme::SECP256K1 (verifier.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sbvhost {

bool k256_pubkey_from_private(const uint8_t d_be[32], uint8_t q[64]);      // false: d = 0 or d >= n
bool k256_sign_with_nonce(const uint8_t d_be[32], const uint8_t k_be[32], const uint8_t digest[32], uint8_t rs[64]);
bool k256_sign_rfc6979(const uint8_t d_be[32], const uint8_t digest[32], uint8_t rs[64]);
// the signer's public key from r | s, the recovery id 0..3 and the digest, by the rules of sbv_secp256k1_recover (include/sbv.h) with
// flags = 0: the CPU form of the device entry, on the same lane functions (csrc/k256_recover.h) with u1 G from the signer's 8-bit comb.
// false, and q zeroed, for a refused input.
bool k256_recover(const uint8_t rs[64], uint8_t recid, const uint8_t digest[32], uint8_t q[64]);
// Keccak-256 (Ethereum's keccak256, not SHA3-256) and the hashes around a recovery, by the rules of sbv_keccak256_msgs,
// sbv_secp256k1_addresses and sbv_secp256k1_recover_addresses (include/sbv.h): the CPU forms of the device entries, on the same lane
// code (csrc/keccak256_dev.h).  keccak256 reads msg[0 .. len) only (msg may be null when len is 0).  k256_address hashes any 64 bytes.
// k256_recover_address is k256_recover followed by k256_address: false, and addr zeroed, for a refused input.
void keccak256(const uint8_t* msg, size_t len, uint8_t digest[32]);
void k256_address(const uint8_t q[64], uint8_t addr[20]);
bool k256_recover_address(const uint8_t rs[64], uint8_t recid, const uint8_t digest[32], uint8_t addr[20]);
// BIP-340 Schnorr by the rules of the sbv_secp256k1_schnorr_ entries (include/sbv.h): the CPU forms of the device entries, on the same
// lane functions (csrc/k256_schnorr.h) with G from the signer's 8-bit comb.  rec = d | P.x, as secret as the key; aux may be null
// (32 zero bytes).  expand and sign return false, with the output zeroed, for a refused key or record.  NOT constant-time.
bool k256_schnorr_expand(const uint8_t d_be[32], uint8_t rec[64]);
bool k256_schnorr_sign(const uint8_t rec[64], const uint8_t msg[32], const uint8_t* aux, uint8_t sig[64]);
bool k256_schnorr_verify(const uint8_t pk[32], const uint8_t msg[32], const uint8_t sig[64]);
// BIP-340 against registered keys (include/sbv.h: sbv_secp256k1_schnorr_lift_keys, _verify_keyed).  lift: key = x | y of lift_x(pk), or
// x | 32 zero bytes and false for a key off the curve.  verify_keyed: the verdict of the device entry for a slot that holds `key`
// (Qx | Qy of either parity): false when the key is no curve point (an invalid slot), else k256_schnorr_verify under Qx.
bool k256_schnorr_lift(const uint8_t pk[32], uint8_t key[64]);
bool k256_schnorr_verify_keyed(const uint8_t key[64], const uint8_t msg[32], const uint8_t sig[64]);

}  // namespace sbvhost
