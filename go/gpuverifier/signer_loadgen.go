//go:build sbv_loadgen

package gpuverifier

import (
	"crypto/ed25519"
	"crypto/sha256"
	"encoding/asn1"
	"math/big"
)

// LoadgenSigner is a Signer whose key may go to the device's batch signer.  It is its own type, in a file that only a
// build with -tags sbv_loadgen contains, because sbv_p256_sign_batch is NOT constant-time (secret-indexed table lookups in
// HBM, include/sbv.h): a consensus node's long-term key must not be able to reach it by accident, so the production Signer
// has no such method.  For load generators and replay tools over throw-away keys.
//
// Scheme selects the signer: SchemeP256 (the zero value) signs with Signer.Key; SchemeEd25519 signs with EdSeed, the 32-byte
// RFC 8032 private key, through sbv_ed25519_expand_keys / sbv_ed25519_sign_msgs — just as little constant-time.
//
// SchemeSecp256k1 signs SHA-256 of each message with K256Key, the 32-byte big-endian private scalar, through
// sbv_secp256k1_sign_batch (K256LowS selects the low-S form) and DER-encodes r, s like the P-256 path.  Go's standard library has
// no secp256k1, so this scheme has no host signer to fall back on: a message the device did not sign (no K256BatchSigner, a fault,
// a key outside [1, n-1]) comes back nil.
type LoadgenSigner struct {
	Signer
	Scheme   Scheme
	EdSeed   []byte
	K256Key  []byte
	K256LowS bool
}

// signBatchSecp256k1: every message under K256Key through the backend's K256BatchSigner, DER-encoded; nil where nothing was signed.
func (s *LoadgenSigner) signBatchSecp256k1(be Backend, msgs [][]byte) [][]byte {
	out := make([][]byte, len(msgs))
	if len(s.K256Key) != 32 {
		panic("gpuverifier: LoadgenSigner under SchemeSecp256k1 needs a 32-byte K256Key")
	}
	kb, has := be.(K256BatchSigner)
	if !has || len(msgs) == 0 {
		return out
	}
	var key [32]byte
	copy(key[:], s.K256Key)
	digests := make([][32]byte, len(msgs))
	for i, m := range msgs {
		digests[i] = sha256.Sum256(m)
	}
	sigs, _, ok, err := kb.SignBatchSecp256k1([][32]byte{key}, make([]uint32, len(msgs)), digests, s.K256LowS)
	for i := range key {
		key[i] = 0
	}
	if err != nil || len(sigs) != len(msgs) {
		return out
	}
	for i := range msgs {
		if !ok[i] {
			continue
		}
		der, e := asn1.Marshal(struct{ R, S *big.Int }{new(big.Int).SetBytes(sigs[i][:32]), new(big.Int).SetBytes(sigs[i][32:])})
		if e == nil {
			out[i] = der
		}
	}
	return out
}

// signBatchEd25519: every message under EdSeed through the backend's EdBatchSigner; what the device did not sign (no such
// backend, a fault) is signed by crypto/ed25519 — the same bytes, RFC 8032 being deterministic.
func (s *LoadgenSigner) signBatchEd25519(be Backend, msgs [][]byte) [][]byte {
	out := make([][]byte, len(msgs))
	if len(s.EdSeed) != ed25519.SeedSize {
		panic("gpuverifier: LoadgenSigner under SchemeEd25519 needs a 32-byte EdSeed")
	}
	if eb, has := be.(EdBatchSigner); has && len(msgs) > 0 {
		var seed [32]byte
		copy(seed[:], s.EdSeed)
		sigs, ok, err := eb.SignBatchEd25519([][32]byte{seed}, make([]uint32, len(msgs)), msgs)
		for i := range seed {
			seed[i] = 0
		}
		if err == nil && len(sigs) == len(msgs) {
			for i := range msgs {
				if ok[i] {
					out[i] = append([]byte(nil), sigs[i][:]...)
				}
			}
		}
	}
	var key ed25519.PrivateKey
	for i, m := range msgs {
		if out[i] == nil {
			if key == nil {
				key = ed25519.NewKeyFromSeed(s.EdSeed)
			}
			out[i] = ed25519.Sign(key, m)
		}
	}
	return out
}

// SignBatch is the batch form of Sign (a consensus node signs once per sequence and
// has no use for it): every message is signed with this key through the backend's batch signer
// (sbv_p256_sign_batch: deterministic RFC 6979 nonces, DER-encoded here); a backend without one, a device fault or an
// unusable key sends the affected messages through Sign.  Counterpart: consensus_amd/host (Signer over p256_host.cc) and
// the device entry it is tested against (tests/test_gpu_sign.py).
func (s *LoadgenSigner) SignBatch(be Backend, msgs [][]byte) [][]byte {
	if s.Scheme == SchemeEd25519 {
		return s.signBatchEd25519(be, msgs)
	}
	if s.Scheme == SchemeSecp256k1 {
		return s.signBatchSecp256k1(be, msgs)
	}
	out := make([][]byte, len(msgs))
	if be != nil && len(msgs) > 0 && s.Key != nil && s.Key.D != nil && s.Key.D.Sign() > 0 && s.Key.D.BitLen() <= 256 {
		var key [32]byte
		s.Key.D.FillBytes(key[:])
		digests := make([][32]byte, len(msgs))
		for i, m := range msgs {
			digests[i] = sha256.Sum256(m)
		}
		sigs, ok, err := be.SignBatch([][32]byte{key}, make([]uint32, len(msgs)), digests)
		for i := range key {
			key[i] = 0
		}
		if err == nil && len(sigs) == len(msgs) {
			for i := range msgs {
				if !ok[i] {
					continue
				}
				der, e := asn1.Marshal(struct{ R, S *big.Int }{new(big.Int).SetBytes(sigs[i][:32]), new(big.Int).SetBytes(sigs[i][32:])})
				if e == nil {
					out[i] = der
				}
			}
		}
	}
	for i, m := range msgs {
		if out[i] == nil {
			out[i] = s.Sign(m)
		}
	}
	return out
}
