package gpuverifier

import (
	"crypto/ecdsa"
	"crypto/ed25519"
	"crypto/sha256"
	"errors"
	"runtime"
	"sync"
)

// Scheme is the signature scheme of a Verifier / Signer pair (consensus_amd/host/verifier.h: enum class Scheme).
//
//	SchemeP256       ECDSA over SHA-256, ASN.1 DER signatures, crypto/ecdsa.VerifyASN1 semantics (the default)
//	SchemeEd25519    crypto/ed25519.Verify semantics, 64-byte R|S signatures, 32-byte keys (BASELINE.json configs[4])
//	SchemeSecp256k1  ECDSA over SHA-256 with DER signatures like P-256, on y^2 = x^3 + 7; keys are 64 raw bytes Qx|Qy.
//	                 Go's standard library has no secp256k1: without a device backend such a batch cannot be judged.
type Scheme int

const (
	SchemeP256 Scheme = iota
	SchemeEd25519
	SchemeSecp256k1
)

// Item is one signature to verify: the signer's key, the signed bytes and the signature.
//
//	Pub   the P-256 key (SchemeP256)
//	Key   the raw key bytes of the other schemes: 32-byte Ed25519 key, or 64 bytes Qx|Qy big-endian for secp256k1
//	Slot  >= 0 when the key is registered with the device (sbv_p256_register_keys, sbv_ed25519_register_keys under
//	      SchemeEd25519, sbv_secp256k1_register_keys under SchemeSecp256k1: one registry per scheme); -1 otherwise
type Item struct {
	Pub  *ecdsa.PublicKey
	Key  []byte
	Slot int32
	Msg  []byte
	Sig  []byte
}

// ErrNoCPUPath is returned by the pure-Go backend for a scheme the standard library cannot verify.
var ErrNoCPUPath = errors.New("gpuverifier: no CPU implementation of this scheme in the standard library")

// Backend verifies a batch; ok[i] reports item i.  An error means the BATCH could not be judged (device fault): the
// caller re-verifies it on the CPU and never turns the error into "invalid signature".
//
// File-by-file counterpart of consensus_amd/host/verifier.h: class Backend (verify / verify_keyed / verify_msgs_keyed /
// verify_ed25519 / verify_k256 are folded into Verify here: the route is chosen inside the backend from the items' slots).
type Backend interface {
	Verify(scheme Scheme, items []Item) (ok []bool, err error)
	// RegisterKey gives the device a P-256 key it will see again (consenters, clients) and returns its comb slot;
	// -1 when there is no registry (then items carry Slot = -1 and travel as generic tuples with the key inline).
	RegisterKey(pub *ecdsa.PublicKey) int32
	// WidenKey marks a registered slot as a consenter's: a key that signs every vote of every decision of the epoch
	// (internal/bft/view.go:531-541, 631, 834).  The device gives it a second, wide comb (sbv_p256_widen_keys: built on the
	// device in milliseconds; 20-bit windows = 436 MB of HBM and u2*Q in 13 additions instead of 32 while at most 16 slots are
	// wide, 16-bit windows beyond); a no-op for a backend without a registry.
	WidenKey(slot int32)
	// SignBatch is the batch form of api.Signer.Sign for P-256 (sbv_p256_sign_batch: RFC 6979 nonces): signature i =
	// ECDSA(keys[keyIndex[i]], digests[i]) as r|s, 64 bytes; ok[i] = false when the key or index is unusable.
	// A backend without batch signing returns ErrNoBatchSigner and the Signer signs one by one with crypto/ecdsa.
	SignBatch(keys [][32]byte, keyIndex []uint32, digests [][32]byte) (sigs [][64]byte, ok []bool, err error)
	Close()
}

// EdKeyRegistry is the optional Ed25519 key registry of a backend (sbv_ed25519_register_keys): RegisterKeyEd25519 gives the
// device a 32-byte key it will see again and returns its slot (-1 when there is no registry: the key then travels inline);
// WidenKeyEd25519 gives a consenter's slot a 16-bit comb (sbv_ed25519_widen_keys: [k](-A) in 16 additions instead of 32).
// Slots are keyed by the encoding's bytes.  An optional interface, so that backends without it need no change.
type EdKeyRegistry interface {
	RegisterKeyEd25519(key []byte) int32
	WidenKeyEd25519(slot int32)
}

// K256KeyRegistry is the optional secp256k1 key registry of a backend (sbv_secp256k1_register_keys): RegisterKeySecp256k1 gives
// the device a 64-byte key Qx|Qy it will see again and returns its slot (-1 when there is no registry: the key then travels
// inline); WidenKeySecp256k1 gives a consenter's slot a 16-bit comb (sbv_secp256k1_widen_keys: u2*Q in 16 additions instead of
// 32).  Slots are keyed by the 64 key bytes and belong to this curve's registry alone.  An optional interface, like EdKeyRegistry.
type K256KeyRegistry interface {
	RegisterKeySecp256k1(key []byte) int32
	WidenKeySecp256k1(slot int32)
}

// EdBatchSigner is the Ed25519 batch signer of a backend (sbv_ed25519_expand_keys + sbv_ed25519_sign_msgs: RFC 8032, so the
// signatures equal crypto/ed25519.Sign's byte for byte): signature i = Ed25519(seeds[keyIndex[i]], msgs[i]) as R|S, 64 bytes;
// ok[i] = false when the index is out of range.  It stands beside Backend.SignBatch as an optional interface, like the key
// registries above, so that a Backend written before it needs no change; a backend without a device signer returns
// ErrNoBatchSigner and the caller signs one by one with crypto/ed25519.  NOT constant-time on the device (include/sbv.h).
type EdBatchSigner interface {
	SignBatchEd25519(seeds [][32]byte, keyIndex []uint32, msgs [][]byte) (sigs [][64]byte, ok []bool, err error)
}

// K256BatchSigner is the secp256k1 batch signer of a backend (sbv_secp256k1_sign_batch: ECDSA with the deterministic nonce of
// RFC 6979): signature i = ECDSA-secp256k1(keys[keyIndex[i]], digests[i]) as r|s, 64 bytes big-endian, and recid[i] its recovery
// id 0..3; lowS replaces s > (n-1)/2 by n - s (the Bitcoin / Ethereum form).  ok[i] = false when the key is not in [1, n-1] or the
// index is out of range.  An optional interface beside Backend like EdBatchSigner, for the same reason; a backend without a device
// signer returns ErrNoBatchSigner.  NOT constant-time on the device (secret-indexed table lookups in HBM, include/sbv.h).
type K256BatchSigner interface {
	SignBatchSecp256k1(keys [][32]byte, keyIndex []uint32, digests [][32]byte, lowS bool) (sigs [][64]byte, recid []byte, ok []bool, err error)
}

// ECDSAMsgSigner is the raw-message ECDSA signer of a backend (sbv_p256_sign_msgs / sbv_secp256k1_sign_msgs: SHA-256, the RFC 6979
// signature and the DER encoding on the device, one call): sigs[i] = the DER signature of msgs[i] under keys[keyIndex[i]], what
// RawMessageVerifier.VerifyMsgs takes as Item.Sig; a nil keyIndex means key i % len(keys); lowS replaces s > (n-1)/2 by n - s on
// either curve (Fabric's BCCSP refuses the high form of P-256).  recid is nil for SchemeP256.  ok[i] = false, and an empty signature, when the key is not in [1, n-1] or the
// index is out of range.  An optional interface beside Backend like K256BatchSigner, for the same reason; a backend without a device
// signer returns ErrNoBatchSigner.  NOT constant-time on the device (include/sbv.h).
type ECDSAMsgSigner interface {
	SignMsgs(scheme Scheme, keys [][32]byte, keyIndex []uint32, msgs [][]byte, lowS bool) (sigs [][]byte, recid []byte, ok []bool, err error)
}

// K256BatchRecoverer is the secp256k1 public-key recovery of a backend (sbv_secp256k1_recover): key i = the signer's Qx|Qy of
// signature sigs[i] (r|s, 64 bytes big-endian) with recovery id recid[i] (0..3, as K256BatchSigner emits it) over digests[i], by the
// rules of libsecp256k1's ecdsa_recover (include/sbv.h); lowS also refuses s > (n-1)/2.  ok[i] = false, and a zero key, for a refused
// input.  Traffic shaped like Ethereum's carries r|s|v and no key: recover, then register the keys (Backend.RegisterKeys of the
// secp256k1 registry) and verify keyed.  An optional interface beside Backend like K256BatchSigner, so that existing backends need no
// change: callers type-assert for it.
type K256BatchRecoverer interface {
	RecoverBatchSecp256k1(sigs [][64]byte, recid []byte, digests [][32]byte, lowS bool) (pubs [][64]byte, ok []bool, err error)
}

// K256AddressRecoverer is K256BatchRecoverer with the signer's 20-byte address Keccak-256(Qx|Qy)[12:] in place of the key
// (sbv_secp256k1_recover_addresses): what Ethereum's ecrecover returns and what traffic shaped like Ethereum's compares.  Rules, recid
// and lowS are those of RecoverBatchSecp256k1; ok[i] = false, and a zero address, for a refused input.  The digests are Keccak-256 of
// the transaction or message (sbv_keccak256_msgs).  EIP-155 v values, EIP-191 prefixes and EIP-55 checksums are the caller's
// formatting.  An optional interface beside K256BatchRecoverer, so that existing backends need no change: callers type-assert.
type K256AddressRecoverer interface {
	RecoverAddressesSecp256k1(sigs [][64]byte, recid []byte, digests [][32]byte, lowS bool) (addrs [][20]byte, ok []bool, err error)
}

// K256Schnorr is the BIP-340 Schnorr pair of a backend over secp256k1 (sbv_secp256k1_schnorr_verify, _expand_keys and _sign): what
// traffic shaped like Bitcoin's carries since Taproot.  VerifyBatchSchnorr: ok[i] = the verdict of BIP-340 "Verify" on the x-only key
// pks[i], the 32-byte message msgs[i] and sigs[i] = R.x|s.  SignBatchSchnorr: signature i = BIP-340 "Default Signing" of msgs[i] under
// keys[keyIndex[i]] with the auxiliary randomness aux[i] (aux == nil: 32 zero bytes for every message); pks[k] is the x-only public
// key of keys[k]; ok[i] = false, and a zero signature, when the key is not in [1, n-1] or the index is out of range.  Signing on the
// device is not constant-time (include/sbv.h).  An optional interface beside Backend like K256BatchRecoverer: callers type-assert.
type K256Schnorr interface {
	VerifyBatchSchnorr(pks [][32]byte, msgs [][32]byte, sigs [][64]byte) (ok []bool, err error)
	SignBatchSchnorr(keys [][32]byte, keyIndex []uint32, msgs [][32]byte, aux [][32]byte) (sigs [][64]byte, pks [][32]byte, ok []bool, err error)
}

// K256SchnorrKeyed is BIP-340 verification against registered secp256k1 keys (sbv_secp256k1_schnorr_lift_keys +
// sbv_secp256k1_register_keys, sbv_secp256k1_schnorr_verify_keyed): for a fixed key set that signs again and again.
// RegisterSchnorrKeys: slots[i] = the slot of the x-only key pks[i] in the registry of K256KeyRegistry (one registry for ECDSA and
// Schnorr; WidenKeySecp256k1 works on these slots); onCurve[i] = false for a key that is no x of a curve point: it gets a slot too,
// against which every signature is rejected.  VerifyBatchSchnorrKeyed: ok[i] = the verdict of BIP-340 "Verify" on msgs[i] and
// sigs[i] = R.x|s under the key of slots[i]; an unknown slot is a reject.  An optional interface beside K256Schnorr, so that
// existing backends need no change: callers type-assert.
type K256SchnorrKeyed interface {
	RegisterSchnorrKeys(pks [][32]byte) (slots []uint32, onCurve []bool, err error)
	VerifyBatchSchnorrKeyed(msgs [][32]byte, sigs [][64]byte, slots []uint32) (ok []bool, err error)
}

// RawMessageVerifier is the raw-message form of Verify for signers that hold no slot (sbv_p256_verify_msgs, its sharded form and
// sbv_secp256k1_verify_msgs): Msg, Sig (ASN.1 DER) and the 64-byte key Qx|Qy of every item go to the device as they are; SHA-256, the
// strict DER parse and the tuple layout run there, so the host only lays bytes out.  ok[i] is what Verify reports for item i: a
// signature that does not parse and a key the verifier refuses are rejects.  SchemeP256 and SchemeSecp256k1 only; Slot is ignored.
// What VerifyProposal's K client requests take when the clients are not registered.  An optional interface beside Backend like the
// key registries, so that existing backends need no change: callers type-assert for it.
type RawMessageVerifier interface {
	VerifyMsgs(scheme Scheme, items []Item) (ok []bool, err error)
}

// SEC1KeyDecoder decodes public keys from their SEC1 octet strings (sbv_p256_decode_keys / sbv_secp256k1_decode_keys): keys[i] is 65
// bytes 04|X|Y or 33 bytes 02/03|X, what elliptic.Marshal / elliptic.MarshalCompressed, an X.509 SubjectPublicKeyInfo and secp256k1
// traffic carry; pubs[i] = X|Y, the 64 bytes Item.Key, the key registries and RawMessageVerifier take.  ok[i] = false, and a zero key,
// for anything elliptic.Unmarshal / UnmarshalCompressed refuse: another length or prefix (the hybrid forms 06 / 07 too), a coordinate
// >= p, a point off the curve, an X without a point.  SchemeP256 and SchemeSecp256k1 only.  The compressed form costs a square root
// per key, which is why it runs on the device.  An optional interface beside Backend like K256SchnorrKeyed: callers type-assert.
type SEC1KeyDecoder interface {
	DecodeKeysSEC1(scheme Scheme, keys [][]byte) (pubs [][64]byte, ok []bool, err error)
}

// ErrNoBatchSigner: the backend has no batch signing entry (the pure-Go backend).
var ErrNoBatchSigner = errors.New("gpuverifier: backend has no batch signer")

// cpuBackend is the standard library: the reference semantics themselves (ecdsa.VerifyASN1 over SHA-256(Msg),
// ed25519.Verify).
type cpuBackend struct{}

func (cpuBackend) Verify(scheme Scheme, items []Item) ([]bool, error) {
	if scheme != SchemeP256 && scheme != SchemeEd25519 {
		return nil, ErrNoCPUPath
	}
	ok := make([]bool, len(items))
	one := func(i int) {
		it := &items[i]
		if scheme == SchemeP256 {
			h := sha256.Sum256(it.Msg)
			ok[i] = it.Pub != nil && ecdsa.VerifyASN1(it.Pub, h[:], it.Sig)
		} else {
			ok[i] = len(it.Key) == ed25519.PublicKeySize && ed25519.Verify(ed25519.PublicKey(it.Key), it.Msg, it.Sig)
		}
	}
	workers := runtime.GOMAXPROCS(0)
	if workers > len(items) {
		workers = len(items)
	}
	if workers <= 1 {
		for i := range items {
			one(i)
		}
		return ok, nil
	}
	var wg sync.WaitGroup // a batch on the CPU route (a proposal below GPUMin, a device fault) uses every core
	for w := 0; w < workers; w++ {
		wg.Add(1)
		go func(w int) {
			defer wg.Done()
			for i := w; i < len(items); i += workers {
				one(i)
			}
		}(w)
	}
	wg.Wait()
	return ok, nil
}
func (cpuBackend) RegisterKey(*ecdsa.PublicKey) int32 { return -1 }
func (cpuBackend) WidenKey(int32)                      {}
func (cpuBackend) SignBatch([][32]byte, []uint32, [][32]byte) ([][64]byte, []bool, error) {
	return nil, nil, ErrNoBatchSigner
}
func (cpuBackend) SignBatchEd25519([][32]byte, []uint32, [][]byte) ([][64]byte, []bool, error) {
	return nil, nil, ErrNoBatchSigner
}
func (cpuBackend) SignBatchSecp256k1([][32]byte, []uint32, [][32]byte, bool) ([][64]byte, []byte, []bool, error) {
	return nil, nil, nil, ErrNoBatchSigner
}
func (cpuBackend) Close() {}
