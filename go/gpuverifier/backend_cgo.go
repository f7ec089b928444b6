//go:build sbvgpu

package gpuverifier

/*
#cgo LDFLAGS: -lsbv
#include <stdlib.h>
#include "sbv.h"
*/
import "C"

import (
	"crypto/ecdsa"
	"crypto/sha256"
	"errors"
	"runtime"
	"sync"
	"unsafe"
)

const (
	tupleBytes   = 160     // r | s | hash | Qx | Qy   (include/sbv.h)
	rshBytes     = 96      // r | s | hash             (registered-key form)
	frontEndMax  = 1 << 21 // sbv_p256_verify_msgs_keyed / sbv_ed25519_verify_msgs take one chunk of at most 2^21
	frontEndFrom = 64      // below this many signatures the host hashes and parses itself (one upload instead of five)
	shardedFrom  = 32768   // above this many registered-key signatures: every GPU of the node, uploads in pieces beside the kernels
)

// gpuBackend talks to libsbv.so.  All device work is funnelled through ONE goroutine locked to its OS thread
// (HIP binds devices per thread; a blocked cgo call pins an OS thread anyway), fed by a channel.
//
// Counterpart of consensus_amd/host/verifier.cc: class SbvBackend — the same four routes:
//
//	every item has a slot, n > shardedFrom     sbv_p256_verify_msgs_keyed_sharded  the same inputs over every GPU of the node (decision replay:
//	                                           50 000 decisions x 11 commit signatures, internal/bft/controller.go:587-633), in pieces
//	every item has a slot, n >= frontEndFrom   sbv_p256_verify_msgs_keyed   raw messages + DER + slots (SHA-256 and DER on the device)
//	every item has a slot                      sbv_p256_verify_batch_keyed  96-byte r|s|hash records + slots
//	otherwise                                  sbv_p256_verify_batch_sharded generic tuples, all GPUs of the node
//	SchemeEd25519, every item has a slot       sbv_ed25519_verify_msgs_keyed  signatures + raw messages + slots (SHA-512 on the device)
//	SchemeSecp256k1, every item has a slot     sbv_secp256k1_verify_msgs_keyed (n >= frontEndFrom) / sbv_secp256k1_verify_batch_keyed
//	SchemeEd25519 / SchemeSecp256k1            sbv_ed25519_verify_msgs / sbv_secp256k1_verify_batch
//
// and, beside Verify, VerifyMsgs (the optional RawMessageVerifier) for signers without a slot: sbv_p256_verify_msgs_sharded /
// sbv_secp256k1_verify_msgs — raw messages + DER + keys, SHA-256, the DER parse and the tuple layout on the device.
type gpuBackend struct {
	jobs     chan *gpuJob
	mu       sync.Mutex
	regs     map[[64]byte]int32
	edRegs   map[[32]byte]int32 // the Ed25519 registry's slots (sbv_ed25519_register_keys), by encoding
	k256Regs map[[64]byte]int32 // the secp256k1 registry's slots (sbv_secp256k1_register_keys), by key bytes: not the slots of regs
}

type gpuJob struct {
	run  func()
	done chan struct{}
}

// NewDeviceBackend initialises every visible MI355X (sbv_init_all).
func NewDeviceBackend() (Backend, error) {
	b := &gpuBackend{jobs: make(chan *gpuJob, 64), regs: map[[64]byte]int32{}, edRegs: map[[32]byte]int32{}, k256Regs: map[[64]byte]int32{}}
	ready := make(chan error, 1)
	go b.loop(ready)
	if err := <-ready; err != nil {
		return nil, err
	}
	return b, nil
}

func lastError() error { return errors.New("libsbv: " + C.GoString(C.sbv_last_error())) }

func (b *gpuBackend) loop(ready chan<- error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if n := C.sbv_init_all(); n <= 0 {
		ready <- lastError()
		return
	}
	ready <- nil
	for j := range b.jobs {
		j.run()
		close(j.done)
	}
	C.sbv_shutdown()
}

// on runs f on the device goroutine and waits for it.
func (b *gpuBackend) on(f func()) {
	j := &gpuJob{run: f, done: make(chan struct{})}
	b.jobs <- j
	<-j.done
}

func keyBytes(pub *ecdsa.PublicKey) [64]byte {
	var k [64]byte
	pub.X.FillBytes(k[0:32]) // keys are validated at registration (non-negative, <= 256 bits)
	pub.Y.FillBytes(k[32:64])
	return k
}

func bitmapToBools(bitmap []byte, n int) []bool {
	ok := make([]bool, n)
	for i := range ok {
		ok[i] = bitmap[i>>3]>>(uint(i)&7)&1 == 1
	}
	return ok
}

func u8(p []byte) *C.uint8_t { return (*C.uint8_t)(unsafe.Pointer(&p[0])) }

// fillRSH writes r | s | hash of one item at t[0:96]: strict DER (cryptobyte rules; on failure r = s = 0, which every
// verify rejects) and SHA-256 of the message.
func fillRSH(t []byte, it *Item) {
	if len(it.Sig) > 0 {
		C.sbv_p256_parse_der(u8(it.Sig), C.size_t(len(it.Sig)), u8(t))
	}
	h := sha256.Sum256(it.Msg)
	copy(t[64:96], h[:])
}

func allSlotted(items []Item) bool {
	for i := range items {
		if items[i].Slot < 0 {
			return false
		}
	}
	return true
}

// packMsgs lays variable-length byte strings back to back with an offset table (n + 1 entries), as the device front
// ends take them.
func packMsgs(get func(i int) []byte, n int) ([]byte, []uint64) {
	off := make([]uint64, n+1)
	total := 0
	for i := 0; i < n; i++ {
		off[i] = uint64(total)
		total += len(get(i))
	}
	off[n] = uint64(total)
	buf := make([]byte, total+1) // never empty: &buf[0] must exist
	for i := 0; i < n; i++ {
		copy(buf[off[i]:], get(i))
	}
	return buf, off
}

// verifyP256 runs on the device goroutine.  Flat []byte / []uint32 / []uint64 buffers only cross the boundary (cgo
// pointer rules); the C side has copied them to the device when the call returns.
func (b *gpuBackend) verifyP256(items []Item) ([]bool, error) {
	n := len(items)
	bitmap := make([]byte, (n+7)/8)
	if allSlotted(items) {
		slots := make([]uint32, n)
		for i := range items {
			slots[i] = uint32(items[i].Slot)
		}
		if n > shardedFrom {
			// the whole batch in one call: the library splits it by device and by piece (every device holds a replica of the key
			// registry and of the consenters' wide combs; no 2^21 limit on this entry)
			msgs, moff := packMsgs(func(i int) []byte { return items[i].Msg }, n)
			sigs, soff := packMsgs(func(i int) []byte { return items[i].Sig }, n)
			rc := C.sbv_p256_verify_msgs_keyed_sharded(u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])), u8(sigs),
				(*C.uint64_t)(unsafe.Pointer(&soff[0])), (*C.uint32_t)(unsafe.Pointer(&slots[0])), C.size_t(n), 0, 0, u8(bitmap), nil, nil)
			if rc != 0 {
				return nil, lastError()
			}
			return bitmapToBools(bitmap, n), nil
		}
		if n >= frontEndFrom {
			for lo := 0; lo < n; lo += frontEndMax {
				hi := lo + frontEndMax
				if hi > n {
					hi = n
				}
				m := hi - lo
				msgs, moff := packMsgs(func(i int) []byte { return items[lo+i].Msg }, m)
				sigs, soff := packMsgs(func(i int) []byte { return items[lo+i].Sig }, m)
				rc := C.sbv_p256_verify_msgs_keyed(u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])), u8(sigs),
					(*C.uint64_t)(unsafe.Pointer(&soff[0])), (*C.uint32_t)(unsafe.Pointer(&slots[lo])), C.size_t(m),
					u8(bitmap[lo/8:])) // lo is a multiple of 2^21: whole bitmap bytes
				if rc != 0 {
					return nil, lastError()
				}
			}
			return bitmapToBools(bitmap, n), nil
		}
		rsh := make([]byte, n*rshBytes)
		for i := range items {
			fillRSH(rsh[i*rshBytes:(i+1)*rshBytes], &items[i])
		}
		if rc := C.sbv_p256_verify_batch_keyed(u8(rsh), (*C.uint32_t)(unsafe.Pointer(&slots[0])), C.size_t(n), u8(bitmap)); rc != 0 {
			return nil, lastError()
		}
		return bitmapToBools(bitmap, n), nil
	}
	buf := make([]byte, n*tupleBytes)
	for i := range items {
		t := buf[i*tupleBytes : (i+1)*tupleBytes]
		fillRSH(t, &items[i])
		// Only the VALIDATED raw key (RegisterKey / p256Raw refuse nil or > 256-bit coordinates and leave Key empty) ever
		// reaches the tuple: big.Int.FillBytes panics on an oversized coordinate, and this runs on the device goroutine.
		// Without one the key field stays zero: (0, 0) is not on the curve, so the kernel rejects the signature, which is
		// what crypto/ecdsa does with such a key.
		if len(items[i].Key) == 64 {
			copy(t[96:160], items[i].Key)
		}
	}
	// all GPUs of the node; a batch that is not worth splitting goes whole to one device, round-robin
	rc := C.sbv_p256_verify_batch_sharded(u8(buf), C.size_t(n), 0, 0, u8(bitmap), nil, nil)
	if rc != 0 {
		return nil, lastError()
	}
	return bitmapToBools(bitmap, n), nil
}

// verifyEd25519Keyed: every item's key is registered (sbv_ed25519_verify_msgs_keyed): signatures n x 64, messages packed and
// slots; k = SHA-512(R | A | M) mod L runs on the device with A from the registry.  A signature of the wrong length is this
// layer's reject: it travels as S = 2^256 - 1, which the device rejects.
func (b *gpuBackend) verifyEd25519Keyed(items []Item) ([]bool, error) {
	n := len(items)
	ok := make([]bool, n)
	for lo := 0; lo < n; lo += frontEndMax {
		hi := lo + frontEndMax
		if hi > n {
			hi = n
		}
		m := hi - lo
		sigs := make([]byte, 64*m)
		slots := make([]uint32, m)
		for k := 0; k < m; k++ {
			it := &items[lo+k]
			if len(it.Sig) == 64 {
				copy(sigs[64*k:], it.Sig)
			} else {
				for j := 32; j < 64; j++ {
					sigs[64*k+j] = 0xFF
				}
			}
			slots[k] = uint32(it.Slot)
		}
		msgs, moff := packMsgs(func(k int) []byte { return items[lo+k].Msg }, m)
		bitmap := make([]byte, (m+7)/8)
		rc := C.sbv_ed25519_verify_msgs_keyed(u8(sigs), u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])),
			(*C.uint32_t)(unsafe.Pointer(&slots[0])), C.size_t(m), u8(bitmap))
		if rc != 0 {
			return nil, lastError()
		}
		for k := 0; k < m; k++ {
			ok[lo+k] = len(items[lo+k].Sig) == 64 && bitmap[k>>3]>>(uint(k)&7)&1 == 1
		}
	}
	return ok, nil
}

// verifyEd25519: signatures n x 64, keys n x 32, messages packed; SHA-512 and the reduction mod L run on the device.
// A signature or key of the wrong length is this layer's reject (crypto/ed25519.Verify returns false / panics on them).
// When every item's key has a registry slot the keyed entry takes the batch (verifyEd25519Keyed).
func (b *gpuBackend) verifyEd25519(items []Item) ([]bool, error) {
	if allSlotted(items) {
		return b.verifyEd25519Keyed(items)
	}
	n := len(items)
	ok := make([]bool, n)
	idx := make([]int, 0, n)
	for i := range items {
		if len(items[i].Sig) == 64 && len(items[i].Key) == 32 {
			idx = append(idx, i)
		}
	}
	for lo := 0; lo < len(idx); lo += frontEndMax {
		hi := lo + frontEndMax
		if hi > len(idx) {
			hi = len(idx)
		}
		m := hi - lo
		sigs := make([]byte, 64*m)
		pks := make([]byte, 32*m)
		for k := 0; k < m; k++ {
			copy(sigs[64*k:], items[idx[lo+k]].Sig)
			copy(pks[32*k:], items[idx[lo+k]].Key)
		}
		msgs, moff := packMsgs(func(k int) []byte { return items[idx[lo+k]].Msg }, m)
		bitmap := make([]byte, (m+7)/8)
		rc := C.sbv_ed25519_verify_msgs(u8(sigs), u8(pks), u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])), C.size_t(m), u8(bitmap))
		if rc != 0 {
			return nil, lastError()
		}
		for k := 0; k < m; k++ {
			ok[idx[lo+k]] = bitmap[k>>3]>>(uint(k)&7)&1 == 1
		}
	}
	return ok, nil
}

// verifySecp256k1Keyed: every item's key has a slot of this curve's registry.  From frontEndFrom signatures on the device front
// end takes raw messages + DER signatures + slots (sbv_secp256k1_verify_msgs_keyed, chunks of at most 2^21); below, 96-byte
// r|s|hash records built here (sbv_secp256k1_verify_batch_keyed).
func (b *gpuBackend) verifySecp256k1Keyed(items []Item) ([]bool, error) {
	n := len(items)
	accept := make([]byte, (n+7)/8)
	slots := make([]uint32, n)
	for i := range items {
		slots[i] = uint32(items[i].Slot)
	}
	if n >= frontEndFrom {
		for lo := 0; lo < n; lo += frontEndMax {
			hi := lo + frontEndMax
			if hi > n {
				hi = n
			}
			m := hi - lo
			msgs, moff := packMsgs(func(i int) []byte { return items[lo+i].Msg }, m)
			sigs, soff := packMsgs(func(i int) []byte { return items[lo+i].Sig }, m)
			rc := C.sbv_secp256k1_verify_msgs_keyed(u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])), u8(sigs),
				(*C.uint64_t)(unsafe.Pointer(&soff[0])), (*C.uint32_t)(unsafe.Pointer(&slots[lo])), C.size_t(m),
				u8(accept[lo/8:])) // lo is a multiple of 2^21: whole bitmap bytes
			if rc != 0 {
				return nil, lastError()
			}
		}
		return bitmapToBools(accept, n), nil
	}
	rsh := make([]byte, n*rshBytes)
	for i := range items {
		fillRSH(rsh[i*rshBytes:(i+1)*rshBytes], &items[i])
	}
	if rc := C.sbv_secp256k1_verify_batch_keyed(u8(rsh), (*C.uint32_t)(unsafe.Pointer(&slots[0])), C.size_t(n), u8(accept)); rc != 0 {
		return nil, lastError()
	}
	return bitmapToBools(accept, n), nil
}

// verifySecp256k1: when every item's key has a registry slot the keyed entries take the batch (verifySecp256k1Keyed); any other
// batch travels as generic tuples with the 64-byte key inline.
func (b *gpuBackend) verifySecp256k1(items []Item) ([]bool, error) {
	if allSlotted(items) {
		return b.verifySecp256k1Keyed(items)
	}
	n := len(items)
	buf := make([]byte, n*tupleBytes)
	for i := range items {
		t := buf[i*tupleBytes : (i+1)*tupleBytes]
		fillRSH(t, &items[i])
		if len(items[i].Key) == 64 {
			copy(t[96:160], items[i].Key)
		} // else: the all-zero key, which is not on the curve
	}
	bitmap := make([]byte, (n+7)/8)
	if rc := C.sbv_secp256k1_verify_batch(u8(buf), C.size_t(n), u8(bitmap)); rc != 0 {
		return nil, lastError()
	}
	return bitmapToBools(bitmap, n), nil
}

func (b *gpuBackend) Verify(scheme Scheme, items []Item) (ok []bool, err error) {
	if len(items) == 0 {
		return nil, nil
	}
	b.on(func() {
		switch scheme {
		case SchemeEd25519:
			ok, err = b.verifyEd25519(items)
		case SchemeSecp256k1:
			ok, err = b.verifySecp256k1(items)
		default:
			ok, err = b.verifyP256(items)
		}
	})
	return ok, err
}

// keysOf lays the items' 64-byte keys back to back; an item without one gets the all-zero key, which is not on either curve.
func keysOf(items []Item) []byte {
	keys := make([]byte, 64*len(items))
	for i := range items {
		if len(items[i].Key) == 64 {
			copy(keys[64*i:], items[i].Key)
		}
	}
	return keys
}

// VerifyMsgs (RawMessageVerifier): raw messages + DER signatures + keys, hashed, parsed and laid out as tuples on the device.
// SchemeP256: the whole batch in one call of the sharded entry (the library splits it by device and by piece; no 2^21 limit; a batch
// that is not worth splitting goes whole to one device).  SchemeSecp256k1: chunks of at most 2^21 on the first device.
func (b *gpuBackend) VerifyMsgs(scheme Scheme, items []Item) (ok []bool, err error) {
	n := len(items)
	if n == 0 {
		return nil, nil
	}
	if scheme != SchemeP256 && scheme != SchemeSecp256k1 {
		return nil, errors.New("gpuverifier: VerifyMsgs takes SchemeP256 or SchemeSecp256k1")
	}
	b.on(func() {
		bitmap := make([]byte, (n+7)/8)
		keys := keysOf(items)
		if scheme == SchemeP256 {
			msgs, moff := packMsgs(func(i int) []byte { return items[i].Msg }, n)
			sigs, soff := packMsgs(func(i int) []byte { return items[i].Sig }, n)
			rc := C.sbv_p256_verify_msgs_sharded(u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])), u8(sigs),
				(*C.uint64_t)(unsafe.Pointer(&soff[0])), u8(keys), C.size_t(n), 0, 0, u8(bitmap), nil, nil)
			if rc != 0 {
				err = lastError()
				return
			}
			ok = bitmapToBools(bitmap, n)
			return
		}
		for lo := 0; lo < n; lo += frontEndMax {
			hi := lo + frontEndMax
			if hi > n {
				hi = n
			}
			m := hi - lo
			msgs, moff := packMsgs(func(i int) []byte { return items[lo+i].Msg }, m)
			sigs, soff := packMsgs(func(i int) []byte { return items[lo+i].Sig }, m)
			rc := C.sbv_secp256k1_verify_msgs(u8(msgs), (*C.uint64_t)(unsafe.Pointer(&moff[0])), u8(sigs),
				(*C.uint64_t)(unsafe.Pointer(&soff[0])), u8(keys[64*lo:]), C.size_t(m), u8(bitmap[lo/8:])) // lo is a multiple of 2^21: whole bitmap bytes
			if rc != 0 {
				err = lastError()
				return
			}
		}
		ok = bitmapToBools(bitmap, n)
	})
	return ok, err
}

// RegisterKey builds the key's comb on the device once (sbv_p256_register_keys: 270 KiB of HBM per key) and remembers
// the slot; registering a key again returns the same slot.  -1 when the device refuses (then the key travels inline).
func (b *gpuBackend) RegisterKey(pub *ecdsa.PublicKey) int32 {
	if pub == nil || pub.X == nil || pub.Y == nil || pub.X.Sign() < 0 || pub.Y.Sign() < 0 || pub.X.BitLen() > 256 || pub.Y.BitLen() > 256 {
		return -1
	}
	k := keyBytes(pub)
	b.mu.Lock()
	if s, hit := b.regs[k]; hit {
		b.mu.Unlock()
		return s
	}
	b.mu.Unlock()
	slot := int32(-1)
	b.on(func() {
		var out C.uint32_t
		if rc := C.sbv_p256_register_keys(u8(k[:]), 1, &out); rc == 0 {
			slot = int32(out)
		}
	})
	if slot >= 0 {
		b.mu.Lock()
		b.regs[k] = slot
		b.mu.Unlock()
	}
	return slot
}

// WidenKey: sbv_p256_widen_keys for one slot (best effort: a slot that gets no wide comb keeps its 8-bit one, verdicts are the same).
func (b *gpuBackend) WidenKey(slot int32) {
	if slot < 0 {
		return
	}
	b.on(func() {
		var s C.uint32_t
		s = C.uint32_t(slot)
		C.sbv_p256_widen_keys(&s, C.size_t(1))
	})
}

// RegisterKeyEd25519 builds the key's 8-bit comb of -A on the device once (sbv_ed25519_register_keys: 384 KiB of HBM per key)
// and remembers the slot; registering the same bytes again returns the same slot.  -1 when the device refuses (the key then
// travels inline).
func (b *gpuBackend) RegisterKeyEd25519(key []byte) int32 {
	if len(key) != 32 {
		return -1
	}
	var k [32]byte
	copy(k[:], key)
	b.mu.Lock()
	if s, hit := b.edRegs[k]; hit {
		b.mu.Unlock()
		return s
	}
	b.mu.Unlock()
	slot := int32(-1)
	b.on(func() {
		var out C.uint32_t
		if rc := C.sbv_ed25519_register_keys(u8(key), 1, &out); rc == 0 {
			slot = int32(out)
		}
	})
	if slot >= 0 {
		b.mu.Lock()
		b.edRegs[k] = slot
		b.mu.Unlock()
	}
	return slot
}

// WidenKeyEd25519: sbv_ed25519_widen_keys for one slot (best effort: a slot without a 16-bit comb keeps its 8-bit one).
func (b *gpuBackend) WidenKeyEd25519(slot int32) {
	if slot < 0 {
		return
	}
	b.on(func() {
		var s C.uint32_t
		s = C.uint32_t(slot)
		C.sbv_ed25519_widen_keys(&s, C.size_t(1))
	})
}

// RegisterKeySecp256k1 builds the key's 8-bit comb on the device once (sbv_secp256k1_register_keys: 270 KiB of HBM per key) and
// remembers the slot; registering the same bytes again returns the same slot.  -1 when the device refuses (the key then
// travels inline).
func (b *gpuBackend) RegisterKeySecp256k1(key []byte) int32 {
	if len(key) != 64 {
		return -1
	}
	var k [64]byte
	copy(k[:], key)
	b.mu.Lock()
	if s, hit := b.k256Regs[k]; hit {
		b.mu.Unlock()
		return s
	}
	b.mu.Unlock()
	slot := int32(-1)
	b.on(func() {
		var out C.uint32_t
		if rc := C.sbv_secp256k1_register_keys(u8(k[:]), 1, &out); rc == 0 {
			slot = int32(out)
		}
	})
	if slot >= 0 {
		b.mu.Lock()
		b.k256Regs[k] = slot
		b.mu.Unlock()
	}
	return slot
}

// WidenKeySecp256k1: sbv_secp256k1_widen_keys for one slot (best effort: a slot without a 16-bit comb keeps its 8-bit one).
func (b *gpuBackend) WidenKeySecp256k1(slot int32) {
	if slot < 0 {
		return
	}
	b.on(func() {
		var s C.uint32_t
		s = C.uint32_t(slot)
		C.sbv_secp256k1_widen_keys(&s, C.size_t(1))
	})
}

// PoolStats is what the grouped P-256 step really holds on the default device (sbv_p256_pool_stats; round 6).  The pools are sized for a
// 288 GB MI355X; a shared or smaller device gets halved pools instead of an error, and a batch whose pools cannot be allocated at all is
// verified by the one-lane kernel — an operator reads here which of the two happened (NomemFallbacks > 0: give the replica more HBM).
type PoolStats struct {
	CacheKeys, GroupsPerBatch uint32 // 0 before the first grouped batch
	Shrunk                    bool   // smaller than asked for
	NomemFallbacks            uint32 // grouped batches that took the one-lane kernel for lack of memory
	HotPool                   uint32 // 16-bit combs of the hot-key pool
	GPUShare                  uint32 // contexts sharing the GPU (SBV_LOGICAL_DEVICES)
}

// PoolStats: sbv_p256_pool_stats.
func (b *gpuBackend) PoolStats() (st PoolStats, err error) {
	b.on(func() {
		var out [6]C.uint32_t
		if rc := C.sbv_p256_pool_stats((*C.uint32_t)(unsafe.Pointer(&out[0]))); rc != 0 {
			err = lastError()
			return
		}
		st = PoolStats{CacheKeys: uint32(out[0]), GroupsPerBatch: uint32(out[1]), Shrunk: out[2] != 0, NomemFallbacks: uint32(out[3]),
			HotPool: uint32(out[4]), GPUShare: uint32(out[5])}
	})
	return st, err
}

// SignBatch: sbv_p256_sign_batch (RFC 6979 nonces on the device; not constant-time — see include/sbv.h).
func (b *gpuBackend) SignBatch(keys [][32]byte, keyIndex []uint32, digests [][32]byte) (sigs [][64]byte, ok []bool, err error) {
	n := len(digests)
	if n == 0 || len(keys) == 0 || len(keyIndex) != n {
		return nil, nil, errors.New("gpuverifier: SignBatch needs keys and one key index per digest")
	}
	kb := make([]byte, 32*len(keys))
	for i := range keys {
		copy(kb[32*i:], keys[i][:])
	}
	db := make([]byte, 32*n)
	for i := range digests {
		copy(db[32*i:], digests[i][:])
	}
	out := make([]byte, 64*n)
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_p256_sign_batch(u8(kb), C.uint32_t(len(keys)), (*C.uint32_t)(unsafe.Pointer(&keyIndex[0])), u8(db), C.size_t(n), u8(out), u8(flags))
		if rc != 0 {
			err = lastError()
		}
	})
	for i := range kb {
		kb[i] = 0
	}
	if err != nil {
		return nil, nil, err
	}
	sigs = make([][64]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		copy(sigs[i][:], out[64*i:64*i+64])
		ok[i] = flags[i] != 0
	}
	return sigs, ok, nil
}

// SignBatchEd25519: sbv_ed25519_expand_keys, then sbv_ed25519_sign_msgs under the records just expanded (RFC 8032 on the device;
// not constant-time — see include/sbv.h).  The records are as secret as the seeds and are zeroed before returning.
func (b *gpuBackend) SignBatchEd25519(seeds [][32]byte, keyIndex []uint32, msgs [][]byte) (sigs [][64]byte, ok []bool, err error) {
	n := len(msgs)
	if n == 0 || len(seeds) == 0 || len(keyIndex) != n {
		return nil, nil, errors.New("gpuverifier: SignBatchEd25519 needs seeds and one key index per message")
	}
	sb := make([]byte, 32*len(seeds))
	for i := range seeds {
		copy(sb[32*i:], seeds[i][:])
	}
	expanded := make([]byte, 96*len(seeds))
	packed, moff := packMsgs(func(i int) []byte { return msgs[i] }, n)
	out := make([]byte, 64*n)
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_ed25519_expand_keys(u8(sb), C.size_t(len(seeds)), u8(expanded), nil)
		if rc == 0 {
			rc = C.sbv_ed25519_sign_msgs(u8(expanded), C.uint32_t(len(seeds)), (*C.uint32_t)(unsafe.Pointer(&keyIndex[0])), u8(packed),
				(*C.uint64_t)(unsafe.Pointer(&moff[0])), C.size_t(n), u8(out), u8(flags))
		}
		if rc != 0 {
			err = lastError()
		}
	})
	for i := range sb {
		sb[i] = 0
	}
	for i := range expanded {
		expanded[i] = 0
	}
	if err != nil {
		return nil, nil, err
	}
	sigs = make([][64]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		copy(sigs[i][:], out[64*i:64*i+64])
		ok[i] = flags[i] != 0
	}
	return sigs, ok, nil
}

// SignBatchSecp256k1: sbv_secp256k1_sign_batch (RFC 6979 nonces on the device; not constant-time — see include/sbv.h).
func (b *gpuBackend) SignBatchSecp256k1(keys [][32]byte, keyIndex []uint32, digests [][32]byte, lowS bool) (sigs [][64]byte, recid []byte, ok []bool, err error) {
	n := len(digests)
	if n == 0 || len(keys) == 0 || len(keyIndex) != n {
		return nil, nil, nil, errors.New("gpuverifier: SignBatchSecp256k1 needs keys and one key index per digest")
	}
	kb := make([]byte, 32*len(keys))
	for i := range keys {
		copy(kb[32*i:], keys[i][:])
	}
	db := make([]byte, 32*n)
	for i := range digests {
		copy(db[32*i:], digests[i][:])
	}
	var mode uint32
	if lowS {
		mode = 1 // SBV_K256_SIGN_LOW_S
	}
	out := make([]byte, 64*n)
	recid = make([]byte, n)
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_secp256k1_sign_batch(u8(kb), C.uint32_t(len(keys)), (*C.uint32_t)(unsafe.Pointer(&keyIndex[0])), u8(db), C.size_t(n), C.uint32_t(mode),
			u8(out), u8(recid), u8(flags))
		if rc != 0 {
			err = lastError()
		}
	})
	for i := range kb {
		kb[i] = 0
	}
	if err != nil {
		return nil, nil, nil, err
	}
	sigs = make([][64]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		copy(sigs[i][:], out[64*i:64*i+64])
		ok[i] = flags[i] != 0
	}
	return sigs, recid, ok, nil
}

// SignMsgs (ECDSAMsgSigner): sbv_p256_sign_msgs / sbv_secp256k1_sign_msgs: SHA-256, RFC 6979 signing and DER on the device, at most
// 2^21 messages per call (not constant-time — see include/sbv.h).
func (b *gpuBackend) SignMsgs(scheme Scheme, keys [][32]byte, keyIndex []uint32, msgs [][]byte, lowS bool) (sigs [][]byte, recid []byte, ok []bool, err error) {
	n := len(msgs)
	if n == 0 || n > frontEndMax || len(keys) == 0 || (keyIndex != nil && len(keyIndex) != n) {
		return nil, nil, nil, errors.New("gpuverifier: SignMsgs needs keys, no key index or one per message, and at most 2^21 messages")
	}
	if scheme != SchemeP256 && scheme != SchemeSecp256k1 {
		return nil, nil, nil, errors.New("gpuverifier: SignMsgs takes SchemeP256 or SchemeSecp256k1")
	}
	kb := make([]byte, 32*len(keys))
	for i := range keys {
		copy(kb[32*i:], keys[i][:])
	}
	var mode uint32
	if lowS {
		mode = 1 // SBV_ECDSA_SIGN_LOW_S
	}
	packed, moff := packMsgs(func(i int) []byte { return msgs[i] }, n)
	out := make([]byte, 72*n) // SBV_ECDSA_DER_MAX each
	soff := make([]uint64, n+1)
	flags := make([]byte, n)
	if scheme == SchemeSecp256k1 {
		recid = make([]byte, n)
	}
	b.on(func() {
		var rc C.int
		var index *uint32 // nil: key i % len(keys), the library's rule for a NULL index
		if keyIndex != nil {
			index = &keyIndex[0]
		}
		if scheme == SchemeP256 {
			rc = C.sbv_p256_sign_msgs(u8(kb), C.uint32_t(len(keys)), (*C.uint32_t)(unsafe.Pointer(index)), u8(packed),
				(*C.uint64_t)(unsafe.Pointer(&moff[0])), C.size_t(n), C.uint32_t(mode), u8(out), (*C.uint64_t)(unsafe.Pointer(&soff[0])), u8(flags))
		} else {
			rc = C.sbv_secp256k1_sign_msgs(u8(kb), C.uint32_t(len(keys)), (*C.uint32_t)(unsafe.Pointer(index)), u8(packed),
				(*C.uint64_t)(unsafe.Pointer(&moff[0])), C.size_t(n), C.uint32_t(mode), u8(out), (*C.uint64_t)(unsafe.Pointer(&soff[0])), u8(recid), u8(flags))
		}
		if rc != 0 {
			err = lastError()
		}
	})
	for i := range kb {
		kb[i] = 0
	}
	if err != nil {
		return nil, nil, nil, err
	}
	sigs = make([][]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		sigs[i] = out[soff[i]:soff[i+1]]
		ok[i] = flags[i] != 0
	}
	return sigs, recid, ok, nil
}

// RecoverBatchSecp256k1: sbv_secp256k1_recover (one device call; nothing secret is involved).
func (b *gpuBackend) RecoverBatchSecp256k1(sigs [][64]byte, recid []byte, digests [][32]byte, lowS bool) (pubs [][64]byte, ok []bool, err error) {
	n := len(sigs)
	if n == 0 || len(recid) != n || len(digests) != n {
		return nil, nil, errors.New("gpuverifier: RecoverBatchSecp256k1 needs one recovery id and one digest per signature")
	}
	sb := make([]byte, 64*n)
	db := make([]byte, 32*n)
	for i := 0; i < n; i++ {
		copy(sb[64*i:], sigs[i][:])
		copy(db[32*i:], digests[i][:])
	}
	var mode uint32
	if lowS {
		mode = 1 // SBV_K256_RECOVER_LOW_S
	}
	out := make([]byte, 64*n)
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_secp256k1_recover(u8(sb), u8(recid), u8(db), C.size_t(n), C.uint32_t(mode), u8(out), u8(flags))
		if rc != 0 {
			err = lastError()
		}
	})
	if err != nil {
		return nil, nil, err
	}
	pubs = make([][64]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		copy(pubs[i][:], out[64*i:64*i+64])
		ok[i] = flags[i] != 0
	}
	return pubs, ok, nil
}

// RecoverAddressesSecp256k1: sbv_secp256k1_recover_addresses (one device call; nothing secret is involved).
func (b *gpuBackend) RecoverAddressesSecp256k1(sigs [][64]byte, recid []byte, digests [][32]byte, lowS bool) (addrs [][20]byte, ok []bool, err error) {
	n := len(sigs)
	if n == 0 || len(recid) != n || len(digests) != n {
		return nil, nil, errors.New("gpuverifier: RecoverAddressesSecp256k1 needs one recovery id and one digest per signature")
	}
	sb := make([]byte, 64*n)
	db := make([]byte, 32*n)
	for i := 0; i < n; i++ {
		copy(sb[64*i:], sigs[i][:])
		copy(db[32*i:], digests[i][:])
	}
	var mode uint32
	if lowS {
		mode = 1 // SBV_K256_RECOVER_LOW_S
	}
	out := make([]byte, 20*n)
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_secp256k1_recover_addresses(u8(sb), u8(recid), u8(db), C.size_t(n), C.uint32_t(mode), u8(out), u8(flags))
		if rc != 0 {
			err = lastError()
		}
	})
	if err != nil {
		return nil, nil, err
	}
	addrs = make([][20]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		copy(addrs[i][:], out[20*i:20*i+20])
		ok[i] = flags[i] != 0
	}
	return addrs, ok, nil
}

// VerifyBatchSchnorr: sbv_secp256k1_schnorr_verify (one device call; nothing secret is involved).
func (b *gpuBackend) VerifyBatchSchnorr(pks [][32]byte, msgs [][32]byte, sigs [][64]byte) (ok []bool, err error) {
	n := len(sigs)
	if n == 0 || len(pks) != n || len(msgs) != n {
		return nil, errors.New("gpuverifier: VerifyBatchSchnorr needs one key and one message per signature")
	}
	pb := make([]byte, 32*n)
	mb := make([]byte, 32*n)
	sb := make([]byte, 64*n)
	for i := 0; i < n; i++ {
		copy(pb[32*i:], pks[i][:])
		copy(mb[32*i:], msgs[i][:])
		copy(sb[64*i:], sigs[i][:])
	}
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_secp256k1_schnorr_verify(u8(pb), u8(mb), u8(sb), C.size_t(n), u8(flags))
		if rc != 0 {
			err = lastError()
		}
	})
	if err != nil {
		return nil, err
	}
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		ok[i] = flags[i] != 0
	}
	return ok, nil
}

// RegisterSchnorrKeys: sbv_secp256k1_schnorr_lift_keys, then sbv_secp256k1_register_keys on the lifted keys, in one visit to the
// device thread.
func (b *gpuBackend) RegisterSchnorrKeys(pks [][32]byte) (slots []uint32, onCurve []bool, err error) {
	m := len(pks)
	if m == 0 {
		return nil, nil, errors.New("gpuverifier: RegisterSchnorrKeys needs a key")
	}
	pb := make([]byte, 32*m)
	for i := range pks {
		copy(pb[32*i:], pks[i][:])
	}
	keys := make([]byte, 64*m)
	flags := make([]byte, m)
	slots = make([]uint32, m)
	b.on(func() {
		rc := C.sbv_secp256k1_schnorr_lift_keys(u8(pb), C.size_t(m), u8(keys), u8(flags))
		if rc == 0 {
			rc = C.sbv_secp256k1_register_keys(u8(keys), C.size_t(m), (*C.uint32_t)(unsafe.Pointer(&slots[0])))
		}
		if rc != 0 {
			err = lastError()
		}
	})
	if err != nil {
		return nil, nil, err
	}
	onCurve = make([]bool, m)
	for i := 0; i < m; i++ {
		onCurve[i] = flags[i] != 0
	}
	return slots, onCurve, nil
}

// VerifyBatchSchnorrKeyed: sbv_secp256k1_schnorr_verify_keyed (one device call; nothing secret is involved).
func (b *gpuBackend) VerifyBatchSchnorrKeyed(msgs [][32]byte, sigs [][64]byte, slots []uint32) (ok []bool, err error) {
	n := len(sigs)
	if n == 0 || len(msgs) != n || len(slots) != n {
		return nil, errors.New("gpuverifier: VerifyBatchSchnorrKeyed needs one message and one slot per signature")
	}
	mb := make([]byte, 32*n)
	sb := make([]byte, 64*n)
	for i := 0; i < n; i++ {
		copy(mb[32*i:], msgs[i][:])
		copy(sb[64*i:], sigs[i][:])
	}
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_secp256k1_schnorr_verify_keyed(u8(mb), u8(sb), (*C.uint32_t)(unsafe.Pointer(&slots[0])), C.size_t(n), u8(flags))
		if rc != 0 {
			err = lastError()
		}
	})
	if err != nil {
		return nil, err
	}
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		ok[i] = flags[i] != 0
	}
	return ok, nil
}

// SignBatchSchnorr: sbv_secp256k1_schnorr_expand_keys, then sbv_secp256k1_schnorr_sign under the records (not constant-time — see
// include/sbv.h).  The records are as secret as the keys and are zeroed with them.
func (b *gpuBackend) SignBatchSchnorr(keys [][32]byte, keyIndex []uint32, msgs [][32]byte, aux [][32]byte) (sigs [][64]byte, pks [][32]byte, ok []bool, err error) {
	n := len(msgs)
	if n == 0 || len(keys) == 0 || len(keyIndex) != n || (aux != nil && len(aux) != n) {
		return nil, nil, nil, errors.New("gpuverifier: SignBatchSchnorr needs keys, one key index per message and no or one aux per message")
	}
	kb := make([]byte, 32*len(keys))
	for i := range keys {
		copy(kb[32*i:], keys[i][:])
	}
	mb := make([]byte, 32*n)
	for i := range msgs {
		copy(mb[32*i:], msgs[i][:])
	}
	var ab []byte
	if aux != nil {
		ab = make([]byte, 32*n)
		for i := range aux {
			copy(ab[32*i:], aux[i][:])
		}
	}
	rec := make([]byte, 64*len(keys))
	pkb := make([]byte, 32*len(keys))
	kok := make([]byte, len(keys))
	out := make([]byte, 64*n)
	flags := make([]byte, n)
	b.on(func() {
		rc := C.sbv_secp256k1_schnorr_expand_keys(u8(kb), C.size_t(len(keys)), u8(rec), u8(pkb), u8(kok))
		if rc == 0 {
			if ab == nil {
				rc = C.sbv_secp256k1_schnorr_sign(u8(rec), C.uint32_t(len(keys)), (*C.uint32_t)(unsafe.Pointer(&keyIndex[0])), u8(mb), nil, C.size_t(n),
					u8(out), u8(flags))
			} else {
				rc = C.sbv_secp256k1_schnorr_sign(u8(rec), C.uint32_t(len(keys)), (*C.uint32_t)(unsafe.Pointer(&keyIndex[0])), u8(mb), u8(ab), C.size_t(n),
					u8(out), u8(flags))
			}
		}
		if rc != 0 {
			err = lastError()
		}
	})
	for i := range kb {
		kb[i] = 0
	}
	for i := range rec {
		rec[i] = 0
	}
	if err != nil {
		return nil, nil, nil, err
	}
	sigs = make([][64]byte, n)
	ok = make([]bool, n)
	for i := 0; i < n; i++ {
		copy(sigs[i][:], out[64*i:64*i+64])
		ok[i] = flags[i] != 0
	}
	pks = make([][32]byte, len(keys))
	for i := range pks {
		copy(pks[i][:], pkb[32*i:32*i+32])
	}
	return sigs, pks, ok, nil
}

func (b *gpuBackend) Close() { close(b.jobs) }

// DecodeKeysSEC1: sbv_p256_decode_keys / sbv_secp256k1_decode_keys on the keys packed back to back (one device call; nothing secret
// is involved).
func (b *gpuBackend) DecodeKeysSEC1(scheme Scheme, keys [][]byte) (pubs [][64]byte, ok []bool, err error) {
	m := len(keys)
	if m == 0 || (scheme != SchemeP256 && scheme != SchemeSecp256k1) {
		return nil, nil, errors.New("gpuverifier: DecodeKeysSEC1 needs a key and an ECDSA scheme")
	}
	offs := make([]uint64, m+1)
	for i := range keys {
		offs[i+1] = offs[i] + uint64(len(keys[i]))
	}
	kb := make([]byte, offs[m]+1) // never empty: the entry refuses a null key array
	for i := range keys {
		copy(kb[offs[i]:], keys[i])
	}
	out := make([]byte, 64*m)
	flags := make([]byte, m)
	b.on(func() {
		var rc C.int
		if scheme == SchemeSecp256k1 {
			rc = C.sbv_secp256k1_decode_keys(u8(kb), (*C.uint64_t)(unsafe.Pointer(&offs[0])), C.size_t(m), u8(out), u8(flags))
		} else {
			rc = C.sbv_p256_decode_keys(u8(kb), (*C.uint64_t)(unsafe.Pointer(&offs[0])), C.size_t(m), u8(out), u8(flags))
		}
		if rc != 0 {
			err = lastError()
		}
	})
	if err != nil {
		return nil, nil, err
	}
	pubs = make([][64]byte, m)
	ok = make([]bool, m)
	for i := 0; i < m; i++ {
		copy(pubs[i][:], out[64*i:64*i+64])
		ok[i] = flags[i] != 0
	}
	return pubs, ok, nil
}
