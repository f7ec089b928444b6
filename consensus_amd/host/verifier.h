// verifier.h — C++ mirror of the reference's plugin pair for this path:
//   api.Verifier  pkg/api/dependencies.go:54-71   (same method names, argument meaning, error behaviour)
//   api.Signer    pkg/api/dependencies.go:46-52
// written in C++ because the reference is compiled code and this image has no Go toolchain; the Go
// cgo adapter a maintainer would add is in INTEGRATION.md and has exactly this structure.
//
// Error behaviour: Go's `error == nil` <=> Status::OK.  Status::INVALID is the Go `error` the
// protocol acts on (vote dropped: internal/bft/view.go:839-842; proposal rejected and leader accused:
// view.go:387-392; request not pooled: controller.go:239-245).  Status::UNAVAILABLE means the
// backend could not answer (device fault, library missing): the Go adapter then verifies with stock
// crypto/ecdsa — this C++ mirror has no CPU verifier on purpose and surfaces the condition instead
// of ever turning it into INVALID.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "formats.h"

namespace sbvhost {

struct Status {
    enum Code { OK = 0, INVALID = 1, UNAVAILABLE = 2 } code = OK;
    std::string msg;
    bool ok() const { return code == OK; }
    static Status Ok() { return Status(); }
    static Status Invalid(const std::string& m) { Status s; s.code = INVALID; s.msg = m; return s; }
    static Status Unavailable(const std::string& m) { Status s; s.code = UNAVAILABLE; s.msg = m; return s; }
};

// What sits below the seam: n tuples -> accept bitmap; returns 0 or a negative infrastructure error
// (include/sbv.h convention).  The product backend is libsbv.so; tests may inject a stand-in, the
// way the reference's own tests inject mocks.VerifierMock (internal/bft/mocks/verifier_mock.go).
class Backend {
 public:
    virtual ~Backend() {}
    virtual int verify(const uint8_t* tuples, size_t n, uint8_t* bitmap) = 0;
    // Optional registered-key form (include/sbv.h: sbv_p256_register_keys / verify_batch_keyed).
    // register_key returns a slot >= 0, or -1 when the backend has no key registry (then callers
    // use verify() with the key carried in the tuple).
    virtual long register_key(const uint8_t q[64]) { (void)q; return -1; }
    // The slot belongs to a consenter: a key that signs every vote of every decision of the epoch (internal/bft/view.go:531-541,
    // 631, 834).  The product backend gives it a wide comb (include/sbv.h: sbv_p256_widen_keys); a no-op elsewhere.
    virtual void widen_key(long slot) { (void)slot; }
    virtual uint64_t keyed_batches() { return 0; }      // test hook: how many verify_keyed batches ran
    virtual uint64_t widened_keys() { return 0; }       // test hook: how many distinct slots widen_key was given
    virtual std::vector<uint32_t> last_k256_slots() { return {}; }      // test hook: the slots of the last verify_k256_keyed batch
    // Page-locked staging memory (include/sbv.h: sbv_host_alloc); nullptr = none available, the caller uses the heap
    virtual void* host_alloc(size_t bytes) { (void)bytes; return nullptr; }
    virtual void host_free(void* p) { (void)p; }
    // Ed25519 variant (include/sbv.h: sbv_ed25519_verify_batch): n tuples of 128 bytes R|S|A|k.  -2 when unsupported.
    virtual int verify_ed25519(const uint8_t* tuples128, size_t n, uint8_t* bitmap) { (void)tuples128; (void)n; (void)bitmap; return -2; }
    // Registered Ed25519 keys (include/sbv.h: sbv_ed25519_register_keys): a slot >= 0 for the 32-byte encoding, or -1 when the backend
    // has no Ed25519 registry (callers then keep A in the 128-byte tuple).  widen_key_ed25519: a 16-bit comb for a consenter's slot.
    virtual long register_key_ed25519(const uint8_t a[32]) { (void)a; return -1; }
    virtual void widen_key_ed25519(long slot) { (void)slot; }
    // n records of 96 bytes R|S|k + slots (sbv_ed25519_verify_batch_keyed); -2 when unsupported
    virtual int verify_ed25519_keyed(const uint8_t* rsk, const uint32_t* slots, size_t n, uint8_t* bitmap) {
        (void)rsk; (void)slots; (void)n; (void)bitmap; return -2;
    }
    // n signatures of 64 bytes + raw messages + slots, k hashed by the backend (sbv_ed25519_verify_msgs_keyed); -2 when unsupported
    virtual int verify_ed25519_msgs_keyed(const uint8_t* sigs, const uint8_t* msgs, const uint64_t* moff, const uint32_t* slots, size_t n,
                                          uint8_t* bitmap) {
        (void)sigs; (void)msgs; (void)moff; (void)slots; (void)n; (void)bitmap; return -2;
    }
    // secp256k1 variant (include/sbv.h: sbv_secp256k1_verify_batch): n tuples of 160 bytes, same layout as verify().  -2 when unsupported.
    virtual int verify_k256(const uint8_t* tuples, size_t n, uint8_t* bitmap) { (void)tuples; (void)n; (void)bitmap; return -2; }
    // Registered secp256k1 keys (include/sbv.h: sbv_secp256k1_register_keys): a slot >= 0 for the 64 key bytes, or -1 when the backend
    // has no registry for this curve (callers then keep the key in the 160-byte tuple).  The registry is the curve's own: its slots
    // mean nothing to verify_keyed.  widen_key_k256: a 16-bit comb for a consenter's slot.
    virtual long register_key_k256(const uint8_t q[64]) { (void)q; return -1; }
    virtual void widen_key_k256(long slot) { (void)slot; }
    // n records of 96 bytes r|s|hash + slots (sbv_secp256k1_verify_batch_keyed); -2 when unsupported
    virtual int verify_k256_keyed(const uint8_t* rsh, const uint32_t* slots, size_t n, uint8_t* bitmap) {
        (void)rsh; (void)slots; (void)n; (void)bitmap; return -2;
    }
    // raw messages + DER signatures + slots, SHA-256 and the DER parse by the backend (sbv_secp256k1_verify_msgs_keyed); -2 when unsupported
    virtual int verify_k256_msgs_keyed(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff,
                                       const uint32_t* slots, size_t n, uint8_t* bitmap) {
        (void)msgs; (void)moff; (void)sigs; (void)soff; (void)slots; (void)n; (void)bitmap; return -2;
    }
    // secp256k1 public-key recovery (include/sbv.h: sbv_secp256k1_recover): n signatures r|s + recovery ids 0..3 + digests -> n keys
    // Qx|Qy and ok[i] = 1 per recovered key (a refused input: 64 zero bytes); -2 when unsupported
    virtual int recover_k256(const uint8_t* sigs, const uint8_t* recid, const uint8_t* digests, size_t n, uint8_t* pubs, uint8_t* ok) {
        (void)sigs; (void)recid; (void)digests; (void)n; (void)pubs; (void)ok; return -2;
    }
    // recover_k256 with the signer's 20-byte address Keccak-256(Qx | Qy)[12:] in place of the key (include/sbv.h:
    // sbv_secp256k1_recover_addresses): addrs n x 20 bytes, ok as recover_k256 (a refused input: 20 zero bytes); -2 when unsupported
    virtual int recover_addresses_k256(const uint8_t* sigs, const uint8_t* recid, const uint8_t* digests, size_t n, uint8_t* addrs, uint8_t* ok) {
        (void)sigs; (void)recid; (void)digests; (void)n; (void)addrs; (void)ok; return -2;
    }
    // Keccak-256 of n messages (include/sbv.h: sbv_keccak256_msgs): message i is msgs[moff[i] .. moff[i+1]), moff starts at 0 and never
    // decreases -> digests n x 32.  The default is a CPU loop over the host form (k256_host.cc); the GPU backend makes one device call.
    // 0, or the backend's error code.
    virtual int keccak256_msgs(const uint8_t* msgs, const uint64_t* moff, size_t n, uint8_t* digests);
    // BIP-340 Schnorr over secp256k1 (include/sbv.h: sbv_secp256k1_schnorr_verify, _sign): x-only keys n x 32, messages n x 32,
    // signatures n x 64 -> ok[i] = 1 per valid signature; records n_keys x 64 from the expansion, key_index (or null: i % n_keys),
    // aux n x 32 (or null: zero bytes) -> signatures and ok.  The default is a CPU loop over the host forms (k256_host.cc); the GPU
    // backend makes one device call.  0, or the backend's error code.
    virtual int schnorr_verify_k256(const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs, size_t n, uint8_t* ok);
    virtual int schnorr_sign_k256(const uint8_t* expanded, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs, const uint8_t* aux,
                                  size_t n, uint8_t* sigs, uint8_t* ok);
    // BIP-340 against registered secp256k1 keys (include/sbv.h: sbv_secp256k1_schnorr_verify_keyed): messages n x 32, signatures n x 64
    // and slots of register_key_k256 -> ok[i] = 1 per valid signature under the slot's Qx; an unknown or invalid slot is a reject.  -2
    // when the backend has no registry; the callback backend loops over the host form, the GPU backend makes one device call.
    virtual int schnorr_verify_keyed_k256(const uint8_t* msgs, const uint8_t* sigs, const uint32_t* slots, size_t n, uint8_t* ok) {
        (void)msgs; (void)sigs; (void)slots; (void)n; (void)ok; return -2;
    }
    virtual int verify_keyed(const uint8_t* rsh, const uint32_t* slots, size_t n, uint8_t* bitmap) {
        (void)rsh; (void)slots; (void)n; (void)bitmap; return -2;
    }
    // Optional device front end (sbv_p256_verify_msgs_keyed): raw messages + DER signatures + slots.
    // Returns -2 when unsupported.
    virtual int verify_msgs_keyed(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff,
                                  const uint32_t* slots, size_t n, uint8_t* bitmap) {
        (void)msgs; (void)moff; (void)sigs; (void)soff; (void)slots; (void)n; (void)bitmap; return -2;
    }
    // Raw messages for signers WITHOUT a slot (include/sbv.h: sbv_p256_verify_msgs, sbv_secp256k1_verify_msgs): raw messages + DER
    // signatures + the signers' keys, n x 64 bytes Qx | Qy; SHA-256, the DER parse and the tuple layout by the backend.  -2 when
    // unsupported: the caller builds the tuples itself.  The callback backend loops over SHA-256, the strict parse and the callback; the
    // GPU backend makes one device call (P-256 above 32 768 requests: the sharded entry, as verify_msgs_keyed).
    virtual int verify_msgs(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n,
                            uint8_t* bitmap) {
        (void)msgs; (void)moff; (void)sigs; (void)soff; (void)keys; (void)n; (void)bitmap; return -2;
    }
    virtual int verify_msgs_k256(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n,
                                 uint8_t* bitmap) {
        (void)msgs; (void)moff; (void)sigs; (void)soff; (void)keys; (void)n; (void)bitmap; return -2;
    }
    // ... and the Ed25519 form (sbv_ed25519_verify_msgs): n signatures of 64 bytes + n keys of 32 bytes + raw messages, k hashed by the
    // backend; -2 when unsupported
    virtual int verify_ed25519_msgs(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* moff, size_t n, uint8_t* bitmap) {
        (void)sigs; (void)pks; (void)msgs; (void)moff; (void)n; (void)bitmap; return -2;
    }
    virtual uint64_t msgs_batches() { return 0; }       // test hook: how many batches the three forms above ran
    // SEC1 public keys -> 64 bytes X | Y each (include/sbv.h: sbv_p256_decode_keys, sbv_secp256k1_decode_keys): key i is
    // keys[koff[i] .. koff[i+1]), koff starts at 0 and never decreases, or null for the 33-byte stride; keys64 m x 64, ok m bytes or
    // null; a refused key is 64 zero bytes.  The default is a CPU loop over the host forms (sec1_host.cc, one square root per
    // compressed key); the GPU backend makes one device call.  0, or the backend's error code.
    virtual int decode_keys(bool k256, const uint8_t* keys, const uint64_t* koff, size_t m, uint8_t* keys64, uint8_t* ok);
    // verify_msgs / verify_msgs_k256 with the signers' keys as SEC1 octet strings (include/sbv.h: sbv_p256_verify_msgs_sec1,
    // sbv_secp256k1_verify_msgs_sec1): bit i = the verdict under the 64 bytes decode_keys gives for key i, a refused key is a reject.
    // The default is decode_keys followed by verify_msgs / verify_msgs_k256 (-2 when those are unsupported); the GPU backend makes one
    // device call, the keys decoded in front of the front end.
    virtual int verify_msgs_sec1(bool k256, const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys,
                                 const uint64_t* koff, size_t n, uint8_t* bitmap);
};
// The host route of a batch of ECDSA requests (what VerifyProposal's workers build when no front end takes the batch): tuple i = strict
// DER parse of signature i (zeros when refused) | SHA-256(message i) | keys[64 i ..), n x 160 bytes, over the worker pool.
void make_tuples_ecdsa(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n,
                       uint8_t* tuples);
std::shared_ptr<Backend> make_sbv_backend(int device);     // device >= 0: sbv_init(device); device < 0: sbv_init_all() + the sharded entry
typedef int (*backend_fn)(const uint8_t* tuples, size_t n, uint8_t* bitmap, void* user);
std::shared_ptr<Backend> make_callback_backend(backend_fn fn, void* user, bool with_key_registry = false);

// A lock for critical sections of a few dozen instructions that N-1 threads hit in the same microsecond (a burst of commit
// votes: view.go:537-541).  Under that pattern std::mutex parks the losers in the kernel — one futex wake-up (5-10 us) per
// hand-over, 15-24 us until the last of 15 votes was queued (profiles/r04/m2_trace_r04h.txt) — a spinning lock hands over in
// ~100 ns.  BasicLockable: works with std::lock_guard / std::unique_lock.
class SpinLock {
 public:
    void lock() {
        // test-and-test-and-set: the waiters spin on a shared (read-only) copy of the line and only the one that sees it free
        // tries the exchange, so a hand-over is one line transfer instead of a storm of them
        while (f_.exchange(true, std::memory_order_acquire)) {
            while (f_.load(std::memory_order_relaxed)) {
#if defined(__x86_64__) || defined(__i386__)
                __builtin_ia32_pause();
#endif
            }
        }
    }
    void unlock() { f_.store(false, std::memory_order_release); }

 private:
    std::atomic<bool> f_{false};
};

struct CoalescerStats {
    uint64_t calls = 0;        // single-signature submissions
    uint64_t batches = 0;      // backend invocations
    uint64_t max_batch = 0;
};

// Collects concurrent single-tuple submissions into one backend batch: the first submitter of a burst becomes its
// leader (no dispatcher thread to wake), waits up to `max_wait` for more (or until `max_batch`), and ships them in one
// call.  This is what turns the <= N-1 goroutines of View.processCommits (view.go:537-541) into one
// GPU micro-batch.  submit_many() bypasses the wait (a VerifyProposal already is a batch).
class Coalescer {
 public:
    Coalescer(std::shared_ptr<Backend> be, size_t max_batch, std::chrono::microseconds max_wait);
    ~Coalescer();
    // 1 = accept, 0 = reject, <0 = backend error
    // slot >= 0: the signer's key is registered with the backend (tuple[96..160) is then ignored)
    // ed25519 = true: `tuple` holds a 128-byte R|S|A|k tuple instead (one Verifier = one scheme, so a burst never mixes)
    // err (optional): on a backend error, the library's error text as the DISPATCHER thread saw it (sbv_last_error() is per
    // thread, and the failing call ran there, not on the submitter)
    int submit(const uint8_t tuple[160], long slot = -1, bool ed25519 = false, bool k256 = false, std::string* err = nullptr);
    int submit_many_ed25519(const uint8_t* tuples128, size_t n, uint8_t* bitmap);
    int submit_many_ed25519_msgs_keyed(const uint8_t* sigs, const uint8_t* msgs, const uint64_t* moff, const uint32_t* slots, size_t n, uint8_t* bitmap);
    int submit_many_k256(const uint8_t* tuples, size_t n, uint8_t* bitmap);
    // the registered-key forms of the secp256k1 Verifier (-2 when the backend has none: the caller takes submit_many_k256)
    int submit_many_k256_keyed(const uint8_t* rsh, const uint32_t* slots, size_t n, uint8_t* bitmap);
    int submit_many_k256_msgs_keyed(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint32_t* slots, size_t n,
                                    uint8_t* bitmap);
    int submit_many(const uint8_t* tuples, size_t n, uint8_t* bitmap);
    int submit_many_keyed(const uint8_t* rsh, const uint32_t* slots, size_t n, uint8_t* bitmap);
    // raw messages + DER signatures + slots through the backend's front end (-2 when it has none)
    int submit_many_msgs_keyed(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint32_t* slots, size_t n,
                               uint8_t* bitmap);
    // raw messages + DER signatures + the signers' keys (no slots) through the backend's generic front ends (-2 when it has none)
    int submit_many_msgs(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n, uint8_t* bitmap);
    int submit_many_k256_msgs(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n,
                              uint8_t* bitmap);
    int submit_many_ed25519_msgs(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* moff, size_t n, uint8_t* bitmap);
    Backend& backend() { return *be_; }
    CoalescerStats stats();
    // How many submissions a burst is expected to bring (N-1 commit votes: view.go:537-541); the dispatcher ships as soon as
    // that many are queued instead of sitting out the window.  0 = unknown.
    void set_burst_hint(size_t n) { burst_hint_.store(n, std::memory_order_relaxed); }

 private:
    struct Job { uint8_t tuple[160]; long slot = -1; bool ed25519 = false; bool k256 = false; int result = -100; std::string err; std::atomic<bool> done{false}; double t_push = 0; };
    void serve_as_leader(const std::atomic<bool>* own_done);
    std::shared_ptr<Backend> be_;
    size_t max_batch_;
    std::chrono::microseconds max_wait_;
    SpinLock mu_;                           // the queue, the leader flag, the statistics
    std::mutex sleep_mu_;                   // only for submitters that gave up spinning (cv_done_)
    std::condition_variable cv_done_;
    std::atomic<int> sleepers_{0};
    bool leader_ = false;                   // under mu_: some submitter is serving the queue
    std::atomic<bool> leader_flag_{false};  // the same, readable by the spinning submitters without the lock
    std::deque<Job*> q_;
    std::atomic<size_t> qn_{0};            // q_.size(), readable without the lock by the spinning dispatcher
    std::atomic<size_t> burst_hint_{0};
    CoalescerStats st_;
};

// Signature scheme of a Verifier / Signer pair.  P256: ECDSA over SHA-256, DER signatures, 64-byte Qx|Qy keys (Go
// crypto/ecdsa.VerifyASN1).  ED25519: the BASELINE.json configs[4] variant — 64-byte R|S signatures, 32-byte keys
// (Go crypto/ed25519.Verify); registered-key slots do not apply (the device groups by key inside each batch).
// SECP256K1: ECDSA over SHA-256 with DER signatures and 64-byte keys exactly like P256, on the other curve
// (include/sbv.h: sbv_secp256k1_verify_batch); consenters and registered clients take slots of the curve's own registry
// (sbv_secp256k1_register_keys), and batches whose signers all have one go through the keyed entries.
enum class Scheme { P256 = 0, ED25519 = 1, SECP256K1 = 2 };

struct VerifierOptions {
    Scheme scheme = Scheme::P256;
    size_t coalesce_max = 4096;
    std::chrono::microseconds coalesce_wait{50};
    bool cache_verified = true;     // commit sigs of sequence s reappear at s+1 (view.go:376, 630)
    // false: client keys are NOT given comb slots on the device; request signatures then travel as generic tuples with the
    // key inline and the device groups them by key inside each batch (what an open client population gets: a replica
    // cannot pre-register keys it has never seen).  Consenter keys are always registered.
    bool device_client_keys = true;
};

class Verifier {
 public:
    Verifier(std::shared_ptr<Backend> be, const VerifierOptions& opt = VerifierOptions());
    ~Verifier();

    // key registry (id -> public key: 64 bytes Qx|Qy, or the first 32 bytes = A_enc under Scheme::ED25519); the kernel
    // re-validates every key
    void RegisterConsenter(uint64_t id, const uint8_t* q);
    void RegisterClient(const std::string& client_id, const uint8_t* q);
    void SetVerificationSequence(uint64_t s);
    void SetDeviceClientKeys(bool on) { std::lock_guard<SpinLock> lk(mu_); opt_.device_client_keys = on; }     // applies to clients registered afterwards

    // ---- api.Verifier ---------------------------------------------------------------------------
    Status VerifyProposal(const Proposal& proposal, std::vector<RequestInfo>* requests);
    Status VerifyRequest(const bytes& val, RequestInfo* info);
    Status VerifyConsenterSig(const Signature& signature, const Proposal& prop, bytes* aux);
    Status VerifySignature(const Signature& signature);
    uint64_t VerificationSequence();
    std::vector<RequestInfo> RequestsFromProposal(const Proposal& proposal);
    bytes AuxiliaryData(const bytes& msg);
    // ---- api.RequestInspector (pkg/api/dependencies.go:80-83) ------------------------------------
    RequestInfo RequestID(const bytes& req);

    // Batch form used by decision replay / sync (pkg/types/types.go:31-34): all signatures of many
    // decisions in one backend call; out[i] = 1 accept / 0 reject.
    Status VerifyConsenterSigBatch(const std::vector<Signature>& sigs, const std::vector<const Proposal*>& props,
                                   std::vector<uint8_t>* out);
    // Scheme::SECP256K1 only: the signers of n signatures that carry no key, as traffic shaped like Ethereum's does: sigs65 = n x 65
    // bytes r | s | v with v = the recovery id as 0..3 or 27..30, digests = n x 32 bytes -> pubs n x 64 bytes Qx|Qy, ok[i] = 1 per
    // recovered key (otherwise 64 zero bytes; any other v is refused).  One backend call (sbv_secp256k1_recover on the device); what an
    // integrator calls before RegisterClient / register_key_k256.  INVALID under another scheme, UNAVAILABLE on a backend error.
    Status RecoverSigners(const uint8_t* sigs65, const uint8_t* digests, size_t n, uint8_t* pubs, uint8_t* ok);
    // Scheme::SECP256K1 only: RecoverSigners with the signers' 20-byte addresses Keccak-256(Qx | Qy)[12:] in place of the keys, which
    // is what traffic shaped like Ethereum's compares (ecrecover): same sigs65 and `v` rules (0..3 or 27..30, anything else refused),
    // addrs20 = n x 20 bytes, ok[i] = 1 per recovered signer (otherwise 20 zero bytes).  One backend call
    // (sbv_secp256k1_recover_addresses on the device).  EIP-155 `v`, EIP-191 prefixes and EIP-55 checksums are the caller's formatting.
    Status RecoverAddresses(const uint8_t* sigs65, const uint8_t* digests, size_t n, uint8_t* addrs20, uint8_t* ok);
    // Keccak-256 (Ethereum's keccak256) of n messages under any scheme: the digests RecoverAddresses and RecoverSigners take.  One
    // backend call (sbv_keccak256_msgs on the device, a CPU loop otherwise).  INVALID for an offset table that does not start at 0 or
    // decreases, UNAVAILABLE on a backend error.
    Status Keccak256Batch(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, uint8_t* digests);
    // Scheme::SECP256K1 only: BIP-340 Schnorr verification of n signatures as traffic shaped like Bitcoin's carries them since Taproot:
    // pks = n x 32 bytes x-only keys, msgs = n x 32 bytes, sigs = n x 64 bytes R.x | s -> ok[i] = 1 per valid signature.  One backend
    // call (sbv_secp256k1_schnorr_verify on the device, a CPU loop otherwise).  INVALID under another scheme, UNAVAILABLE on a backend error.
    Status VerifySchnorr(const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs, size_t n, uint8_t* ok);
    // Scheme::SECP256K1 only: BIP-340 against the backend's registered secp256k1 keys, for a fixed key set that signs again and again.
    // RegisterSchnorrKey: an x-only key -> its slot in the registry RegisterConsenter / RegisterClient use on this curve (lift_x, then
    // register_key_k256), -1 when the backend has no registry or the scheme is another; a key off the curve gets a slot too, against
    // which every signature is rejected.  VerifySchnorrKeyed: msgs n x 32, sigs n x 64, slots n x u32 -> ok[i], one backend call
    // (sbv_secp256k1_schnorr_verify_keyed on the device).  INVALID under another scheme, UNAVAILABLE without a registry or on an error.
    long RegisterSchnorrKey(const uint8_t pk[32]);
    Status VerifySchnorrKeyed(const uint8_t* msgs, const uint8_t* sigs, const uint32_t* slots, size_t n, uint8_t* ok);
    // The ECDSA schemes only: public keys as SEC1 octet strings (65 bytes 04 | X | Y or 33 bytes 02/03 | X: what an X.509
    // SubjectPublicKeyInfo, Go's elliptic.Marshal / MarshalCompressed and secp256k1 traffic carry).  DecodeKeys: m keys packed back to
    // back with m + 1 offsets (null: the 33-byte stride) -> keys64 m x 64 bytes X | Y and ok[i] (may be null), one backend call
    // (sbv_p256_decode_keys / sbv_secp256k1_decode_keys on the device, a CPU loop otherwise).  INVALID under Scheme::ED25519 or for a
    // bad offset table, UNAVAILABLE on a backend error.  RegisterConsenterSec1 / RegisterClientSec1: decode, then RegisterConsenter /
    // RegisterClient on the 64 bytes — the key is decoded once, at registration, and every later signature of that signer goes through
    // the scheme's registered-key entries; false, and nothing registered, for a refused key.
    Status DecodeKeys(const uint8_t* keys, const uint64_t* key_offsets, size_t m, uint8_t* keys64, uint8_t* ok);
    // The unregistered raw-message route for a caller that holds SEC1 keys: n messages, DER signatures and SEC1 keys, each packed back to
    // back with n + 1 offsets (key_offsets null: the 33-byte stride) -> bitmap, bit i = signature i verifies over SHA-256(message i)
    // under key i; a key that does not decode is a reject.  One backend call (the _sec1 entries on the device: the keys are decoded
    // once per signature there; for signers that repeat, register them instead).  n <= 2^21.  INVALID under Scheme::ED25519, for a bad
    // offset table or a larger n; UNAVAILABLE on a backend error.
    Status VerifyMsgsSec1(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets, const uint8_t* keys,
                          const uint64_t* key_offsets, size_t n, uint8_t* bitmap);
    bool RegisterConsenterSec1(uint64_t id, const uint8_t* key, size_t len);
    bool RegisterClientSec1(const std::string& client_id, const uint8_t* key, size_t len);
    CoalescerStats stats() { return co_.stats(); }
    Scheme scheme() const { return opt_.scheme; }

 private:
    bool consenter_key(uint64_t id, uint8_t q[64], long* slot = nullptr);
    bool client_key(const std::string& id, uint8_t q[64], long* slot = nullptr);
    void make_tuple(const uint8_t q[64], const bytes& msg, const bytes& sig_der, uint8_t out[160]);
    static void make_tuple_ed25519(const uint8_t a_enc[32], const bytes& msg, const bytes& sig, uint8_t out[128]);
    bool ed() const { return opt_.scheme == Scheme::ED25519; }
    bool k256() const { return opt_.scheme == Scheme::SECP256K1; }
    size_t key_bytes() const { return ed() ? 32 : 64; }
    Status verify_one(const uint8_t q[64], const bytes& msg, const bytes& sig, long slot = -1);
    std::string cache_key(const uint8_t q[64], const bytes& msg, const bytes& sig) const;
    SpinLock mu_;
    std::map<uint64_t, bytes> consenters_;
    std::map<uint64_t, long> consenter_slot_;
    std::map<std::string, long> client_slot_;       // backend key slot per client, -1 without a registry
    std::map<std::string, bytes> clients_;
    uint64_t seq_ = 0;
    VerifierOptions opt_;
    Coalescer co_;
    SpinLock cache_mu_;
    std::unordered_map<std::string, bool> cache_;
    // Grow-only staging arrays of the raw-messages batch path, page-locked when the backend offers it: handing
    // pageable memory to a ~100 MB batch costs more in the runtime's pinning than the kernels take.
    struct Staging {
        void* p = nullptr; size_t cap = 0; bool pinned = false;
    };
    void* staging(Staging& s, size_t bytes);
    void staging_release(Staging& s);
    std::mutex staging_mu_;
    Staging st_msgs_, st_sigs_, st_moff_, st_soff_, st_slots_;
    // Proposal.Digest() once per Proposal object (formats.h: ProposalDigestSlot).  digest_of: the digest, computed here by the
    // first caller (concurrent first callers wait for it instead of hashing the same megabytes N - 1 times) or awaited from the
    // prefetch.  digest_prefetch: VerifyProposal hands ASN.1 + SHA-256 of the proposal to a worker thread, so that it runs
    // beside the backend call and the prepare round (a K = 10 000 proposal is 1.7 MB: ~1.2 ms of marshalling + SHA-256 that the
    // first commit vote used to pay); the worker reads the caller's object only until it holds the marshalled bytes, and
    // VerifyProposal does not return before that (the caller may drop the proposal afterwards).
    bytes digest_of(const Proposal& p);
    void digest_prefetch(const Proposal& p, std::shared_ptr<ProposalDigestSlot>* slot_out);
    void digest_worker();
    struct DigestJob { const Proposal* p; std::shared_ptr<ProposalDigestSlot> slot; };
    std::mutex dw_mu_;
    std::condition_variable dw_cv_;
    std::vector<DigestJob> dw_jobs_;
    std::thread dw_thread_;
    bool dw_stop_ = false;
};

// api.Signer for one node (pkg/api/dependencies.go:46-52)
class Signer {
 public:
    // private_key: the P-256 / secp256k1 scalar d, or the RFC 8032 seed under Scheme::ED25519
    Signer(uint64_t id, const uint8_t private_key[32], Scheme scheme = Scheme::P256);
    uint64_t id() const { return id_; }
    const uint8_t* public_key() const { return q_; }                        // 64 bytes Qx|Qy, or 32 bytes A_enc (+ 32 zero bytes)
    bytes Sign(const bytes& msg);                                           // DER over SHA-256(msg), or the 64-byte Ed25519 R|S
    // one signature per message, equal to Sign of each; with a device initialised Ed25519 is one sbv_ed25519_sign_msgs call and
    // P-256 / secp256k1 one sbv_p256_sign_msgs / sbv_secp256k1_sign_msgs call: hashing and DER on the device (verifier.cc).  low_s:
    // the ECDSA schemes return s <= (n-1)/2
    std::vector<bytes> SignBatch(const std::vector<bytes>& msgs, bool low_s = false);
    bytes SignLowS(const bytes& msg);                                       // Sign with s > (n-1)/2 replaced by n - s (ECDSA schemes)
    Signature SignProposal(const Proposal& proposal, const bytes& auxiliary_input);
    ~Signer() { volatile uint8_t* p = ed_rec_; for (int i = 0; i < 96; ++i) p[i] = 0; }

 private:
    uint64_t id_;
    Scheme scheme_;
    uint8_t d_[32], q_[64];
    uint8_t ed_rec_[96] = {0};          // Ed25519: the expanded record of sbv_ed25519_expand_keys (a mod L | prefix | A_enc), from the first SignBatch on
    bool ed_rec_ready_ = false;
};

// f = (n-1)/3, q = ceil((n+f+1)/2)   internal/bft/util.go:183-187
void compute_quorum(uint64_t n, int* q, int* f);

}  // namespace sbvhost
