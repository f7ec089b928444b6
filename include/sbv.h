/*
 * sbv.h — C-ABI of libsbv.so: MI355X (gfx950) batch signature verification for SmartBFT.
 *
 * This is the drop-in boundary below the reference's plugin seam
 *     api.Verifier            /root/reference/pkg/api/dependencies.go:54-71
 * A Go (cgo) implementation of api.Verifier — see INTEGRATION.md — parses / hashes each
 * types.Signature{ID, Value, Msg} (pkg/types/types.go:25-29) or request into one 160-byte
 * tuple and hands whole batches to the functions below.  The reference has no FFI for this
 * path (every Verifier it ships is a no-op: examples/naive_chain/node.go:86-96,
 * test/test_app.go:231-248); each entry point cites the reference call site whose work it
 * takes over.
 *
 * Conventions
 *   - every function returns SBV_OK (0) or a negative SBV_E* infrastructure error.  A return
 *     value NEVER means "signature invalid": verdicts are only in the accept bitmap, and a
 *     caller must treat <0 as "could not verify" (fall back to its own CPU path) — returning
 *     a Go error for a device fault would depose an honest leader (internal/bft/view.go:387-392).
 *   - tuple layout (big-endian, 5 x 32 bytes):  r | s | hash | Qx | Qy
 *       r, s   : signature integers (from sbv_p256_parse_der; a parse failure is encoded as
 *                r = s = 0, which the range check rejects)
 *       hash   : leftmost 32 bytes of the message digest, or the shorter digest left-padded
 *                with zeros (crypto/ecdsa hashToNat)
 *       Qx, Qy : affine public key
 *   - accept bitmap: ceil(n/8) bytes, bit (i & 7) of byte (i >> 3) = tuple i (LSB first),
 *     1 = crypto/ecdsa.VerifyASN1 would return true.
 *   - there is NO CPU fallback inside the library: without a usable gfx950 device every
 *     compute entry point returns SBV_ENODEV.
 *   - all functions are thread-safe.  There is one context per DEVICE (sbv_init(d) creates device d's; the first one
 *     initialised is the default the single-device entry points use; sbv_init_all() creates one per visible gfx950 device and
 *     the sharded / _on entries address them); device work is serialised per context.  The tuning setters
 *     (sbv_p256_set_grouping, sbv_p256_key_cache, sbv_profile_enable, sbv_shard_mode) are process-wide: they apply to every
 *     initialised device and to devices initialised later, also when called before sbv_init.
 */
#ifndef SBV_H_
#define SBV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBV_OK 0
#define SBV_ENODEV (-1)    /* no HIP device / not a gfx950 / runtime failure at init */
#define SBV_EINVAL (-2)    /* bad argument */
#define SBV_ENOMEM (-3)    /* device or pinned-host allocation failed */
#define SBV_EDEVICE (-4)   /* a HIP call failed during the batch (see sbv_last_error) */
#define SBV_ENOTINIT (-5)  /* sbv_init has not succeeded */
#define SBV_EPARSE (-6)    /* sbv_p256_parse_der: not a strict DER ECDSA-Sig-Value */

#define SBV_P256_TUPLE_BYTES 160

/* Initialise the context on HIP device `device` (>= 0): uploads the fixed-base table and
 * sizes scratch lazily.  Must be called once before Consensus.Start()
 * (pkg/consensus/consensus.go:107; the Verifier is injected at :35). Idempotent. */
int sbv_init(int device);
int sbv_shutdown(void);
/* Number of visible HIP devices (<0 on runtime failure). */
int sbv_device_count(void);

/* Verify n tuples in host memory; blocks until the bitmap is written.
 * Takes over: the K request signatures of VerifyProposal (internal/bft/view.go:555), the
 * coalesced VerifyConsenterSig calls of processCommits (view.go:537-541, 834-838) and
 * verifyPrevCommitSignatures (view.go:630-635), VerifyRequest (controller.go:239) under
 * Pool.Prune (controller.go:742-745), ValidateLastDecision / VerifySignature
 * (viewchanger.go:598, 660, 718, 983, 1022, 1076). */
int sbv_p256_verify_batch(const uint8_t* tuples, size_t n, uint8_t* accept_bitmap);

/* In-step key grouping for the generic entry points (consensus_amd/csrc/p256_group.h): tuples are grouped by public key on
 * the device; keys used by at least `min_count` tuples of THIS batch — or already held by the key-table cache below, however
 * few of their signatures the batch carries — (at most `max_groups` of them) get / reuse a comb table and their signatures
 * take the no-doubling kernels; everything else takes the generic kernel inside the same step.  Verdicts are identical.
 * `min_batch` = batches from this size on take the grouped step.  Defaults: enabled; min_batch 64 while the key-table cache is
 * on (a warm batch of a few thousand tuples skips the 256 doublings per signature), 2^17 while it is off (nothing outlives the
 * call then, and below ~2^17 building tables costs more latency than the doubling kernel takes); min_count 8 for P-256 (counted
 * exactly; the Ed25519 / secp256k1 steps, whose tables are always full, keep 64 and at most
 * 2048 groups); max_groups 65536 (round 5; 2048 before — a 2^20 batch over 4096 keys sent half its tuples to the one-lane kernel).
 * Passing a non-zero min_batch sets both thresholds (and the variant schemes'); SBV_GROUP_MIN_BATCH_DEFAULT restores the built-in
 * ones together with the built-in min_count and max_groups (a non-zero min_count / max_groups in the same call still applies);
 * 0 for a numeric argument keeps its current value.  Env: SBV_GROUP=0
 * disables, SBV_GROUP_MIN_BATCH=<n>.  What IS remembered between calls is the key-table cache. */
#define SBV_GROUP_MIN_BATCH_DEFAULT ((size_t)-1)
int sbv_p256_set_grouping(int enabled, size_t min_batch, uint32_t min_count, uint32_t max_groups);

/* Persistent key-table cache.  The comb a grouped batch builds for a key is a pure function of the key's 64 bytes, and
 * SmartBFT's signer sets are stable for whole epochs (pkg/types/types.go:25-29; reconfiguration:
 * pkg/consensus/consensus.go:185-252), so the tables are kept in HBM (270 KiB per key) and later batches only build the
 * tables of keys they have not met: a "warm" batch skips the doubling chains and the table kernels altogether.  Verdicts
 * cannot depend on it (a slot is found by comparing all 64 key bytes and holds exactly what the batch would have built).
 * enabled: default 1; switching it off also empties it.  capacity: keys kept (default 16384; 0 = unchanged); when full,
 * further keys are simply rebuilt per batch.  stats: out[0] = cached keys, out[1] / out[2] = groups of the last grouped
 * batch that hit / missed, out[3] = capacity.  bench.py measures its headline with the cache OFF (every step cold). */
int sbv_p256_key_cache(int enabled, uint32_t capacity);
int sbv_p256_key_cache_stats(uint32_t out[4]);
/* The same cache for every signature scheme of the library (round 4).  Consenter and client traffic on the secp256k1 and
 * Ed25519 variants is the same handful of keys forever (internal/bft/view.go:631, 834), so their grouped steps keep their
 * per-key combs too — each scheme in a pool of its OWN: a slot is found by the key bytes, and the same 64 bytes can be a
 * point of both ECDSA curves (a shared table would let a crafted key be verified against the other curve's comb).
 * scheme = SBV_SCHEME_*; defaults: on, 16384 (P-256) / 1024 (secp256k1: 270 KiB per key) / 1024 (Ed25519: 384 KiB per key)
 * keys.  With a scheme's cache on, its batches take the grouped step from 64 tuples (sbv_p256_set_grouping's min_batch).
 * sbv_p256_key_cache(e, c) == sbv_key_cache(SBV_SCHEME_P256, e, c). */
#define SBV_SCHEME_P256 0
#define SBV_SCHEME_SECP256K1 1
#define SBV_SCHEME_ED25519 2
int sbv_key_cache(int scheme, int enabled, uint32_t capacity);
int sbv_key_cache_stats(int scheme, uint32_t out[4]);

/* Same, on device-resident buffers, asynchronous on `hip_stream` (a hipStream_t; NULL = the
 * default stream).  d_tuples: n*160 bytes, 16-byte aligned.  d_bitmap: ceil(n/8) bytes.
 * The caller synchronises the stream.  Used by bench.py / multi-GPU shards.
 * The stream contract of this and every other `_dev` / `_dev_part` entry (tests/test_gpu_stream_order.py):
 *   - work queued on `hip_stream` BEFORE the call is seen: a kernel or copy that produces the inputs there needs no synchronisation
 *     in front of the call, although the library reads them on streams of its own as well;
 *   - work queued on `hip_stream` AFTER the call sees the complete output and may overwrite the inputs at once: every reader the
 *     library started on another stream is joined back into `hip_stream` inside the call;
 *   - any OTHER stream of the caller's that produces the inputs or consumes the output needs an event of the caller's between it
 *     and `hip_stream`, as for any other stream-ordered work;
 *   - the buffers must stay allocated until `hip_stream` has passed the call (the library keeps no reference beyond that point; a
 *     hipFree in front of it is the caller's error);
 *   - calls from different streams and from different host threads, of any scheme, host-pointer entries and setters included, are
 *     ordered against each other by the library: it shares scratch, grouping arrays and table pools between them and asks no
 *     event of the caller for that.  A call that has to grow a buffer, and every setter that frees or rewrites device state,
 *     waits on the host for the calls queued before it; an entry that says so (`_dev_part`) waits for its own stream once. */
int sbv_p256_verify_batch_dev(const void* d_tuples, size_t n, void* d_bitmap, void* hip_stream);

/* ---- registered public keys ---------------------------------------------------------------------
 * SmartBFT's consenter set (and an application's client set) is a registry: types.Signature.ID
 * selects the key (pkg/types/types.go:25-29), it is not carried per signature.  Registering a key
 * builds a fixed-base comb for it (33 x 128 affine multiples, 270 KiB of HBM per key) once, after
 * which a verification against that key needs NO point doublings: R = u1*G + u2*Q is 13 + 32.2 = 45.2 mixed
 * additions on average (13 from the 20-bit comb of G, 32 key-comb windows + the rarely needed carry window; ~5x fewer field
 * multiplications than the generic form).  Batches of at most 32 signatures take a one-launch latency form (stage A of the
 * call on the calling CPU thread with one inversion, records and verdicts in mapped host memory, 16 lanes per signature), up to 32768 the 8-lanes-per-signature kernel.  Verdicts are identical to
 * the generic entry points: a key that crypto/ecdsa would refuse (coordinate >= p, off curve) still
 * gets a slot, flagged invalid, and every signature against it is rejected.
 *   keys: m x 64 bytes (Qx|Qy big-endian).  slots_out[i] = slot of keys[i] (equal keys share a slot). */
int sbv_p256_register_keys(const uint8_t* keys, size_t m, uint32_t* slots_out);
int sbv_p256_key_count(void);
int sbv_p256_clear_keys(void);
/* Wide combs for the consenters' keys (round 4).  The consenters of a cluster are a handful of keys that sign every vote of every
 * decision for a whole epoch (pkg/types/types.go:25-29; internal/bft/view.go:531-541 collects 2f+1 of their commit signatures per
 * decision, view.go:631 and :834 verify them; reconfiguration replaces the set: pkg/consensus/consensus.go:185-252), and HBM holds
 * 288 GB: sbv_p256_widen_keys gives the named registered slots a second, `bits`-wide comb (the layout of the comb of G), after
 * which u2*Q is ceil(257 / bits) additions instead of 32.2 — 16 bits: 16 additions, 35.7 MB per key; 20 bits: 13 additions,
 * 436 MB per key.  A wavefront whose signatures all belong to wide slots takes the wide
 * combs, any other the 8-bit combs every key keeps; verdicts are identical.  Slots that are wide already are skipped, slots
 * beyond `max_keys` wide ones stay narrow (no error); an unregistered slot is SBV_EINVAL.  On a device fault the call returns
 * SBV_EDEVICE / SBV_ENOMEM and leaves the registry as it was: the named slots keep their 8-bit combs and may be named again.
 * sbv_p256_wide_keys sets the width and the cap for every device.  Default: bits = SBV_WIDE_BITS_AUTO, 64 keys — 20-bit combs
 * while at most 16 slots are wide (a 16-node cluster: 7 GB), 16-bit combs beyond (64 keys: 2.3 GB); crossing the line rebuilds
 * what was there, on the device, in milliseconds.  An explicit width (10..20) is kept whatever the count; bits = 0 switches the
 * feature off and frees the tables; another width rebuilds the combs of the slots already widened.  Env: SBV_KEYED_WIDE_BITS
 * (0 = off, 1 = auto), SBV_KEYED_WIDE_MAX.  stats: out[0] = wide slots, out[1] = bits, out[2] = max_keys, out[3] = KiB per key. */
#define SBV_WIDE_BITS_AUTO 1
int sbv_p256_wide_keys(int bits, uint32_t max_keys);
int sbv_p256_widen_keys(const uint32_t* slots, size_t m);
int sbv_p256_wide_key_stats(uint32_t out[4]);
/* The combs are built on the device (consensus_amd/csrc/p256_widetab29.h: two launches for all the keys of a call: 0.01 s for 16
 * keys at 16 bits, 0.03 s at 20 bits, measured); SBV_KEYED_WIDE_HOST=1 selects the host builder.  Diagnostics: sbv_p256_wide_selfcheck(slot) = 1 when the
 * device-resident comb of `slot` equals the host builder's output byte for byte, 0 when it differs. */
int sbv_p256_wide_selfcheck(uint32_t slot);
/* rsh: n x 96 bytes (r|s|hash, big-endian), slots: n key slots.  Takes over VerifyConsenterSig
 * (view.go:631, 834), VerifySignature (viewchanger.go:598...) and decision replay for registered
 * signers.  An out-of-range slot is a reject, not an error. */
int sbv_p256_verify_batch_keyed(const uint8_t* rsh, const uint32_t* slots, size_t n, uint8_t* accept_bitmap);
int sbv_p256_verify_batch_keyed_dev(const void* d_rsh, const void* d_slots, size_t n, void* d_bitmap, void* hip_stream);

/* Batch signing: the batch form of api.Signer.Sign / SignProposal (pkg/api/dependencies.go:46-52;
 * examples and tests sign with crypto/ecdsa over SHA-256).  Signature i = ECDSA-P256(key[key_index[i]], digests[i]) with the
 * deterministic nonce of RFC 6979 (HMAC-SHA256), bit-identical to consensus_amd/host's Signer; key_index == NULL means key
 * i % n_keys.  keys: n_keys x 32 bytes (private scalar, big-endian); digests: n x 32 bytes (SHA-256 of the message);
 * sigs: n x 64 bytes r | s (big-endian; DER-encode for types.Signature.Value); ok[i] = 0 when key i is not in [1, N-1] or the
 * index is out of range (sigs[i] is then all zero).  NOT constant-time (secret-indexed table lookups in HBM): for test
 * traffic and trusted single-tenant hosts, see consensus_amd/csrc/p256_sign.h.
 * SBV_ENOTINIT before sbv_init, for both entries and whatever the arguments.  n == 0 is SBV_OK and writes nothing.  Otherwise
 * SBV_EINVAL, with nothing written: a null keys, digests, sigs or ok, n_keys == 0, and for the `_dev` entry a d_keys, d_key_index,
 * d_digests or d_sigs that is not 4-byte aligned (the kernel reads and writes them as 32-bit words); d_ok is a byte array and may
 * sit at any address.  A refused call leaves the library as it was: the next good call signs.
 * sbv_p256_sign_batch takes host pointers, uses device buffers of the call's own size, waits for the result and zeroes the device
 * copy of the keys before it frees it.  That holds for every host-pointer form below that takes or makes secrets (the signers,
 * sbv_secp256k1_pubkeys, both expand_keys entries and the sign / Schnorr debug entries): the device copies of private keys, seeds and
 * expanded records are zeroed before they are released, on success and on failure alike.  The zeroing is itself device work whose
 * result no call reports: if the fill or the wait for it fails, as on a faulted device, the buffers are still released, unzeroed.
 * sbv_p256_sign_batch_dev takes device pointers, launches on `hip_stream` and returns without synchronising, under the stream
 * contract of the `_dev` entries above; it may be the first call of a process after sbv_init.  Both are
 * held byte for byte to an independent RFC 6979 signer, the retry of section 3.2 h (a first candidate >= N: 2^-32 per signature)
 * included, in tests/test_emul_sign.py and tests/test_gpu_sign.py. */
int sbv_p256_sign_batch(const uint8_t* keys, uint32_t n_keys, const uint32_t* key_index, const uint8_t* digests, size_t n,
                        uint8_t* sigs, uint8_t* ok);
int sbv_p256_sign_batch_dev(const void* d_keys, uint32_t n_keys, const void* d_key_index, const void* d_digests, size_t n,
                            void* d_sigs, void* d_ok, void* hip_stream);

/* secp256k1 batch signing: the batch form of api.Signer.Sign for the secp256k1 variant.  Signature i = ECDSA-secp256k1(
 * key[key_index[i]], digests[i]) with the deterministic nonce of RFC 6979 (HMAC-SHA256); with flags = 0 bit-identical to
 * consensus_amd/host's Signer (k256_sign_rfc6979).  The rules are sbv_p256_sign_batch's: keys: n_keys x 32 bytes (private scalar,
 * big-endian); digests: n x 32 bytes; sigs: n x 64 bytes r | s (big-endian); key_index == NULL means key i % n_keys; ok[i] = 0 with
 * 64 zero bytes in sigs[i] and recid[i] = 0 when the key is not in [1, n-1] or the index is >= n_keys.  n == 0 is SBV_OK and writes
 * nothing.  Beyond the P-256 entry:
 *   flags   SBV_K256_SIGN_LOW_S: s > (n-1)/2 is replaced by n - s, the form Bitcoin- and Ethereum-shaped verifiers require (the
 *           verifier of this library has no low-S rule and accepts both forms).  Any other bit is SBV_EINVAL.
 *   recid   n bytes, or NULL when not wanted: the recovery id 0..3 of signature i.  Bit 0 = parity of the y of R = k G (flipped when
 *           low-S negated s), bit 1 = R.x >= n (probability ~2^-128).  Q = r^-1 (s R' - e G) for the point R' with x = r
 *           (+ n when bit 1 is set) and y of parity bit 0.
 * SBV_EINVAL: a null required pointer, n_keys == 0, an unknown flag bit, and for the `_stream` forms a device pointer (keys, key
 * index, digests, sigs, pubs) that is not 4-byte aligned; SBV_ENOTINIT before sbv_init.
 *   sbv_secp256k1_pubkeys   keys: m x 32 bytes -> pubs: m x 64 bytes Qx | Qy of d G, ok[i] = 0 with 64 zero bytes for d outside [1, n-1].
 * The host-pointer forms use device buffers of the call's own size, wait for the result and zero the device copy of the keys before
 * they free it.  The `_stream` forms take device pointers, launch on `hip_stream` and return without synchronising, under the stream
 * contract of the `_dev` entries above for every buffer they name.  They own no mutable device state: two
 * calls on two streams share nothing but the read-only 16-bit comb of G, uploaded (synchronously) by the first secp256k1 call of
 * the process, which may be one of these.  They are named `_stream` and not `_dev` for the reason the Ed25519 entries are; their
 * schedules (late producer, early overwriter, X-Y-X) are in tests/test_gpu_k256_sign.py.
 * NOT constant-time (secret-indexed table lookups in HBM, variable-time inversions): for test traffic and trusted single-tenant
 * hosts, see consensus_amd/csrc/k256_sign.h.
 * (The return types stand on lines of their own, as for the hot-key entries below: the registered-key entries are counted by their
 * one-line form.) */
#define SBV_K256_SIGN_LOW_S 1u
int
sbv_secp256k1_sign_batch(const uint8_t* keys, uint32_t n_keys, const uint32_t* key_index, const uint8_t* digests, size_t n,
                         uint32_t flags, uint8_t* sigs, uint8_t* recid, uint8_t* ok);
int
sbv_secp256k1_sign_batch_stream(const void* d_keys, uint32_t n_keys, const void* d_key_index, const void* d_digests, size_t n,
                                uint32_t flags, void* d_sigs, void* d_recid, void* d_ok, void* hip_stream);
int
sbv_secp256k1_pubkeys(const uint8_t* keys, size_t m, uint8_t* pubs, uint8_t* ok);
int
sbv_secp256k1_pubkeys_stream(const void* d_keys, size_t m, void* d_pubs, void* d_ok, void* hip_stream);
/* Test only: one case of a unit operation of the signer per lane on the device, host pointers.  Every case reads one 192-byte record
 * of six fields and writes one 128-byte record of four fields; a field is a 32-byte big-endian integer, unused fields are ignored
 * on input and zero on output, and output field 3 is the operation's ok (0 or 1; a case that is not ok is all zero).
 *   op 0   in: d | digest                        out: k | K | V   the first RFC 6979 candidate and the DRBG state behind it (V = k);
 *                                                                 ok = 0 for d outside [1, n-1]
 *   op 1   in: K | V                             out: K' | V' | k'   the section 3.2 h update after a rejected candidate V:
 *                                                                 K' = HMAC(K, V || 00), V' = HMAC(K', V), k' = HMAC(K', V')
 *   op 2   in: k                                 out: x | y of k G, affine; ok = 0 for k outside [1, n-1]
 *   op 3   in: x | y_odd | d | k | e | flags     out: r | s | recid   k256_sign_finish on plain integers: x any 256-bit value, d and
 *                                                                 e < n, k in [1, n-1]; ok = 0 when r = 0 or s = 0
 * Any other op is SBV_EINVAL. */
int sbv_debug_secp256k1_sign_op(int op, const uint8_t* in, uint8_t* out, size_t n);

/* secp256k1 batch public-key recovery: the consumer of the recovery id above.  Traffic shaped like Ethereum's carries no public key
 * but 65 bytes r | s | v; this returns the signer's key Q of every (r, s, recid, digest), ready for the verify entries or for
 * sbv_secp256k1_register_keys.  sigs: n x 64 bytes r | s (big-endian), recid: n bytes, digests: n x 32 bytes — exactly the arrays
 * sbv_secp256k1_sign_batch emits — pubs: n x 64 bytes Qx | Qy, ok: n bytes.  The rules are those of libsecp256k1's ecdsa_recover;
 * item i fails, with ok[i] = 0 and 64 zero bytes in pubs[i], unless all of these hold:
 *   - r and s are in [1, n-1];
 *   - recid is in 0..3;
 *   - x = r + (recid & 2 ? n : 0) is below p (only r < p - n can take the + n branch);
 *   - y^2 = x^3 + 7 has a root; y is the root whose canonical parity is recid & 1, R' = (x, y);
 *   - with e = the digest reduced mod n as the verifier reduces it, u1 = (n - e) r^-1 mod n (0 for e = 0) and u2 = s r^-1 mod n,
 *     Q = u2 R' + u1 G is not the point at infinity.
 * Then ok[i] = 1 and pubs[i] = the affine, canonical Qx | Qy, and the verify entries accept (r, s, digest, Q).
 *   flags   SBV_K256_RECOVER_LOW_S: also refuses s > (n-1)/2, as Bitcoin- and Ethereum-shaped verifiers do.  Any other bit is SBV_EINVAL.
 * A lane needs a table strip in device memory, so the kernel runs at most SBV_K256_RECOVER_LANES lanes, each over items L, L + LANES,
 * ...: sbv_secp256k1_recover_workspace(n) = min(n, SBV_K256_RECOVER_LANES) strips of 1536 bytes is all the workspace any n needs.
 * sbv_secp256k1_recover takes host pointers, uses device buffers and a workspace of the call's own size, waits for the result and
 * frees them.  sbv_secp256k1_recover_stream takes device pointers and the caller's workspace (d_work, work_bytes >=
 * sbv_secp256k1_recover_workspace(n)), launches on `hip_stream` and returns without synchronising, under the stream contract of the
 * `_dev` entries for every buffer it names, the workspace included: two calls that may overlap need two
 * workspaces.  It owns no mutable device state and shares only the read-only 16-bit comb of G, uploaded (synchronously) by the first
 * secp256k1 call of the process, which may be this one.  It is named `_stream` for the reason the signer's entries are; its
 * schedules are in tests/test_gpu_k256_recover.py.
 * SBV_EINVAL: a null required pointer, an unknown flag bit, and for the `_stream` form a device pointer (sigs, digests, pubs) that
 * is not 4-byte aligned, a d_work that is not 16-byte aligned or work_bytes too small; SBV_ENOTINIT before sbv_init.  n == 0 is
 * SBV_OK and writes nothing.  Nothing here is secret, so variable time is no concern. */
#define SBV_K256_RECOVER_LOW_S 1u
#ifndef SBV_K256_RECOVER_LANES
#define SBV_K256_RECOVER_LANES 131072 /* one full residency of an MI355X: 256 CUs x 4 SIMDs x 2 waves x 64 lanes */
#endif
int
sbv_secp256k1_recover(const uint8_t* sigs, const uint8_t* recid, const uint8_t* digests, size_t n, uint32_t flags, uint8_t* pubs,
                      uint8_t* ok);
size_t
sbv_secp256k1_recover_workspace(size_t n);
int
sbv_secp256k1_recover_stream(const void* d_sigs, const void* d_recid, const void* d_digests, size_t n, uint32_t flags, void* d_pubs,
                             void* d_ok, void* d_work, size_t work_bytes, void* hip_stream);
/* Test only: one case of a unit operation of the recovery per lane on the device, host pointers, in the records of
 * sbv_debug_secp256k1_sign_op (192 bytes in, 128 bytes out, output field 3 = ok, a case that is not ok is all zero).
 *   op 0   in: a                  out: a^((p+1)/4)   the square root; ok = a is a square mod p (a is any 256-bit value)
 *   op 1   in: r | recid          out: x | y         the lifted point R'; ok = 0 when recid > 3, x >= p or x^3 + 7 is no square
 *   op 2   in: x | y | u1 | u2    out: Qx | Qy       u2 (x, y) + u1 G for a point of the curve and u1, u2 < n; ok = 0: infinity
 * Any other op is SBV_EINVAL. */
int sbv_debug_secp256k1_recover_op(int op, const uint8_t* in, uint8_t* out, size_t n);

/* Keccak-256 and Ethereum-style addresses: the two hashes at either end of a recovery.  Keccak-256 is the original Keccak at rate 136
 * with the padding byte 0x01 (what Ethereum calls keccak256), NOT FIPS 202's SHA3-256, which differs in that one byte.
 *   sbv_keccak256_msgs                msgs: all messages back to back, msg_offsets: n + 1 offsets, message i is
 *                                     msgs[msg_offsets[i] .. msg_offsets[i+1]); digests: n x 32 bytes.  The offset table follows the rule
 *                                     of sbv_ed25519_sign_msgs: it starts at 0 and never decreases, otherwise SBV_EINVAL; msgs may be
 *                                     NULL when every message is empty.  The digests are exactly the `digests` array that
 *                                     sbv_secp256k1_sign_batch and sbv_secp256k1_recover take.
 *   sbv_secp256k1_addresses           pubs: m x 64 bytes Qx | Qy (big-endian, as sbv_secp256k1_pubkeys and sbv_secp256k1_recover emit);
 *                                     addrs: m x 20 bytes, Keccak-256(Qx | Qy)[12..31].  A pure hash: the key is not checked against
 *                                     the curve, and 64 zero bytes have an address like any other input.
 *   sbv_secp256k1_recover_addresses   sbv_secp256k1_recover with the address in place of the key: what Ethereum's ecrecover returns.
 *                                     Arrays, rules, flags and workspace (sbv_secp256k1_recover_workspace(n), 16-byte aligned) are
 *                                     exactly that entry's; addrs: n x 20 bytes, ok: n bytes.  For every item ok[i] is that entry's
 *                                     ok[i]; addrs[i] is the address of that entry's key when ok[i] = 1 and 20 zero bytes when
 *                                     ok[i] = 0.  The stride of addrs is 20 bytes and byte 20 n is not written.
 * EIP-155 `v` values, EIP-191 prefixes and EIP-55 checksums are the caller's formatting.
 * The host-pointer forms use device buffers of the call's own size, wait for the result and free them.  The `_stream` forms take device
 * pointers, launch on `hip_stream` and return without synchronising, under the stream contract of the `_dev` entries (DESIGN.md
 * section 4.2.4) for every buffer they name, the workspace included.  The two hash entries own no state and upload nothing;
 * sbv_secp256k1_recover_addresses_stream shares only the read-only 16-bit comb of G, uploaded (synchronously) by the first secp256k1
 * call of the process, which may be this one.  In sbv_keccak256_msgs_stream nothing on the host sees the offsets: an item whose offset
 * pair decreases gets 32 zero bytes and nothing of the messages is read for it; d_msgs may be NULL when every message is empty.
 * They are named `_stream` for the reason the signer's entries are; their schedules are in tests/test_gpu_keccak.py.
 * SBV_EINVAL: a null required pointer, an unknown flag bit, a bad offset table (host-pointer form), and for the `_stream` forms a
 * device pointer to digests, keys, signatures or addresses that is not 4-byte aligned, a d_msg_offsets that is not 8-byte aligned, a
 * d_work that is not 16-byte aligned or work_bytes too small; d_msgs may have any alignment.  SBV_ENOTINIT before sbv_init.  n == 0
 * (m == 0) is SBV_OK and writes nothing.  Nothing here is secret. */
int
sbv_keccak256_msgs(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, uint8_t* digests);
int
sbv_keccak256_msgs_stream(const void* d_msgs, const void* d_msg_offsets, size_t n, void* d_digests, void* hip_stream);
int
sbv_secp256k1_addresses(const uint8_t* pubs, size_t m, uint8_t* addrs);
int
sbv_secp256k1_addresses_stream(const void* d_pubs, size_t m, void* d_addrs, void* hip_stream);
int
sbv_secp256k1_recover_addresses(const uint8_t* sigs, const uint8_t* recid, const uint8_t* digests, size_t n, uint32_t flags, uint8_t* addrs,
                                uint8_t* ok);
int
sbv_secp256k1_recover_addresses_stream(const void* d_sigs, const void* d_recid, const void* d_digests, size_t n, uint32_t flags,
                                       void* d_addrs, void* d_ok, void* d_work, size_t work_bytes, void* hip_stream);
/* Test only: one case of a unit operation of Keccak per lane on the device, host pointers.
 *   op 0   in: 200 bytes, the 25 lanes of a state A[x + 5 y], each little-endian   out: 200 bytes, the state after one Keccak-f[1600]
 * Any other op is SBV_EINVAL. */
int sbv_debug_keccak_op(int op, const uint8_t* in, uint8_t* out, size_t n);

/* BIP-340 Schnorr signatures over secp256k1 (Bitcoin's since Taproot): batch verification, key expansion and batch signing.  Keys are
 * x-only (32 bytes: the x of the point with even y), messages are 32 bytes, signatures are 64 bytes R.x | s, all big-endian; `ok`
 * is one byte per item (0 or 1), as in the sign, pubkeys and recover family, not a bitmap.
 *
 * Verification follows BIP-340 "Verify" exactly.  pks: n x 32, msgs: n x 32, sigs: n x 64, ok: n bytes.  ok[i] = 1 iff all hold:
 *   - pk < p and pk^3 + 7 is a square mod p; P = lift_x(pk) is the point with that x and even y;
 *   - r < p and s < n (s = 0 is in range);
 *   - with e = int(SHA256 tagged "BIP0340/challenge" of r | pk | msg) mod n, R = s G - e P is not the point at infinity, has even y
 *     and x = r.
 * A lane needs a table strip in device memory, exactly as recovery does: at most SBV_K256_RECOVER_LANES lanes run, each over items L,
 * L + LANES, ..., and sbv_secp256k1_schnorr_verify_workspace(n) = min(n, SBV_K256_RECOVER_LANES) strips of 1536 bytes serves any n.
 * sbv_secp256k1_schnorr_verify takes host pointers, uses device buffers and a workspace of the call's own size, waits and frees
 * them.  sbv_secp256k1_schnorr_verify_stream takes device pointers and the caller's workspace (d_work, work_bytes >= the size above),
 * launches on `hip_stream` and returns without synchronising, under the stream contract of the `_dev` entries (DESIGN.md section
 * 4.2.4) for every buffer it names, the workspace included: two calls that may overlap need two workspaces.
 *
 * Signing is BIP-340 "Default Signing" without its optional final self-verification, in two steps so that the base multiplication
 * for the key is paid once and not once per signature (as for sbv_ed25519_expand_keys; libsecp256k1 calls the record a keypair).
 *   sbv_secp256k1_schnorr_expand_keys   keys: m x 32 bytes (d', big-endian).  expanded: m x 64 bytes, one RECORD per key:
 *                                           bytes  0..31  d     d' when P = d' G has even y, else n - d'
 *                                           bytes 32..63  P.x   the x-only public key
 *                                       pks: m x 32 bytes P.x, or NULL when not wanted.  ok[i] = 0 with an all-zero record (and
 *                                       key) for d' outside [1, n-1].
 *   sbv_secp256k1_schnorr_sign          expanded: n_keys records; key_index: n x u32, or NULL meaning key i % n_keys; msgs: n x 32;
 *                                       aux: n x 32 bytes of auxiliary randomness, or NULL meaning 32 zero bytes for every item
 *                                       (what libsecp256k1 does without auxiliary data); sigs: n x 64; ok: n bytes.  ok[i] = 0 with
 *                                       64 zero bytes when the index is >= n_keys, the record's d is outside [1, n-1] (the record
 *                                       of a refused key) or the nonce is 0 (probability ~2^-256).
 * A RECORD IS AS SECRET AS ITS KEY.  Records must come from sbv_secp256k1_schnorr_expand_keys: the signer does not check that P.x
 * belongs to d, and a record whose P.x does not yields signatures that can leak d.
 * The host-pointer forms use device buffers of the call's own size, wait for the result and zero the device copies of keys and
 * records before they free them.  The `_stream` forms take device pointers, launch on `hip_stream` and return without synchronising,
 * under the same stream contract.  None of the `_stream` forms owns mutable device state: they share only the read-only 16-bit comb
 * of G, uploaded (synchronously) by the first secp256k1 call of the process, which may be any of them.  They are named `_stream` for
 * the reason the ECDSA signer's entries are; their schedules are in tests/test_gpu_k256_schnorr.py.
 * SBV_EINVAL: a null required pointer, n_keys == 0, and for the `_stream` forms a device pointer to data that is not 4-byte aligned,
 * a d_work that is not 16-byte aligned or work_bytes too small; SBV_ENOTINIT before sbv_init.  n == 0 (m == 0) is SBV_OK and writes
 * nothing.
 * Expansion and signing are NOT constant-time (secret-indexed table lookups in HBM, a variable-time inversion): for test traffic and
 * trusted single-tenant hosts, see consensus_amd/csrc/k256_schnorr.h.  Verification handles nothing secret. */
int
sbv_secp256k1_schnorr_verify(const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs, size_t n, uint8_t* ok);
size_t
sbv_secp256k1_schnorr_verify_workspace(size_t n);
int
sbv_secp256k1_schnorr_verify_stream(const void* d_pks, const void* d_msgs, const void* d_sigs, size_t n, void* d_ok, void* d_work,
                                    size_t work_bytes, void* hip_stream);
int
sbv_secp256k1_schnorr_expand_keys(const uint8_t* keys, size_t m, uint8_t* expanded, uint8_t* pks, uint8_t* ok);
int
sbv_secp256k1_schnorr_expand_keys_stream(const void* d_keys, size_t m, void* d_expanded, void* d_pks, void* d_ok, void* hip_stream);
int
sbv_secp256k1_schnorr_sign(const uint8_t* expanded, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs, const uint8_t* aux,
                           size_t n, uint8_t* sigs, uint8_t* ok);
int
sbv_secp256k1_schnorr_sign_stream(const void* d_expanded, uint32_t n_keys, const void* d_key_index, const void* d_msgs, const void* d_aux,
                                  size_t n, void* d_sigs, void* d_ok, void* hip_stream);
/* Test only: one case of a unit operation of the Schnorr lanes per lane on the device, host pointers, in the records of
 * sbv_debug_secp256k1_sign_op (192 bytes in, 128 bytes out, output field 3 = ok).
 *   op 0   in: a | b | c, selector   out: the tagged hash     selector = the last 4 bytes of field 5: 0 "BIP0340/aux" of a alone,
 *                                                             1 "BIP0340/nonce", 2 "BIP0340/challenge" of a | b | c; ok = 1
 *   op 1   in: x                     out: y                   lift_x: the even root of x^3 + 7; ok = 0 (all zero) for x >= p or no root
 *   op 2   in: X | Y | Z | r         out: x | y               the affine form of a Jacobian point (coordinates below p; Z = 0 is
 *                                                             infinity: all zero); ok = the verdict of the final check of "Verify":
 *                                                             not infinity, x = r, y even
 *   op 3   in: d | Px | k' | m       out: R.x | s             the signing equation on plain integers (d < n): R = k' G, k = k' or
 *                                                             n - k' by the parity of R.y, s = k + e d; ok = 0 (all zero) for k'
 *                                                             outside [1, n-1]
 * Any other op is SBV_EINVAL.  The double-scalar walk is op 2 of sbv_debug_secp256k1_recover_op. */
int
sbv_debug_secp256k1_schnorr_op(int op, const uint8_t* in, uint8_t* out, size_t n);

/* BIP-340 Schnorr verification against REGISTERED secp256k1 keys: the fixed key set of a consenter group, verified from the combs the
 * registry of sbv_secp256k1_register_keys holds in device memory.  There is no second registry: a slot is a slot of that registry, one
 * slot serves the ECDSA keyed entries and this one, and sbv_secp256k1_wide_keys / sbv_secp256k1_widen_keys / sbv_secp256k1_clear_keys
 * work unchanged.
 *   sbv_secp256k1_schnorr_lift_keys      pks: m x 32 bytes (x-only).  keys64: m x 64 bytes x | y of lift_x(pk), the point with that x
 *                                        and even y — the bytes sbv_secp256k1_register_keys takes.  ok: m bytes, or NULL when not
 *                                        wanted.  For pk >= p or pk^3 + 7 no square: ok[i] = 0 and keys64 = pk | 32 zero bytes.  No
 *                                        curve point has y = 0, so registering such an output gives an INVALID slot, and every
 *                                        signature against it is rejected: the verdict of sbv_secp256k1_schnorr_verify for that key.
 *                                        Registration of an x-only key is lift_keys followed by register_keys.
 *   sbv_secp256k1_schnorr_verify_keyed   msgs: n x 32, sigs: n x 64 (R.x | s), slots: n x u32, ok: n bytes (0 or 1, not a bitmap).
 *                                        ok[i] is byte for byte what sbv_secp256k1_schnorr_verify answers for the same message and
 *                                        signature with pk = the first 32 bytes (Qx) of the slot's key as registered.  The registered
 *                                        Qy may have either parity (a key registered for ECDSA serves as it is): BIP-340's key is the
 *                                        point with even y, P = Q or -Q, and R = s G - e P is walked as s G + u2 Q with u2 = n - e for
 *                                        an even Qy and u2 = e for an odd one.  An out-of-range slot, an invalid slot, r >= p, s >= n
 *                                        and R at infinity are rejects, not errors.  With no registered key every item is a reject.
 * Per item: two SHA-256 compressions, the comb of G, the slot's comb (8-bit, or 16-bit when every live lane of the wavefront owns
 * one, the rule of sbv_secp256k1_verify_batch_keyed) and one field inversion; no square root, no doubling, no workspace, no cap on
 * the grid.  n (m) <= 2^32 per call; there is no 2^21 chunking because no scratch plane of the context is used.
 * The host-pointer forms use device buffers of the call's own size, wait for the result and free them.  The `_stream` forms take
 * device pointers, launch on `hip_stream` and return without synchronising, under the stream contract of the `_dev` entries
 *  for every buffer they name.  They write no state of the library: the registry's tables and the comb of G
 * are read-only, and a registration or widening that replaces the registry's arrays synchronises the device before it frees the old
 * ones, so a queued call stays valid, as for sbv_secp256k1_verify_batch_keyed_dev.  The first secp256k1 call of the process uploads
 * the comb of G synchronously, and it may be one of these.  Their schedules are in tests/test_gpu_k256_schnorr_keyed.py.
 * SBV_EINVAL: a null required pointer, n > 2^32, and for the `_stream` forms a device pointer to data that is not 4-byte aligned;
 * SBV_ENOTINIT before sbv_init.  n == 0 (m == 0) is SBV_OK and writes nothing.  Nothing here is secret. */
int
sbv_secp256k1_schnorr_lift_keys(const uint8_t* pks, size_t m, uint8_t* keys64, uint8_t* ok);
int
sbv_secp256k1_schnorr_lift_keys_stream(const void* d_pks, size_t m, void* d_keys64, void* d_ok, void* hip_stream);
int
sbv_secp256k1_schnorr_verify_keyed(const uint8_t* msgs, const uint8_t* sigs, const uint32_t* slots, size_t n, uint8_t* ok);
int
sbv_secp256k1_schnorr_verify_keyed_stream(const void* d_msgs, const void* d_sigs, const void* d_slots, size_t n, void* d_ok,
                                          void* hip_stream);
/* Test only: the keyed walk, one case per lane, host pointers, in the records of sbv_debug_secp256k1_sign_op (192 bytes in, 128 bytes
 * out, output field 3 = ok) plus one slot per case.
 *   op 0   in: u1 | u2 (below n)     out: x | y               the affine u1 G + u2 Q_slot through exactly the walk and the wavefront
 *                                                             rule of sbv_secp256k1_schnorr_verify_keyed; ok = 0 (all zero) for
 *                                                             infinity and for an out-of-range or invalid slot
 * Any other op is SBV_EINVAL; at most 65536 cases.  The final check is op 2 of sbv_debug_secp256k1_schnorr_op. */
int
sbv_debug_secp256k1_schnorr_keyed_op(int op, const uint8_t* in, const uint32_t* slots, uint8_t* out, size_t n);

/* Ed25519 batch signing (RFC 8032 section 5.1.6, pure Ed25519): the batch form of api.Signer.Sign for the Ed25519 variant, in two
 * steps so that a key is expanded once and not once per signature.  Signatures and public keys are byte-identical to RFC 8032,
 * Go's crypto/ed25519 and consensus_amd/host's Signer (the scheme is deterministic: tests compare every byte).
 *   sbv_ed25519_expand_keys   seeds: m x 32 bytes (the RFC 8032 private key).  expanded: m x 96 bytes, one EXPANDED RECORD per key:
 *                                 bytes  0..31  a mod L   the clamped secret scalar, reduced mod the group order L, little-endian
 *                                 bytes 32..63  prefix    the upper half of SHA-512(seed)
 *                                 bytes 64..95  A_enc     the public key
 *                             (a mod L and not a: the comb walker takes scalars below 2^253; B has order L, so [a mod L]B = A and
 *                             S = r + k (a mod L) mod L is the same S.)  pks: m x 32 bytes, or NULL when only the records are wanted.
 *                             A record is as secret as its seed.
 *   sbv_ed25519_sign_msgs     signature i = Ed25519(expanded[key_index[i]], msgs[msg_offsets[i] .. msg_offsets[i+1])); key_index == NULL
 *                             means key i % n_keys.  sigs: n x 64 bytes R | S; ok[i] = 1, or 0 with 64 zero bytes where key_index[i] >=
 *                             n_keys.  SBV_EINVAL: a null pointer (msgs may be null when every message is empty), n_keys == 0,
 *                             n > 2^21, an offset table that does not start at 0 or that decreases (the rule of
 *                             sbv_ed25519_verify_msgs).  n == 0 (m == 0) is SBV_OK and writes nothing.
 * The host-pointer forms use device buffers of the call's own size, wait for the result and zero the device copies of seeds and
 * records before they free them.
 * The `_stream` forms take device pointers (d_seeds, d_expanded, d_pks, d_key_index, d_sigs: 4-byte aligned; d_msg_offsets: n + 1
 * uint64, 8-byte aligned), launch on `hip_stream` and return without synchronising, under the stream contract of the `_dev` entries
 * above for every buffer they name.  They own no mutable device state — two calls on two streams share
 * nothing but the read-only comb of B, uploaded on the first Ed25519 call of the process — and they read only `hip_stream`-ordered
 * inputs, so nothing has to be joined back.  The device cannot refuse a whole call: a lane whose offset pair decreases answers
 * ok[i] = 0 and 64 zero bytes and reads nothing of the messages, like a lane with an unknown key; offsets beyond the message
 * buffer are the caller's error.  They are named `_stream` and not `_dev` because the schedules every `_dev` entry is run under are
 * a fixed table in tests/test_gpu_stream_order.py; the schedules of these two (late producer, early overwriter, X-Y-X) are in
 * tests/test_gpu_ed25519_sign.py.
 * NOT constant-time: the comb of B is indexed by digits of the secret scalars a and r and lives in HBM.  For load generation, test
 * traffic and trusted single-tenant hosts; see consensus_amd/csrc/ed25519_sign.h. */
int sbv_ed25519_expand_keys(const uint8_t* seeds, size_t m, uint8_t* expanded, uint8_t* pks);
int sbv_ed25519_sign_msgs(const uint8_t* expanded, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs,
                          const uint64_t* msg_offsets, size_t n, uint8_t* sigs, uint8_t* ok);
int sbv_ed25519_expand_keys_stream(const void* d_seeds, size_t m, void* d_expanded, void* d_pks, void* hip_stream);
int sbv_ed25519_sign_msgs_stream(const void* d_expanded, uint32_t n_keys, const void* d_key_index, const void* d_msgs,
                                 const void* d_msg_offsets, size_t n, void* d_sigs, void* d_ok, void* hip_stream);
/* Test only: one case of a unit operation of the signer per lane on the device, host pointers, 32 bytes out per case.
 * op 0: sc25519_muladd, in = k | a | r (96 bytes, each < L) -> (k a + r) mod L;  op 1: sc25519_reduce256, in = 32 bytes -> mod L;
 * op 2: in = a scalar s < L -> encode([s]B) through the comb walker and ed_encode.  Any other op is SBV_EINVAL. */
int sbv_debug_ed25519_sign_op(int op, const uint8_t* in, uint8_t* out, size_t n);

/* Message front end on the device: SHA-256 of each message and the strict DER
 * parse of each signature run as a kernel in front of the registered-key verification, so the host
 * only concatenates bytes.  msg i = msgs[msg_offsets[i] .. msg_offsets[i+1]), signature i (ASN.1 DER,
 * types.Signature.Value) = sigs[sig_offsets[i] .. sig_offsets[i+1]), signer = slots[i].
 * Equivalent to crypto/ecdsa.VerifyASN1(key[slots[i]], sha256(msg i), sig i) for every i. */
int sbv_p256_verify_msgs_keyed(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs,
                               const uint64_t* sig_offsets, const uint32_t* slots, size_t n, uint8_t* accept_bitmap);

/* ---- secp256k1 variant ("other curves": api.Verifier / api.Signer are curve-agnostic,
 * pkg/api/dependencies.go:46-71) --------------------------------------------------------------------------------------
 * The same 160-byte tuples r | s | hash | Qx | Qy and the same rules as sbv_p256_verify_batch (1 <= r, s <= n - 1, key
 * coordinates < p and on the curve, hash = leftmost 32 bytes reduced mod n, R = infinity rejected, accept iff
 * R.x mod n == r; no low-S rule at this layer) over y^2 = x^3 + 7, p = 2^256 - 2^32 - 977.  One lane per signature
 * (consensus_amd/csrc/k256_core.h); the 35.7 MB comb of G is built on the first call of a process. */
int sbv_secp256k1_verify_batch(const uint8_t* tuples, size_t n, uint8_t* accept_bitmap);
int sbv_secp256k1_verify_batch_dev(const void* d_tuples, size_t n, void* d_bitmap, void* hip_stream);

/* ---- Ed25519 variant (BASELINE.json configs[4]) ----------------------------------------------------
 * Semantics of Go crypto/ed25519.Verify(pk, msg, sig) (crypto/internal/edwards25519): S canonical,
 * A decoded with Go's leniency (non-canonical y accepted, no small-order rejection), cofactorless
 * [S]B = R + [k]A checked by re-encoding R byte-wise.
 * Tuple, 128 bytes little-endian as on the wire:  R (32) | S (32) | public key (32) | k (32), where
 * k = SHA-512(R || pk || msg) mod L is produced by sbv_ed25519_make_tuples (host) or, for the raw-message
 * entry sbv_ed25519_verify_msgs, on the device.  A tuple with k >= L or S >= L is rejected.  len(sig) != 64 is
 * the caller's reject (encode S = 2^256 - 1). */
#define SBV_ED25519_TUPLE_BYTES 128
int sbv_ed25519_verify_batch(const uint8_t* tuples, size_t n, uint8_t* accept_bitmap);
int sbv_ed25519_verify_batch_dev(const void* d_tuples, size_t n, void* d_bitmap, void* hip_stream);
/* Builds the tuples: sigs n x 64, pks n x 32, msgs packed (offsets[i]..offsets[i+1]) -> tuples n x 128. */
int sbv_ed25519_make_tuples(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* offsets,
                            size_t n, uint8_t* tuples_out);
/* Raw-message entry: the same inputs as sbv_ed25519_make_tuples, hashed on the device (SHA-512 + reduction mod L per
 * lane, consensus_amd/csrc/sha512_dev.h) and verified in the same call; n <= 2^21.  What a Verifier's
 * VerifyProposal / decision replay hands over when signatures are Ed25519 (internal/bft/view.go:555). */
int sbv_ed25519_verify_msgs(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* msg_offsets,
                            size_t n, uint8_t* accept_bitmap);

/* Registered Ed25519 keys: the consenters' (and registered clients') keys get a slot once, after which a verification against
 * that key needs no doublings and no grouping work: [S]B from the comb of B plus [k](-A) in 32 additions from the slot's 8-bit
 * comb of -A (384 KiB of HBM per key), or in 16 from a 16-bit comb after sbv_ed25519_widen_keys (64 MiB per key).  Four launches
 * per call: records -> tuples (A from the registry), [S]B, [k](-A), the encoding check (consensus_amd/csrc/ed25519_keyed.h).
 *   pks: m x 32 bytes (the encoded A).  slots_out[i] = slot of pks[i].  Slots are keyed by the encoding's BYTES, not by the point:
 *     k hashes the bytes, so two encodings of one point get two slots; equal encodings share one.  An encoding that Go's
 *     edwards25519 Point.SetBytes refuses still gets a slot, flagged invalid: every signature against it is rejected.  At most
 *     65 536 keys (SBV_EINVAL beyond).  Nothing is allocated before the first registration.
 *   sbv_ed25519_wide_keys: cap on the slots with a 16-bit comb (0 = none; default 64 = 4 GiB; at most 4096); lowering it
 *     returns the slots beyond the cap to their 8-bit combs.  sbv_ed25519_widen_keys: 16-bit combs for the named slots, built on
 *     the device from their 8-bit combs; a slot that is wide already, is not a point or lies beyond the cap stays as it is (no
 *     error); an unregistered slot is SBV_EINVAL.  stats: out[0] = wide slots, out[1] = 16 (bits), out[2] = the cap,
 *     out[3] = KiB per wide comb.  sbv_ed25519_wide_selfcheck(slot) = 1 when the device comb equals the host builder's byte
 *     for byte, 0 when it differs, SBV_EINVAL when the slot has no wide comb.
 *   rsk: n x 96 bytes R | S | k, little-endian: the 128-byte tuple without A, with k = SHA-512(R || A || M) mod L over the
 *     registered encoding.  slots: n slots.  A wavefront whose signatures all belong to wide slots walks the 16-bit combs, any
 *     other the 8-bit combs every slot keeps; verdicts are bit-identical to sbv_ed25519_verify_batch on the equivalent tuples.
 *     An out-of-range slot, S >= L or k >= L is a reject, not an error; len(sig) != 64 is the caller's reject (S = 2^256 - 1).
 *     _dev: d_rsk 16-byte aligned, on `hip_stream`, the caller synchronises.
 *   sbv_ed25519_verify_msgs_keyed: sigs n x 64 (R | S), message i = msgs[msg_offsets[i] .. msg_offsets[i+1]), signer slots[i]; k is
 *     computed on the device from the registry's encoding; n <= 2^21.
 * A failed registration or widening (SBV_ENOMEM, SBV_EDEVICE) leaves the registry as it was.  These entries run on the default
 * context (registry replication to other devices is not provided); sbv_shutdown forgets the registry. */
int sbv_ed25519_register_keys(const uint8_t* pks, size_t m, uint32_t* slots_out);
int sbv_ed25519_key_count(void);
int sbv_ed25519_clear_keys(void);
int sbv_ed25519_wide_keys(uint32_t max_keys);
int sbv_ed25519_widen_keys(const uint32_t* slots, size_t m);
int sbv_ed25519_wide_key_stats(uint32_t out[4]);
int sbv_ed25519_wide_selfcheck(uint32_t slot);
int sbv_ed25519_verify_batch_keyed(const uint8_t* rsk, const uint32_t* slots, size_t n, uint8_t* accept_bitmap);
int sbv_ed25519_verify_batch_keyed_dev(const void* d_rsk, const void* d_slots, size_t n, void* d_bitmap, void* hip_stream);
int sbv_ed25519_verify_msgs_keyed(const uint8_t* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
                                  const uint32_t* slots, size_t n, uint8_t* accept_bitmap);

/* Registered secp256k1 keys: the consenters' (and registered clients') keys get a slot once, after which a verification against
 * that key needs no doublings, no per-signature table and no grouping work: u1 * G from the comb of G (13 additions at the default
 * 20 bits) plus u2 * Q in 32.2 additions from the slot's 8-bit comb of Q (33 x 128 x 64 B = 270 KiB of HBM per key), or in 16 from a
 * 16-bit comb after sbv_secp256k1_widen_keys (17 windows x 32 768 entries x 64 B = 35.7 MB per key).  Two launches per call: stage A on
 * the records, then one lane per signature (consensus_amd/csrc/k256_keyed.h).
 *   keys: m x 64 bytes Qx | Qy big-endian.  slots_out[i] = slot of keys[i].  Slots are keyed by the 64 key BYTES: equal keys share a
 *     slot, slots are numbered by first registration.  A key that pointFromAffine refuses (a coordinate >= p, a point off
 *     y^2 = x^3 + 7, (0, 0)) still gets a slot, flagged invalid: every signature against it is rejected.  At most 65 536 keys
 *     (SBV_EINVAL beyond).  Nothing is allocated before the first registration; capacity doubles from 64 slots, live slots are copied
 *     on the device.  The combs are built on the device and are byte for byte the tables the grouped step builds for the same key.
 *   The registry is its own: it never shares a table, a slot index or a hash with the P-256 registry or with either key-table cache
 *     (a byte string can be a point of both curves).  A slot number of one registry means nothing in the other.
 *   sbv_secp256k1_wide_keys: cap on the slots with a 16-bit comb (0 = none; default 64 = 2.3 GB; at most 4096); lowering it returns
 *     the slots beyond the cap to their 8-bit combs.  sbv_secp256k1_widen_keys: 16-bit combs for the named slots, built on the device
 *     from their 8-bit combs; a slot that is wide already, is invalid or lies beyond the cap stays as it is (no error); an
 *     unregistered slot is SBV_EINVAL.  stats: out[0] = wide slots, out[1] = 16 (bits), out[2] = the cap, out[3] = KiB per wide
 *     comb.  sbv_secp256k1_wide_selfcheck(slot) = 1 when the device comb equals the host builder's byte for byte, 0 when it differs,
 *     SBV_EINVAL when the slot has no wide comb.
 *   rsh: n x 96 bytes r | s | hash, big-endian: the 160-byte tuple without its key.  slots: n slots.  A wavefront whose live
 *     signatures all belong to wide slots walks the 16-bit combs, any other the 8-bit combs every slot keeps; verdicts are
 *     bit-identical to sbv_secp256k1_verify_batch on the equivalent 160-byte tuples.  An out-of-range slot, r or s outside
 *     [1, n - 1] and R = infinity are rejects, not errors: return codes never mean "invalid signature".  Batches larger than 2^21
 *     are chunked.  _dev: d_rsh 16-byte aligned, on `hip_stream`, the caller synchronises.
 *   sbv_secp256k1_verify_msgs_keyed: the device front end of sbv_p256_verify_msgs_keyed (SHA-256 + strict DER parse, which knows
 *     nothing of the curve) in front of the keyed step: message i = msgs[msg_offsets[i] .. msg_offsets[i+1]), DER signature i =
 *     sigs[sig_offsets[i] .. sig_offsets[i+1]), signer slots[i]; n <= 2^21; an offset table that does not start at 0 or decreases
 *     is SBV_EINVAL; a signature that does not parse is a reject.
 * A failed registration or widening (SBV_ENOMEM, SBV_EDEVICE) leaves the registry as it was.  These entries run on the default
 * context (registry replication to other devices is not provided); sbv_shutdown forgets the registry.  Without a device every
 * entry returns what its siblings return (SBV_ENODEV from sbv_init, SBV_ENOTINIT after it). */
int sbv_secp256k1_register_keys(const uint8_t* keys, size_t m, uint32_t* slots_out);
int sbv_secp256k1_key_count(void);
int sbv_secp256k1_clear_keys(void);
int sbv_secp256k1_wide_keys(uint32_t max_keys);
int sbv_secp256k1_widen_keys(const uint32_t* slots, size_t m);
int sbv_secp256k1_wide_key_stats(uint32_t out[4]);
int sbv_secp256k1_wide_selfcheck(uint32_t slot);
int sbv_secp256k1_verify_batch_keyed(const uint8_t* rsh, const uint32_t* slots, size_t n, uint8_t* accept_bitmap);
int sbv_secp256k1_verify_batch_keyed_dev(const void* d_rsh, const void* d_slots, size_t n, void* d_bitmap, void* hip_stream);
int sbv_secp256k1_verify_msgs_keyed(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs,
                                    const uint64_t* sig_offsets, const uint32_t* slots, size_t n, uint8_t* accept_bitmap);

/* Raw messages for the GENERIC verifiers (SURVEY.md §8(f) row 1 for signers that hold no slot: VerifyProposal's K client requests
 * when the clients are not registered, internal/bft/view.go:553-559).  The inputs of sbv_p256_verify_msgs_keyed with the signers'
 * keys in place of slots: message i = msgs[msg_offsets[i] .. msg_offsets[i+1]), DER signature i = sigs[sig_offsets[i] ..
 * sig_offsets[i+1]), keys = n x 64 bytes Qx | Qy, big-endian.  One kernel (consensus_amd/csrc/msg_frontend_kernels.hip, the same for
 * both curves) hashes the messages (SHA-256), parses the signatures (strict DER) and writes the 160-byte tuples on the device; the
 * tuple step then runs on them as on uploaded ones (grouped step, key-table cache and hot-key pools included).  Bit i equals what
 * sbv_p256_verify_batch / sbv_secp256k1_verify_batch return for the tuple sbv_p256_parse_der(sig i) | sbv_sha256_batch(msg i) |
 * keys[i]; for P-256 that is crypto/ecdsa.VerifyASN1(key i, sha256(msg i), sig i).  A signature that does not parse is a reject, and
 * so is a key the verifier refuses (a coordinate >= p, a point off the curve, (0, 0)): return codes never mean "invalid".
 *   SBV_ENOTINIT before sbv_init; n == 0 is SBV_OK and writes nothing; n > 2^21 is SBV_EINVAL, refused before any array is read;
 *   a null msg_offsets, sig_offsets, keys or accept_bitmap is SBV_EINVAL (msgs may be null when every message is empty); an offset
 *   table that does not start at 0 or that decreases is SBV_EINVAL.  A refused call leaves the library as it was.
 *   prep_us of sbv_last_timing includes the front-end kernel (P-256: and stage A).
 * Measured (one MI355X, 2^20 requests over 1 024 signers, pageable host memory; tools/bench_verify_msgs.py): against SHA-256 + strict DER on 16 CPUs
 * followed by the tuple entry, one call of these entries takes, for messages of 64 / 200 / 1 024 bytes, P-256 11.50 → 7.56 / 13.74 → 10.01 / 37.97 → 26.80 ms and secp256k1 12.40 → 9.47 / 15.19 → 12.47 / 33.11 → 29.02 ms
 * (medians of 10 calls).  At no measured size is the entry slower than that route.  The call itself is longer than the tuple call alone (more bytes go up, and
 * the SHA-256 loader reads byte by byte: the front-end kernel takes 0.38 / 0.66 / 2.23 ms per 2^20 messages of those sizes); what it saves is the host's pass.
 * The sharded form overlaps the uploads with the kernels, piece by piece: 5.61 / 8.39 / 23.94 ms on one device. */
int sbv_p256_verify_msgs(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets,
                         const uint8_t* keys, size_t n, uint8_t* accept_bitmap);
int
sbv_secp256k1_verify_msgs(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets,
                          const uint8_t* keys, size_t n, uint8_t* accept_bitmap);

/* Raw-message ECDSA signing: SHA-256, RFC 6979 signing and DER in one call, the signing side of the two entries above and the ECDSA
 * form of sbv_ed25519_sign_msgs.  Signature i = DER SEQUENCE { INTEGER r, INTEGER s } of ECDSA(keys[key_index[i]],
 * SHA-256(msgs[msg_offsets[i] .. msg_offsets[i+1]))) with the deterministic nonce of RFC 6979; with flags = 0 byte-identical to
 * Signer::Sign of consensus_amd/host.  key_index == NULL means key i % n_keys; keys: n_keys x 32 bytes (private scalar, big-endian).
 * Three kernels run per call: k_sha256_msgs (one lane per message), the signing kernel of sbv_p256_sign_batch /
 * sbv_secp256k1_sign_batch as it is, and k_ecdsa_sig_finish (low-S for P-256, the minimal DER encoding as a 72-byte record);
 * consensus_amd/csrc/ecdsa_sign_msgs.h, ecdsa_sign_msgs_kernels.hip.
 *   flags   SBV_ECDSA_SIGN_LOW_S: s > (n-1)/2 is replaced by n - s on either curve (Fabric's BCCSP refuses the high form of P-256;
 *           secp256k1: the flag of sbv_secp256k1_sign_batch, passed through, recid bit 0 flipped with it).  Any other bit is SBV_EINVAL.
 * Host forms (sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs): the signatures come back packed back to back in sigs (the caller provides
 * SBV_ECDSA_DER_MAX * n bytes) with sig_offsets (n + 1 entries, the first 0): exactly the pair sbv_p256_verify_msgs /
 * sbv_secp256k1_verify_msgs take.  The packing is a host pass over the downloaded records.  ok: n bytes; recid: n bytes or NULL.
 * A refused item has ok[i] = 0, an empty signature (equal offsets) and recid 0: a key outside [1, n-1], an index >= n_keys, and in a
 * `_stream` call a decreasing offset pair.
 * `_stream` forms: device pointers, launched on `hip_stream`, no synchronisation, under the stream contract of the `_dev` entries
 *  for every buffer they name; they own no mutable device state and may be the first call after sbv_init.
 * They write d_records (n x 72 bytes, record i zero behind its length, all zero when refused), d_len (n bytes: 0 or 8..72), d_ok
 * and, for secp256k1, d_recid (or NULL).  d_work: sbv_ecdsa_sign_msgs_workspace(n) bytes (the digests and r | s between the
 * kernels), the caller's, 4-byte aligned, not shared between calls in flight.
 * sbv_sha256_msgs: the first kernel on its own: digests = n x 32 bytes, SHA-256 of message i; in the `_stream` form a decreasing
 * offset pair gives the digest of the empty message.
 * SBV_ENOTINIT before sbv_init, whatever the arguments.  n == 0 is SBV_OK and writes nothing.  SBV_EINVAL, with nothing written: a null
 * required pointer (msgs may be null when every message is empty), n_keys == 0, an unknown flag bit, n > 2^21, in a host form an
 * offset table that does not start at 0 or that decreases, in a `_stream` form a misaligned device pointer (4 bytes for keys, key
 * index, records, digests and workspace, 8 for the offsets).  A refused call leaves the library as it was.
 * The host forms use device buffers of the call's own size, wait for the result and zero the device copy of the keys before they
 * free it.  NOT constant-time, like the signers underneath (secret-indexed table lookups in HBM; low-S and the encoder branch on s and
 * on the leading bytes of r and s): for test traffic and trusted single-tenant hosts.
 *   sbv_debug_ecdsa_der_op   test only: k_ecdsa_sig_finish on given integers.  curve 0 = P-256, 1 = secp256k1; rs: n x 64 bytes;
 *                            flags SBV_ECDSA_SIGN_LOW_S applies low-S (s must then be in [1, n-1]); records: n x 72, len: n bytes.
 *                            An unknown curve or flag, a null pointer or n > 2^21 is SBV_EINVAL. */
#define SBV_ECDSA_SIGN_LOW_S 1u        /* same bit as SBV_K256_SIGN_LOW_S */
#define SBV_ECDSA_DER_MAX 72
int sbv_sha256_msgs(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, uint8_t* digests);
int sbv_sha256_msgs_stream(const void* d_msgs, const void* d_msg_offsets, size_t n, void* d_digests, void* hip_stream);
int sbv_p256_sign_msgs(const uint8_t* keys, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs,
                       const uint64_t* msg_offsets, size_t n, uint32_t flags, uint8_t* sigs, uint64_t* sig_offsets, uint8_t* ok);
int
sbv_secp256k1_sign_msgs(const uint8_t* keys, uint32_t n_keys, const uint32_t* key_index, const uint8_t* msgs,
                        const uint64_t* msg_offsets, size_t n, uint32_t flags, uint8_t* sigs, uint64_t* sig_offsets, uint8_t* recid,
                        uint8_t* ok);
size_t sbv_ecdsa_sign_msgs_workspace(size_t n);
int sbv_p256_sign_msgs_stream(const void* d_keys, uint32_t n_keys, const void* d_key_index, const void* d_msgs,
                              const void* d_msg_offsets, size_t n, uint32_t flags, void* d_records, void* d_len, void* d_ok,
                              void* d_work, void* hip_stream);
int
sbv_secp256k1_sign_msgs_stream(const void* d_keys, uint32_t n_keys, const void* d_key_index, const void* d_msgs,
                               const void* d_msg_offsets, size_t n, uint32_t flags, void* d_records, void* d_len, void* d_recid,
                               void* d_ok, void* d_work, void* hip_stream);
int sbv_debug_ecdsa_der_op(int curve, uint32_t flags, const uint8_t* rs, uint8_t* records, uint8_t* len, size_t n);

/* SEC1 public keys.  Every ECDSA entry above takes a key as 64 raw bytes Qx | Qy; keys travel as SEC1 octet strings (SEC1 2.3.3: 65
 * bytes 04 | X | Y, or 33 bytes 02/03 | X — the content of an X.509 SubjectPublicKeyInfo, Go's elliptic.Marshal /
 * MarshalCompressed, every secp256k1 key on a wire).  These entries decode them on the device, one key per lane
 * (consensus_amd/csrc/sec1_keys.h, sec1_keys_kernels.hip): the compressed form costs a square root mod p per key, a^((p+1)/4) on either
 * curve (253 squarings).  The rules are SEC1 2.3.4 as Go applies them (elliptic.Unmarshal, elliptic.UnmarshalCompressed):
 *   length 65, first byte 04        accepted iff X < p, Y < p and the point is on the curve
 *   length 33, first byte 02 / 03   accepted iff X < p and X^3 + aX + b is a square; Y is the root whose low bit is the prefix's
 *   everything else                 refused: any other length (0 and 1 included, so the one-byte point at infinity too) and the hybrid
 *                                   prefixes 06 / 07 (Go and Bitcoin's strict-encoding rule refuse them; libsecp256k1 and OpenSSL
 *                                   would accept them)
 * A refused key is 64 zero bytes and ok[i] = 0; an accepted one is X | Y and ok[i] = 1.  (0, 0) is on neither curve, so every
 * verifier of the library rejects against a refused key.  Only the bytes of key i are read, at any alignment.
 *   sbv_*_decode_keys          keys: the m keys packed back to back; key i = keys[key_offsets[i] .. key_offsets[i+1]).  key_offsets ==
 *                              NULL means the fixed 33-byte stride, key i = keys[33 i .. 33 i + 33) (compressed keys only).
 *                              Otherwise m + 1 offsets, the first 0, never decreasing, else SBV_EINVAL.  keys64: m x 64 bytes;
 *                              ok: m bytes or NULL.  The buffers are of the call's own size; the call waits for the result.
 *   sbv_*_decode_keys_stream   device pointers, launched on `hip_stream`, no synchronisation, under the stream contract of the `_dev`
 *                              entries for every buffer they name.  They own no mutable device state and
 *                              may be the first call of a process after sbv_init.  key_bytes: the size of d_keys; each lane holds
 *                              its own offset pair against it (monotone, inside it), and a pair that fails is a refused key, not
 *                              a read outside the buffer.  With d_key_offsets == NULL a key behind key_bytes is refused likewise.
 *                              d_keys64 must be 4-byte aligned and d_key_offsets 8-byte aligned, else SBV_EINVAL; d_keys and d_ok may
 *                              be at any address.
 * SBV_ENOTINIT before sbv_init, whatever the arguments; m == 0 is SBV_OK and writes nothing; a null keys with m > 0, a null keys64 or
 * m > 2^32 is SBV_EINVAL with nothing written.  A refused call leaves the library as it was.
 * Registering a compressed key is decode_keys followed by sbv_p256_register_keys / sbv_secp256k1_register_keys on keys64, as
 * sbv_secp256k1_schnorr_lift_keys followed by register_keys registers an x-only key.
 *   sbv_*_verify_msgs_sec1     sbv_p256_verify_msgs / sbv_secp256k1_verify_msgs with the signers' keys as a packed SEC1 array: key i =
 *                              keys[key_offsets[i] .. key_offsets[i+1]) (NULL: the 33-byte stride).  The packed keys and their offsets
 *                              go up, the decode kernel fills the n x 64 key array the front end reads, and the existing path runs
 *                              untouched.  Bit i is by definition what the verify_msgs entry of the curve returns when keys[i] is the
 *                              64 bytes decode_keys writes for key i: a refused key is a reject, never an error.  Limits (n <= 2^21),
 *                              return codes and prep_us accounting (the decode kernel counts as prep) as verify_msgs; a key offset
 *                              table that does not start at 0 or that decreases is SBV_EINVAL.  Keys are decoded once per SIGNATURE,
 *                              not once per distinct signer.  For signers that repeat: decode once, register the keys, and use the
 *                              keyed entries (sbv_p256_verify_msgs_keyed, sbv_secp256k1_verify_msgs_keyed).  No sharded form.
 *   sbv_debug_sec1_op          test only: one case per lane, n <= 65 536, curve 0 = P-256, 1 = secp256k1; in: n x 192 bytes, out: n x
 *                              128 bytes, byte 127 = ok, all zero when not ok (the records of sbv_debug_secp256k1_recover_op).
 *                                op 0  a (32 bytes, taken mod p) -> a^((p+1)/4) mod p (32 bytes); ok = a is a square
 *                                op 1  x (32 bytes), parity (byte 63: 0 / 1) -> x | y of the point with that x and parity; ok = 0
 *                                      for x >= p, no point with that x, or a parity byte above 1
 *                              Any other op or curve, a null pointer or n > 65 536 is SBV_EINVAL. */
int sbv_p256_decode_keys(const uint8_t* keys, const uint64_t* key_offsets, size_t m, uint8_t* keys64, uint8_t* ok);
int
sbv_secp256k1_decode_keys(const uint8_t* keys, const uint64_t* key_offsets, size_t m, uint8_t* keys64, uint8_t* ok);
int sbv_p256_decode_keys_stream(const void* d_keys, const void* d_key_offsets, size_t key_bytes, size_t m, void* d_keys64,
                                void* d_ok, void* hip_stream);
int
sbv_secp256k1_decode_keys_stream(const void* d_keys, const void* d_key_offsets, size_t key_bytes, size_t m, void* d_keys64,
                                 void* d_ok, void* hip_stream);
int sbv_p256_verify_msgs_sec1(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets,
                              const uint8_t* keys, const uint64_t* key_offsets, size_t n, uint8_t* accept_bitmap);
int
sbv_secp256k1_verify_msgs_sec1(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets,
                               const uint8_t* keys, const uint64_t* key_offsets, size_t n, uint8_t* accept_bitmap);
int sbv_debug_sec1_op(int curve, int op, const uint8_t* in, uint8_t* out, size_t n);

/* Strict DER parse of an ECDSA-Sig-Value with Go x/crypto/cryptobyte rules
 * (crypto/ecdsa.parseSignature): out = r | s, 32 bytes each, big-endian, zero padded.
 * Returns SBV_OK or SBV_EPARSE (then out is all zero, which every verify rejects). */
int sbv_p256_parse_der(const uint8_t* der, size_t len, uint8_t out_rs[64]);

/* SHA-256 of n messages packed back to back (offsets[i]..offsets[i+1]) -> n*32 bytes.
 * Host implementation used to build tuples (hash = SHA-256(Signature.Msg)).  On x86-64 CPUs with the SHA extensions the
 * compression function runs on them (as Go's crypto/sha256 does); sbv_sha256_uses_cpu_extensions() says which one is in use
 * (SBV_SHA_PORTABLE=1 in the environment keeps the portable loop). */
int sbv_sha256_batch(const uint8_t* msgs, const uint64_t* offsets, size_t n, uint8_t* out_hashes);
int sbv_sha256_uses_cpu_extensions(void);

typedef struct sbv_timing {
    double h2d_us;      /* host -> device copy of the tuples   (host-pointer entry only) */
    double prep_us;     /* stage A kernel (range checks, s^-1, u1, u2)                   */
    double verify_us;   /* stage B kernel (u1*G + u2*Q, final comparison)                */
    double d2h_us;      /* bitmap device -> host                                          */
    double total_us;    /* wall clock of the whole call                                   */
    uint64_t n;         /* tuples in the call                                             */
} sbv_timing;
/* Timing of the most recent sbv_p256_verify_batch call made by any thread. */
int sbv_last_timing(sbv_timing* out);

/* Per-kernel timing of the device-pointer entries (bench.py's roofline leg).  While enabled,
 * every call of a device-pointer verify entry (sbv_p256_verify_batch_dev, sbv_p256_verify_batch_keyed_dev,
 * sbv_ed25519_verify_batch_dev, sbv_ed25519_verify_batch_keyed_dev, sbv_secp256k1_verify_batch_dev) records HIP events
 * around its kernels ON THE CALLER'S STREAM; sbv_profile_read waits for them and returns the sums (microseconds) and the
 * number of stage-B launches since the previous read (a step without stage A records its middle event at its start).
 * on = 1: an event triple per launch (before stage A, after stage A, after stage B) AND a pair around every launch of the
 * dominant kernel; on = 2: the dominant-kernel pairs only (what bench.py keeps inside its timed region: every recorded event
 * is a packet between two kernels of the step); on = 0: off.  Process-wide: applies to every initialised device and to
 * devices initialised later. */
int sbv_profile_enable(int on);
int sbv_profile_read(double* prep_us, double* verify_us, uint64_t* launches);
/* Same window as sbv_profile_read (call it BEFORE sbv_profile_read, which resets): summed duration and number
 * of launches of the dominant stage-B kernel alone — k_verify_keyed_q (one launch per chunk of key-comb windows; k_ed_qphase /
 * k_k256_qphase for the grouped steps of the device-pointer entries of the other two schemes)
 * when the batch was grouped, else k_p256_verify. */
int sbv_profile_read_dominant(double* dominant_us, uint64_t* dominant_launches);
/* Device-side counters of the most recent grouped batch: out[0] = key groups, out[1] = tuples verified through
 * the per-batch key tables, out[2] = tuples verified by the generic kernel, out[3] = ungrouped tuples rejected
 * for their public key alone (pointFromAffine: coordinate >= p or off the curve).  Synchronises the device. */
int sbv_p256_last_group_stats(uint32_t out[4]);
/* Table classes of the most recent grouped P-256 batch (round 5; consensus_amd/csrc/p256_group.h).  Every grouped key gets its ROWS —
 * the babies b * 2^(8j) Q and giants 16 a * 2^(8j) Q of every window: a comb with 4-bit windows, two additions per window — which pay
 * from ~4 signatures per key; the FILL that completes the 8-bit comb (three quarters of a table's cost, one addition per window) is
 * spent on keys that sign at least 256 tuples of the batch (SBV_FULL_TABLE_MIN), also later: a key cached with rows only is upgraded
 * by the first batch in which it is hot.  out[0] = groups verified from a full table, out[1] = groups whose table was filled in this
 * batch, out[2] = grouped tuples served by the rows-only pass.  Verdicts never depend on the class.  Synchronises the device.
 * K arbitrary clients per proposal: internal/bft/view.go:553-559. */
int sbv_p256_last_table_classes(uint32_t out[3]);
/* Pools of the grouped P-256 step on the default device (round 6).  The defaults — a key-table cache of 16 384 keys and 65 536 groups per
 * batch: 25 GB of combs — are sized for a 288 GB MI355X; a device that cannot hold them (a shared or smaller part, one of several
 * contexts folded onto one GPU by SBV_LOGICAL_DEVICES) gets halved pools instead of SBV_ENOMEM, and a batch whose pools cannot be
 * allocated at all is verified by the one-lane kernel: a Verifier must stay live (internal/bft/view.go:387-392 deposes a leader on a
 * VerifyProposal error).  out[0] = cached keys the pool holds, out[1] = groups per batch, out[2] = 1 when either is smaller than asked
 * for, out[3] = grouped batches that fell back to the one-lane kernel for lack of memory, out[4] = combs of the hot-key pool,
 * out[5] = contexts sharing this GPU.  out[0..1] are 0 before the first grouped batch.  Rates change with the pools, verdicts never. */
int sbv_p256_pool_stats(uint32_t out[6]);
/* Diagnostics (tests / tools): every promoted hot-key comb of context `device` compared with the host builder, and the consistency of the
 * pool's bookkeeping.  out[0] promoted slots, [1] combs that differ, [2] the first such comb, [3] its first differing entry, [4] how many of
 * its entries differ, [5] index / owner inconsistencies, [6] combs claimed by more than one slot, [7] combs handed out so far.  Slow. */
int sbv_debug_hot_check(int device, uint32_t out[8]);
/* Diagnostics (tests / tools): the key-grouping state that the LAST grouped launch of any scheme left in context `device` — the hash
 * table, representatives, counts, group lists, sort cursors and key-cache slots that no verdict shows.  Both calls wait for the device and
 * copy; they launch nothing.  sbv_debug_group_header: out[0] scheme (SBV_SCHEME_*; 0xFFFFFFFF before the first grouped launch), [1] n of
 * that launch, [2] ht_mask, [3] max_groups, [4] min_count, [5] sample_mask, [6] min_samples, [7] the grouping hash's seed, [8] sorted — as
 * the launch saw them —, [9] capacity and [10] on / off of the scheme's key-table cache, [11] a serial number that grows by one per grouped
 * launch, [12] groups of the batch, [13] cached keys, [14..15] 0.  sbv_debug_group_array copies elements [0, count) of one array
 * (u32 each; COLD and ACC: bytes) and answers SBV_EINVAL beyond its length: n for the per-tuple arrays, max_groups for the per-group
 * ones, ht_mask + 1, 12 counters, capacity x 16 key words, 4 cache counters. */
#define SBV_GROUP_ARRAY_HT 0
#define SBV_GROUP_ARRAY_REP 1
#define SBV_GROUP_ARRAY_CNT 2
#define SBV_GROUP_ARRAY_SLOT_OF 3
#define SBV_GROUP_ARRAY_GROUP_REP 4
#define SBV_GROUP_ARRAY_COUNTERS 5
#define SBV_GROUP_ARRAY_SLOTS 6
#define SBV_GROUP_ARRAY_GRP_IDX 7
#define SBV_GROUP_ARRAY_GRP_OF 8
#define SBV_GROUP_ARRAY_UNG_IDX 9
#define SBV_GROUP_ARRAY_UNG_CAND 10
#define SBV_GROUP_ARRAY_GCOUNT 11
#define SBV_GROUP_ARRAY_GCURSOR 12
#define SBV_GROUP_ARRAY_TSLOT 13
#define SBV_GROUP_ARRAY_COLD 14
#define SBV_GROUP_ARRAY_ACC 15
#define SBV_GROUP_ARRAY_CACHE_KEYS 16
#define SBV_GROUP_ARRAY_CACHE_COUNT 17
int sbv_debug_group_header(int device, uint32_t out[16]);
int sbv_debug_group_array(int device, int which, size_t count, void* out);
/* Hot keys (round 5): wide combs in the GENERIC path.  A key that arrives inside tuples — a client key of VerifyProposal
 * (internal/bft/view.go:553-559), a consenter of a replica that registered nothing — and keeps being hit is promoted: once the
 * key-table cache has verified `min_hits` tuples against its slot, a 16-bit comb (35.7 MB; up to `max_keys` of them, default 1024 =
 * 36.5 GB of the 288, less if the device lacks the room) is built on the device behind a batch's verdicts, at most 64 keys per batch,
 * from base points the slot's 8-bit table already holds.  Later batches verify its tuples in 13 + 17 comb additions instead of
 * 13 + 32, in one launch that needs no table of the batch.  Needs the key-table cache (on by default); verdicts never depend on it.
 * max_keys = 0 switches it off; min_hits = 0 keeps the current value (default 4096).  Env: SBV_HOT_KEYS, SBV_HOT_MIN_HITS.
 * stats: out[0] = promoted keys, out[1] = pool capacity, out[2] = tuples the wide pass served in the last grouped batch,
 * out[3] = min_hits.  sbv_p256_hot_selfcheck(i) = 1 when promoted comb i equals the host builder's output for its key. */
int sbv_p256_hot_keys(uint32_t max_keys, uint32_t min_hits);
int sbv_p256_hot_key_stats(uint32_t out[4]);
int sbv_p256_hot_selfcheck(uint32_t index);
/* The same for the Ed25519 variant (round 6): a cache slot of that scheme whose count passes `min_hits` gets a 16-bit comb of -A
 * (16 windows x 32 768 affine-Niels entries at a 128-byte pitch = 64 MiB), built on the device from base points the slot's 8-bit comb
 * holds; later batches add [k](-A) for its tuples in 16 additions instead of 32, in one launch that needs no table of the batch.  Same
 * bookkeeping as above (counts per slot, decay, eviction with hysteresis).  Default: up to 1024 keys (64 GiB of the 288; fewer if the
 * device lacks the room) from 4096 hits on; max_keys = 0 switches it off; env SBV_ED_HOT_KEYS, SBV_ED_HOT_MIN_HITS.  A comb costs
 * about 80 us of device time to build, behind a batch's verdicts, and saves about 0.5 ns per tuple verified from it afterwards: it
 * pays for signers that stay (consenters), which is what the decaying count selects.  Verdicts never depend on it.  stats /
 * selfcheck as for P-256. */
int sbv_ed25519_hot_keys(uint32_t max_keys, uint32_t min_hits);
int sbv_ed25519_hot_key_stats(uint32_t out[4]);
int sbv_ed25519_hot_selfcheck(uint32_t index);
/* The same for the secp256k1 variant: a cache slot of that scheme whose count passes `min_hits` gets a 16-bit comb of Q (17 windows x
 * 32 768 affine entries of 64 bytes = 35.7 MB, the layout of the registered path's widened slots), built on the device from the slot's
 * 8-bit comb; later batches add u2 * Q for its tuples in 17 additions instead of 32.2, in one launch that needs no table of the batch.
 * Same bookkeeping as above (counts per slot, decay, at most 64 promotions per batch, eviction with hysteresis).  OFF by default:
 * sbv_secp256k1_hot_keys(max_keys, min_hits) switches the pool on with up to max_keys combs (at most 4096; fewer if the device lacks
 * the room), max_keys = 0 switches it off and frees it; min_hits = 0 keeps the current value (default 4096); env SBV_K256_HOT_KEYS,
 * SBV_K256_HOT_MIN_HITS.  Needs this scheme's key-table cache; forgotten whenever the cache is.  Verdicts never depend on it.  stats /
 * selfcheck as for P-256: selfcheck(i) = 1 when promoted comb i equals the host builder's comb of its owner's key byte for byte.
 * (The return types stand on lines of their own: the registered-key entries above are counted by their one-line form.) */
int
sbv_secp256k1_hot_keys(uint32_t max_keys, uint32_t min_hits);
int
sbv_secp256k1_hot_key_stats(uint32_t out[4]);
int
sbv_secp256k1_hot_selfcheck(uint32_t index);

/* Page-locked host memory for the host-pointer entries.  Handing pageable memory to a 100 MB batch makes the HIP
 * runtime pin (or bounce) it inside the call — measured at 25 ms for a 550 000-signature replay batch whose kernels
 * take 5 ms.  A caller that lays its batch out in sbv_host_alloc memory gets a plain DMA.  NULL on failure (or
 * before sbv_init); sbv_host_free accepts NULL. */
void* sbv_host_alloc(size_t bytes);
void sbv_host_free(void* p);

/* ---- every GPU of the node behind one process ---------------------------------------------------------------------
 * The reference injects ONE Verifier into a replica process (pkg/consensus/consensus.go:35, 107); that process drives all
 * the GPUs of its node.  sbv_init(d) may be called for several devices (the first one stays the default of the
 * single-device entry points above); sbv_init_all() initialises every visible gfx950 device and returns how many.
 *
 * sbv_p256_verify_batch_sharded splits a host batch into contiguous shards, one per device (BASELINE.json: "client-request
 * signatures queued in the RequestPool and the 2f+1 consenter Commit signatures collected per proposal are sharded across
 * the 8 GPUs of one node"), each a multiple of lcm(512, 8 * group) tuples: whole bitmap bytes per device and — with
 * group = signatures per proposal (11 at N = 16: internal/bft/util.go:183-187) — whole proposals, so that each device
 * also emits the per-proposal quorum bit (>= quorum accepted signatures by DISTINCT keys, the rule of
 * internal/bft/viewchanger.go:681-727).  When more than one device took part, one in-place ncclAllGather of the bitmap
 * shards (RCCL over xGMI, uint8, per-device streams) leaves the full bitmap on every device and one D2H returns it (with
 * fewer shards than devices the idle ranks of the node-wide communicator join with an unused slot); a batch smaller than
 * twice the per-device minimum is NOT split — it goes whole to one device, round-robin, with no collective.  The minimum is
 * chosen per batch (sbv_shard_min_for: 2^16 tuples when a sample of the batch shows a handful of signers — consenter commit
 * signatures, configs[3]: 550 000 tuples over 16 keys span 8 devices, 68 750 each — and 2^17 otherwise; SBV_SHARD_MIN
 * overrides both).
 * Each device takes its shard in pieces through two upload slots: the host -> device copy of piece i + 1 runs on a copy stream
 * beside the kernels of piece i (pieces of 2^18 tuples while the key-table cache is on — the first piece builds the signers'
 * combs, the later ones find them — and whole launches when it is off; SBV_SHARD_PIECE overrides the size).
 *   group = 0: plain tuples.  quorum_bitmap may be NULL; otherwise ceil((n / group) / 8) bytes, bit p = proposal p.
 *   info (optional) reports what was done.  sbv_shard_plan is the pure split (testable without a GPU):
 *   first[0..shards], returns shards.  sbv_p256_verify_batch_on runs a whole batch on one chosen device. */
typedef struct sbv_shard_info {
    int devices;              /* devices available to the call                              */
    int shards;               /* shards the batch was split into (1 = not split)            */
    int mode;                 /* 0 = one device, 1 = RCCL all-gather, 2 = per-device D2H, 3 = key-affine + RCCL all-reduce, 4 = key-affine + host OR */
    size_t tuples_per_shard;
    double h2d_us;            /* slowest device: the copies' own durations, summed over its pieces           */
    double kernels_us;        /* slowest device: end of its first copy -> end of its last kernel (stage A + B,
                                 quorum bits; waits for later copies included)                                */
    double gather_us;         /* all-gather + final D2H                                      */
    double total_us;
} sbv_shard_info;
/* SBV_LOGICAL_DEVICES=G (environment, read at initialisation; round 6): sbv_init accepts G device indices and sbv_init_all creates G
 * contexts, context i on HIP device i % (visible devices), every pool budget divided by the contexts that share a GPU.  One MI355X then
 * runs the sharded entries exactly as a G-GPU node would — G shards from G host threads, shard offsets > 0, idle contexts, the bitmap
 * gathered through the host (an RCCL communicator needs one rank per physical device) — which is how the one-GPU test tier covers them.
 * sbv_init_all initialises its devices in parallel, one host thread each. */
int sbv_init_all(void);
int sbv_initialised_devices(int* out, int max);
size_t sbv_shard_plan(size_t n, int devices, size_t group, size_t min_per_device, size_t* first);
/* The per-device minimum the sharded entry plans THIS host batch with (pure host code, no device needed): the public keys of
 * 256 evenly spaced tuples are compared; <= 32 distinct ones = few signers.  Reference: the traffic it tells apart is
 * ValidateLastDecision / decision replay (internal/bft/viewchanger.go:681-727: N consenters) against VerifyProposal's K
 * client requests (internal/bft/view.go:553-559). */
size_t sbv_shard_min_for(const uint8_t* tuples, size_t n, size_t group);
int sbv_p256_verify_batch_sharded(const uint8_t* tuples, size_t n, size_t group, uint32_t quorum, uint8_t* accept_bitmap,
                                  uint8_t* quorum_bitmap, sbv_shard_info* info);
int sbv_p256_verify_batch_on(int device, const uint8_t* tuples, size_t n, uint8_t* accept_bitmap);
/* The registered-key form of the sharded entry (round 5): configs[3] as BASELINE.json words it — "11 consenter sigs x 50k proposals
 * sharded over 8 GPUs" — on the consenters' resident combs.  rsh: n x 96 bytes r | s | hash, slots: n key slots (100 B per signature
 * over PCIe instead of 160).  The key registry is process-wide: sbv_p256_register_keys / sbv_p256_widen_keys replicate a key's 8-bit
 * comb and a consenter's wide comb onto every initialised device (a device initialised later, or one whose replication failed, is
 * brought up to date in front of the call; if that fails the call returns < 0 — a stale device never answers "invalid"), so a slot
 * means the same key wherever its shard lands.  Plan, pieces (2^17 signatures; SBV_SHARD_PIECE_KEYED), collective and info as for
 * sbv_p256_verify_batch_sharded with the few-signers minimum (2^16 per device); quorum bit p = proposal p carries >= quorum accepted
 * signatures by DISTINCT slots (equal keys share a slot), the rule of internal/bft/viewchanger.go:681-727 for the signatures
 * internal/bft/view.go:531-541 collects.  Also the pipelined host-pointer entry for large registered-key batches on ONE device
 * (sbv_init only): the upload of piece i + 1 runs beside the kernels of piece i.  An out-of-range slot is a reject, not an error. */
int sbv_p256_verify_batch_keyed_sharded(const uint8_t* rsh, const uint32_t* slots, size_t n, size_t group, uint32_t quorum,
                                        uint8_t* accept_bitmap, uint8_t* quorum_bitmap, sbv_shard_info* info);
/* ... and its raw-messages form: sbv_p256_verify_msgs_keyed's inputs (messages and DER signatures packed back to back, their offset
 * tables, key slots) through the same plan — SHA-256 and the strict DER parse run on every device over its share, piece by piece
 * beside the uploads, so a replaying replica's host pass only lays bytes out (decision replay: internal/bft/controller.go:587-633;
 * the signatures of a decision: pkg/types/types.go:31-34).  No 2^21 limit: pieces are launches.  The offset tables need not start
 * at 0 (msgs / sigs are the bases they refer to: a slice of a larger batch's tables is a valid argument).  Equivalent to
 * crypto/ecdsa.VerifyASN1(key[slots[i]], sha256(msg i), sig i) for every i; quorum bits as above. */
int sbv_p256_verify_msgs_keyed_sharded(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets,
                                       const uint32_t* slots, size_t n, size_t group, uint32_t quorum, uint8_t* accept_bitmap,
                                       uint8_t* quorum_bitmap, sbv_shard_info* info);
/* The raw-messages form of sbv_p256_verify_batch_sharded: sbv_p256_verify_msgs's inputs (keys, not slots: no registry is read)
 * through the tuple entry's plan and pieces (2^18 signatures while the key-table cache is on; SBV_SHARD_PIECE), SHA-256 and the strict
 * DER parse on every device over its share, piece by piece beside the uploads.  No 2^21 limit; the offset tables need not start at 0;
 * a piece whose table slice decreases or is implausible (more than 64 KiB per message or 4 KiB per signature on average) is
 * SBV_EINVAL.  The per-device minimum comes from the same 256-key sample as sbv_shard_min_for, taken from `keys`.  Quorum bits count
 * DISTINCT keys.  This entry ALWAYS splits contiguously, whatever sbv_shard_mode says: the key-affine split hands every device the
 * whole batch, which here would mean every message to every device.  Verdicts as sbv_p256_verify_msgs. */
int sbv_p256_verify_msgs_sharded(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sigs, const uint64_t* sig_offsets,
                                 const uint8_t* keys, size_t n, size_t group, uint32_t quorum, uint8_t* accept_bitmap,
                                 uint8_t* quorum_bitmap, sbv_shard_info* info);
/* Key-affine partition (the other way to spread a batch: by signer instead of by position).  A contiguous split hands every
 * device signatures of every signer, so every device builds every key's tables — the part of a cold step that does not shrink
 * with the shard.  With sbv_shard_mode(1, parts) the sharded entry partitions by a hash of the public key: part p (on device
 * p % devices; parts = 0 means one per device, more parts than devices run one after another — how a single GPU rehearses an
 * 8-GPU partition) verifies the tuples of "its" keys only.  Every participating device receives the WHOLE batch over its own
 * PCIe link (the price of not bucketing on the host); the per-device bitmaps have disjoint bits and are combined with one
 * in-place ncclAllReduce(sum, uint8) (info->mode 3) or an OR on the host (mode 4); quorum bits are computed on the first device
 * from the combined bitmap.  Env: SBV_SHARD_MODE=keys, SBV_SHARD_PARTS=<n>.  Same verdicts as every other entry.
 * sbv_p256_verify_batch_dev_part is the device-resident building block: part `part` of `parts` of n tuples already in HBM
 * (default device), asynchronous on hip_stream except for ONE internal synchronisation (the member count sizes the launches);
 * d_bitmap_words: ceil(n / 32) 32-bit words, 4-byte aligned, receives this part's verdict bits (all other bits 0);
 * *part_tuples (optional) = how many tuples the part held.  Call sites: the same as sbv_p256_verify_batch_sharded
 * (VerifyProposal's K request signatures, decision replay: internal/bft/view.go:553-559, controller.go:587-633). */
int sbv_shard_mode(int by_key, unsigned parts);
int sbv_p256_verify_batch_dev_part(const void* d_tuples, size_t n, uint32_t part, uint32_t parts, void* d_bitmap_words,
                                   void* hip_stream, size_t* part_tuples);

/* Human-readable description of the calling thread's last failing call ("" if none). */
const char* sbv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SBV_H_ */
