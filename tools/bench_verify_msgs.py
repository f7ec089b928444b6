#!/usr/bin/env python3
"""The raw-message entries of the generic verifiers (include/sbv.h: sbv_p256_verify_msgs, sbv_secp256k1_verify_msgs,
sbv_p256_verify_msgs_sharded) against the host route they replace, one MI355X, one process.  One JSON line per curve and message size.

--n requests (default 2^20) over 1024 signers, every 8th spoiled (a message byte flipped), as the headline batch of bench.py; the
signatures are made on the device (RFC 6979) for --unique distinct messages (default 2^18) and repeated to fill the batch — neither
route remembers a verdict, so a repeated signature costs what a fresh one costs.  Messages of 64, 200 and 1 024 bytes.  Every bitmap is
compared with the tuple route's before anything is timed.  Per curve --settle untimed tuple calls first (the generic step's hot keys
settle), then per leg --warm calls and --steps timed ones; median, minimum and maximum:
  a  the host route as the Verifier runs it: make_tuples_ecdsa (SHA-256 + strict DER over the host library's worker pool), then the
     tuple entry; the host preparation and the call are timed separately
  b  the raw-message entry, one call
  c  prep_us of sbv_last_timing for b and for the tuple entry on the same signatures: the difference is the front-end kernel's share
  d  the sharded raw-message entry on one device (P-256 only)
All buffers are pageable host memory on both routes, as in the Verifier's path for unregistered clients.
Usage: bench_verify_msgs.py [--n N] [--unique U] [--sizes 64,200,1024] [--warm 3] [--steps 10] [--curves p256,k256]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402

import consensus_amd as sbv  # noqa: E402
import hostlib  # noqa: E402
import p256_py  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--unique", type=int, default=1 << 18)
ap.add_argument("--sizes", default="64,200,1024")
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--curves", default="p256,k256")
ap.add_argument("--signers", type=int, default=1024)
ap.add_argument("--settle", type=int, default=20, help="untimed tuple calls per curve before the first leg: the hot keys of the generic step settle (16 calls)")
args = ap.parse_args()
n, uniq, nk = args.n, min(args.unique, args.n), args.signers
assert n % uniq == 0 and n <= 1 << 21

sbv.init(0)
lib, host = sbv.load(), hostlib.load()
C, V, S, U64P = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
for name in ("sbv_p256_verify_msgs", "sbv_secp256k1_verify_msgs"):
    getattr(lib, name).argtypes = [V, V, V, V, V, S, V]
for name in ("sbv_p256_verify_batch", "sbv_secp256k1_verify_batch"):
    getattr(lib, name).argtypes = [V, S, V]
lib.sbv_p256_verify_msgs_sharded.argtypes = [V, V, V, V, V, S, S, ctypes.c_uint32, V, V, V]
host.sbvh_make_tuples_ecdsa.argtypes = [V, V, V, V, V, S, V]
host.sbvh_make_tuples_ecdsa.restype = None
host.sbvh_pubkey.argtypes = [C, C]


def summary(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def timed(fn, warm, steps):
    """wall-clock microseconds of `steps` calls after `warm` untimed ones; fn returns what to keep per call (or None)"""
    for _ in range(warm):
        fn()
    us, kept = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        k = fn()
        us.append(1e6 * (time.perf_counter() - t0))
        kept.append(k)
    return us, kept


def private_keys(curve):
    order = p256_py.N if curve == "p256" else 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
    return b"".join((int.from_bytes(hashlib.sha256(b"bench_verify_msgs %s %d" % (curve.encode(), i)).digest(), "big") % (order - 1) + 1).to_bytes(32, "big")
                    for i in range(nk))


def public_keys(curve, priv):
    if curve == "k256":
        pubs, ok = sbv.secp256k1_pubkeys(priv)
        assert ok == b"\x01" * nk
        return pubs
    out = b""
    for i in range(nk):
        q = ctypes.create_string_buffer(64)
        assert host.sbvh_pubkey(priv[32 * i:32 * i + 32], q) == 0
        out += q.raw
    return out


def batch(curve, size, priv, pubs):
    """(messages [n, size] uint8, DER blob, DER offsets [n + 1] uint64, keys [n, 64] uint8)"""
    rng = np.random.default_rng(size + (0 if curve == "p256" else 7))
    msgs_u = rng.integers(0, 256, (uniq, size), dtype=np.uint8)
    digests = b"".join(hashlib.sha256(msgs_u[i].tobytes()).digest() for i in range(uniq))
    kidx = [i % nk for i in range(uniq)]
    if curve == "p256":
        rs, ok = sbv.sign_batch(priv, digests, kidx)
    else:
        rs, _, ok = sbv.secp256k1_sign_batch(priv, digests, kidx)
    assert ok == b"\x01" * uniq
    ders = [p256_py.der_encode_sig(int.from_bytes(rs[64 * i:64 * i + 32], "big"), int.from_bytes(rs[64 * i + 32:64 * i + 64], "big")) for i in range(uniq)]
    reps = n // uniq
    msgs = np.ascontiguousarray(np.tile(msgs_u, (reps, 1)))
    msgs[7::8, size // 2] ^= 1                                  # every 8th request spoiled
    lens = np.array([len(d) for d in ders] * reps, dtype=np.uint64)
    soff = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=soff[1:])
    sigs = np.frombuffer(b"".join(ders) * reps, dtype=np.uint8).copy()
    pk = np.frombuffer(pubs, dtype=np.uint8).reshape(nk, 64)
    keys = np.ascontiguousarray(pk[np.arange(n) % uniq % nk])
    return msgs, sigs, soff, keys


def run(curve, size, priv, pubs):
    msgs, sigs, soff, keys = batch(curve, size, priv, pubs)
    moff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(size))
    tuples = np.zeros(n * 160, dtype=np.uint8)
    bm_a, bm_b, bm_d = (np.zeros((n + 7) // 8, dtype=np.uint8) for _ in range(3))
    entry = lib.sbv_p256_verify_msgs if curve == "p256" else lib.sbv_secp256k1_verify_msgs
    tuple_entry = lib.sbv_p256_verify_batch if curve == "p256" else lib.sbv_secp256k1_verify_batch
    p = [a.ctypes.data for a in (msgs, moff, sigs, soff, keys)]

    def host_prep():
        host.sbvh_make_tuples_ecdsa(*p, n, tuples.ctypes.data)

    def tuple_call():
        sbv._check(tuple_entry(tuples.ctypes.data, n, bm_a.ctypes.data))
        return sbv.last_timing().prep_us

    def msgs_call():
        sbv._check(entry(*p, n, bm_b.ctypes.data))
        return sbv.last_timing().prep_us

    info = sbv.ShardInfo()

    def sharded_call():
        sbv._check(lib.sbv_p256_verify_msgs_sharded(*p, n, 0, 0, bm_d.ctypes.data, None, ctypes.byref(info)))
        return info.kernels_us

    # correctness first: every bitmap equals the tuple route's, which accepts exactly the unspoiled requests
    host_prep(); tuple_call(); msgs_call()
    want = np.packbits((np.arange(n) % 8 != 7).astype(np.uint8), bitorder="little")
    assert bm_a.tobytes() == want.tobytes(), "the tuple route does not accept exactly the unspoiled requests"
    assert bm_b.tobytes() == bm_a.tobytes(), "the raw-message entry disagrees with the tuple route"
    if curve == "p256":
        sharded_call()
        assert bm_d.tobytes() == bm_a.tobytes(), "the sharded raw-message entry disagrees with the tuple route"
    for _ in range(SETTLE.pop(curve, 0)):
        tuple_call()
    prep_us, _ = timed(host_prep, 1, args.steps)
    call_us, tuple_prep = timed(tuple_call, args.warm, args.steps)
    msgs_us, msgs_prep = timed(msgs_call, args.warm, args.steps)
    out = {"curve": curve, "n": n, "message_bytes": size, "signers": nk, "unique_signatures": uniq,
           "a_host_prep_us": summary(prep_us), "a_tuple_call_us": summary(call_us),
           "a_total_us": summary([x + y for x, y in zip(prep_us, call_us)]), "b_msgs_call_us": summary(msgs_us),
           "c_prep_us_msgs": summary(msgs_prep), "c_prep_us_tuples": summary(tuple_prep),
           "c_front_end_us": round(statistics.median(msgs_prep) - statistics.median(tuple_prep), 1),
           "b_M_per_s": round(n / statistics.median(msgs_us), 1),
           "a_M_per_s": round(n / (statistics.median(prep_us) + statistics.median(call_us)), 1)}
    if curve == "p256":
        shard_us, shard_kern = timed(sharded_call, args.warm, args.steps)
        out.update(d_sharded_call_us=summary(shard_us), d_kernels_us=summary(shard_kern), d_M_per_s=round(n / statistics.median(shard_us), 1))
    print(json.dumps(out), flush=True)


SETTLE = {curve: args.settle for curve in args.curves.split(",")}
for curve in args.curves.split(","):
    priv = private_keys(curve)
    pubs = public_keys(curve, priv)
    for size in (int(x) for x in args.sizes.split(",")):
        run(curve, size, priv, pubs)
