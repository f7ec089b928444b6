#!/usr/bin/env python3
"""SEC1 public keys on one MI355X (include/sbv.h: sbv_p256_decode_keys, sbv_secp256k1_decode_keys, their _stream forms and the _sec1
verify entries), one process, every yardstick measured beside the figure it is read against.  One JSON line per leg.

Workload: --n keys / items (default 2^18) under --signers signers (default 1 024), the keys compressed (the 33-byte stride), every 8th
request spoiled.  Every output is compared before anything is timed.  --warm warm calls and --steps timed ones per leg (3 and 10):
median with min .. max.  Per curve --settle untimed verify_msgs calls first (the generic step's hot keys settle).
  decode   per curve: decode_keys_stream on device-resident buffers; for secp256k1 beside sbv_secp256k1_schnorr_lift_keys_stream on the
           same x-coordinates (the same square root: the decode should sit inside that yardstick's own call-to-call range); the
           host-pointer decode_keys; the host forms (consensus_amd/host: the same lane code under g++) on 1 thread (--n1 keys) and on 16
  verify   per curve and message size (64 / 200 / 1 024 bytes): verify_msgs_sec1 against (a) verify_msgs on pre-decoded keys — the
           difference is the price of decoding — and (b) the route it replaces: host decode on 16 threads, then verify_msgs.  The
           entry ships if at no size it is slower than (b) by more than (b)'s own spread.
All host buffers are pageable memory.
Usage: bench_sec1.py [--n N] [--n1 N1] [--signers K] [--sizes 64,200,1024] [--warm 3] [--steps 10] [--curves p256,k256]"""
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
ap.add_argument("--n", type=int, default=1 << 18)
ap.add_argument("--n1", type=int, default=1 << 13, help="keys of the one-thread host leg")
ap.add_argument("--signers", type=int, default=1024)
ap.add_argument("--sizes", default="64,200,1024")
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--curves", default="p256,k256")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--settle", type=int, default=48, help="untimed verify_msgs calls per curve before its first leg: the generic step's hot keys settle (16 calls to count, 16 to promote)")
args = ap.parse_args()
n, nk = args.n, args.signers
assert n <= 1 << 21 and n % nk == 0

sbv.init(0)
import torch  # noqa: E402

lib, host = sbv.load(), hostlib.load()
C, V, S = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t
for name in ("sbv_p256_verify_msgs", "sbv_secp256k1_verify_msgs"):
    getattr(lib, name).argtypes = [V, V, V, V, V, S, V]
for name in ("sbv_p256_verify_msgs_sec1", "sbv_secp256k1_verify_msgs_sec1"):
    getattr(lib, name).argtypes = [V, V, V, V, V, V, S, V]
for name in ("sbv_p256_decode_keys", "sbv_secp256k1_decode_keys"):
    getattr(lib, name).argtypes = [V, V, S, V, V]
host.sbvh_pubkey.argtypes = [C, C]
host.sbvh_sec1_decode_batch.argtypes = [ctypes.c_int, V, V, S, V, V, ctypes.c_int]
host.sbvh_sec1_decode_batch.restype = None
NAME = {"p256": "p256", "k256": "secp256k1"}
ORDER = {"p256": p256_py.N, "k256": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141}


def summary(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def timed(fn, sync=lambda: None, warm=None, steps=None):
    """wall-clock microseconds of `steps` calls after `warm` untimed ones"""
    us = []
    warm, steps = args.warm if warm is None else warm, args.steps if steps is None else steps
    for rep in range(warm + steps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep >= warm:
            us.append(1e6 * (time.perf_counter() - t0))
    return us


def signers(curve):
    priv = b"".join((int.from_bytes(hashlib.sha256(b"bench_sec1 %s %d" % (curve.encode(), i)).digest(), "big") % (ORDER[curve] - 1) + 1).to_bytes(32, "big")
                    for i in range(nk))
    if curve == "k256":
        pubs, ok = sbv.secp256k1_pubkeys(priv)
        assert ok == b"\x01" * nk
    else:
        pubs = b""
        for i in range(nk):
            q = ctypes.create_string_buffer(64)
            assert host.sbvh_pubkey(priv[32 * i:32 * i + 32], q) == 0
            pubs += q.raw
    pk = np.frombuffer(pubs, dtype=np.uint8).reshape(nk, 64)
    comp = np.empty((nk, 33), dtype=np.uint8)
    comp[:, 0] = 2 + (pk[:, 63] & 1)
    comp[:, 1:] = pk[:, :32]
    return priv, pk, comp


def decode_legs(curve, pk, comp):
    cid = 0 if curve == "p256" else 1
    idx = np.arange(n) % nk
    keys33 = np.ascontiguousarray(comp[idx])                       # n x 33: the stride form
    want = np.ascontiguousarray(pk[idx])
    d_k, d_64, d_ok = torch.from_numpy(keys33.reshape(-1)).cuda(), torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    sync = torch.cuda.synchronize
    stream_fn = sbv.p256_decode_keys_stream if curve == "p256" else sbv.secp256k1_decode_keys_stream

    def dev():
        stream_fn(d_k.data_ptr(), 0, 33 * n, n, d_64.data_ptr(), d_ok.data_ptr(), st.cuda_stream)
    sync()
    dev()
    sync()
    assert d_64.cpu().numpy().tobytes() == want.tobytes() and bool(d_ok.all().item()), "decode_keys_stream: a key differs"
    out = {"leg": "decode", "curve": curve, "n": n, "signers": nk}
    t_dev = timed(dev, sync)
    out["decode_keys_stream_us"] = summary(t_dev)
    out["decode_keys_stream_M_keys_per_s"] = round(n / statistics.median(t_dev), 1)
    if curve == "k256":
        d_x = torch.from_numpy(np.ascontiguousarray(pk[idx][:, :32]).reshape(-1)).cuda()
        d_l64, d_lok = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")

        def lift():
            sbv.secp256k1_schnorr_lift_keys_stream(d_x.data_ptr(), n, d_l64.data_ptr(), d_lok.data_ptr(), st.cuda_stream)
        sync()
        lift()
        sync()
        assert bool(d_lok.all().item()) and torch.equal(d_l64.view(n, 64)[:, :32], d_64.view(n, 64)[:, :32])
        t_lift = timed(lift, sync)
        t_dev2 = timed(dev, sync)
        out["yardstick_schnorr_lift_keys_stream_us"] = summary(t_lift)
        out["decode_keys_stream_again_us"] = summary(t_dev2)
        out["decode_inside_the_lift_range"] = bool(min(t_lift) <= statistics.median(t_dev) <= max(t_lift))
    # host pointers
    h64, hok = np.zeros(64 * n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    fn = getattr(lib, "sbv_%s_decode_keys" % NAME[curve])

    def hostptr():
        sbv._check(fn(keys33.ctypes.data, None, n, h64.ctypes.data, hok.ctypes.data))
    hostptr()
    assert h64.tobytes() == want.tobytes() and bool(hok.all())
    out["decode_keys_host_pointers_us"] = summary(timed(hostptr))
    # the host forms
    n1 = min(args.n1, n)
    for threads, m, warm, steps in ((1, n1, 1, 3), (args.threads, n, 1, args.steps)):
        h64[:] = 0

        def cpu():
            host.sbvh_sec1_decode_batch(cid, keys33.ctypes.data, None, m, h64.ctypes.data, hok.ctypes.data, threads)
        cpu()
        assert h64[:64 * m].tobytes() == want[:m].tobytes()
        t = timed(cpu, warm=warm, steps=steps)
        out["host_form_%d_threads_us" % threads] = dict(summary(t), keys=m, k_keys_per_s=round(1e3 * m / statistics.median(t), 1))
    print(json.dumps(out), flush=True)
    return keys33, want


def verify_legs(curve, size, priv, keys33, keys64):
    cid = 0 if curve == "p256" else 1
    rng = np.random.default_rng(size + 11 * cid)
    msgs = rng.integers(0, 256, (n, size), dtype=np.uint8)
    moff = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
    sign = sbv.p256_sign_msgs if curve == "p256" else sbv.secp256k1_sign_msgs
    res = sign(priv, msgs.tobytes(), offsets=[int(x) for x in moff])
    sig_blob, soff_l, ok = res[0], res[1], res[-1]
    assert ok == b"\x01" * n
    sigs, soff = np.frombuffer(sig_blob, dtype=np.uint8).copy(), np.array(soff_l, dtype=np.uint64)
    msgs[7::8, size // 2] ^= 1                                      # every 8th request spoiled
    bm = [np.zeros((n + 7) // 8, dtype=np.uint8) for _ in range(3)]
    dec = np.zeros((n, 64), dtype=np.uint8)
    entry = getattr(lib, "sbv_%s_verify_msgs" % NAME[curve])
    sec1 = getattr(lib, "sbv_%s_verify_msgs_sec1" % NAME[curve])
    head = [a.ctypes.data for a in (msgs, moff, sigs, soff)]

    def a_predecoded():
        sbv._check(entry(*head, keys64.ctypes.data, n, bm[0].ctypes.data))

    def b_host_decode_then_verify():
        host.sbvh_sec1_decode_batch(cid, keys33.ctypes.data, None, n, dec.ctypes.data, None, args.threads)
        sbv._check(entry(*head, dec.ctypes.data, n, bm[1].ctypes.data))

    def c_sec1():
        sbv._check(sec1(*head, keys33.ctypes.data, None, n, bm[2].ctypes.data))
    a_predecoded(); b_host_decode_then_verify(); c_sec1()
    want = np.packbits((np.arange(n) % 8 != 7).astype(np.uint8), bitorder="little")
    assert bm[0].tobytes() == want.tobytes(), "verify_msgs does not accept exactly the unspoiled requests"
    assert bm[1].tobytes() == want.tobytes() and bm[2].tobytes() == want.tobytes(), "a route disagrees with verify_msgs on pre-decoded keys"
    for _ in range(SETTLE.pop(curve, 0)):
        a_predecoded()                                              # a promoting step takes several times a settled one: keep them out of every leg
    ta, tc, tb = timed(a_predecoded), timed(c_sec1), timed(b_host_decode_then_verify)
    ta2 = timed(a_predecoded)
    spread_b = max(tb) - min(tb)
    out = {"leg": "verify", "curve": curve, "n": n, "message_bytes": size, "signers": nk,
           "a_verify_msgs_predecoded_us": summary(ta), "a_again_us": summary(ta2), "b_host_decode_16_threads_then_verify_msgs_us": summary(tb),
           "verify_msgs_sec1_us": summary(tc), "price_of_decoding_us": round(statistics.median(tc) - statistics.median(ta), 1),
           "sec1_M_per_s": round(n / statistics.median(tc), 1), "b_M_per_s": round(n / statistics.median(tb), 1),
           "ships": bool(statistics.median(tc) <= statistics.median(tb) + spread_b)}
    print(json.dumps(out), flush=True)


SETTLE = {curve: args.settle for curve in args.curves.split(",")}
for curve in args.curves.split(","):
    priv, pk, comp = signers(curve)
    keys33, keys64 = decode_legs(curve, pk, comp)
    for size in (int(x) for x in args.sizes.split(",")):
        verify_legs(curve, size, priv, keys33, keys64)
