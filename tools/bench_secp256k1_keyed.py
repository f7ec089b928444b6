#!/usr/bin/env python3
"""Registered secp256k1 keys (include/sbv.h: sbv_secp256k1_register_keys) against the generic secp256k1 entry, one MI355X.  One JSON line.

On one seeded set of 2^20 signatures over 16 keys (every 8th with a bit of r | s | hash flipped):
  keyed_narrow / keyed_wide    sbv_secp256k1_verify_batch_keyed_dev on device-resident records, 8-bit combs and then after widen_keys;
  generic_cold / generic_warm  sbv_secp256k1_verify_batch_dev on the same signatures as 160-byte tuples, with the curve's key-table
                               cache off (every step builds every comb) and on once it holds the keys;
  burst                        the N = 16 commit quorum: 15 signatures through sbv_secp256k1_verify_batch_keyed and through
                               sbv_secp256k1_verify_batch, p50 / p99 of the host-side call time over `--calls` calls.
Steps are timed with device events around each call; the figures are medians.  Usage: bench_secp256k1_keyed.py [--steps K] [--calls C]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import consensus_amd as sbv  # noqa: E402
import hostlib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=16)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--calls", type=int, default=1000)
ap.add_argument("--settle", type=int, default=3, help="generic steps before the warm figure (the key-table cache fills in the first)")
args = ap.parse_args()
n, nk = args.n, args.keys

sbv.init(0)
h = hostlib.load()
V = ctypes.c_void_p
h.sbvh_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, V, V, ctypes.c_int]
tuples = np.zeros(n * 160, dtype=np.uint8)
expect = np.zeros((n + 7) // 8, dtype=np.uint8)
h.sbvh_k256_gen_batch(0x6B5EED, n, nk, 0, tuples.ctypes.data, expect.ctypes.data, min(16, os.cpu_count() or 1))
t = tuples.reshape(n, 160)
idx = np.arange(7, n, 8)
t[idx, (idx * 7919) % 96] ^= (1 << (idx % 8)).astype(np.uint8)
ukeys, inv = np.unique(t[:, 96:], axis=0, return_inverse=True)
assert len(ukeys) == nk
recs = np.ascontiguousarray(t[:, :96])
sbv.secp256k1_clear_keys()
t0 = time.perf_counter()
slots_of_key = sbv.secp256k1_register_keys([k.tobytes() for k in ukeys])
register_s = time.perf_counter() - t0
slots = np.array(slots_of_key, dtype=np.uint32)[inv.reshape(-1)]

stream = torch.cuda.current_stream()
d_t = torch.from_numpy(tuples).cuda()
d_r = torch.from_numpy(recs.reshape(-1)).cuda()
d_s = torch.from_numpy(slots.view(np.int32)).cuda()
d_b = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")


def timed(fn, steps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), d_b.cpu().numpy().tobytes()


def keyed():
    sbv.secp256k1_verify_batch_keyed_dev(d_r.data_ptr(), d_s.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)


def generic():
    sbv.secp256k1_verify_batch_dev(d_t.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)


out = {"tool": "bench_secp256k1_keyed", "n": n, "keys": nk, "steps": args.steps, "register_s": round(register_s, 3)}
res = {}
out["keyed_narrow_ms"], res["narrow"] = timed(keyed, args.steps)
t0 = time.perf_counter()
sbv.secp256k1_widen_keys(slots_of_key)
out["widen_s"] = round(time.perf_counter() - t0, 3)
out["wide_slots"] = sbv.secp256k1_wide_key_stats()[0]
out["keyed_wide_ms"], res["wide"] = timed(keyed, args.steps)
K = sbv.SCHEME_SECP256K1
sbv.key_cache(False, 0, K)
out["generic_cold_ms"], res["cold"] = timed(generic, args.steps)
sbv.key_cache(True, 1024, K)
out["generic_warm_ms"], res["warm"] = timed(generic, args.steps, warmup=args.settle)
out["key_cache_stats"] = list(sbv.key_cache_stats(K))
for k in ("keyed_narrow_ms", "keyed_wide_ms", "generic_cold_ms", "generic_warm_ms"):
    out[k.replace("_ms", "_Mps")] = round(n / (out[k] * 1e3), 1)
    out[k] = round(out[k], 3)
out["verdicts_equal"] = len(set(res.values())) == 1
out["accepted"] = int(sum(bin(b).count("1") for b in res["narrow"]))

# the commit quorum at N = 16: 15 votes by 15 consenters
lib = sbv.load()
lib.sbv_secp256k1_verify_batch_keyed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
lib.sbv_secp256k1_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
q = 15
b_recs = np.ascontiguousarray(recs[:q]).reshape(-1)
b_slots = np.ascontiguousarray(slots[:q])
b_tup = np.ascontiguousarray(t[:q]).reshape(-1)
bm_k, bm_g = ctypes.create_string_buffer(2), ctypes.create_string_buffer(2)


def lat(call):
    for _ in range(20):
        call()
    us = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        call()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.percentile(us, 50)), 1), round(float(np.percentile(us, 99)), 1)


out["burst_keyed_wide_p50_us"], out["burst_keyed_wide_p99_us"] = lat(lambda: sbv._check(lib.sbv_secp256k1_verify_batch_keyed(b_recs.ctypes.data, b_slots.ctypes.data, q, bm_k)))
sbv.secp256k1_wide_keys(0)
sbv.secp256k1_wide_keys(64)
out["burst_keyed_narrow_p50_us"], out["burst_keyed_narrow_p99_us"] = lat(lambda: sbv._check(lib.sbv_secp256k1_verify_batch_keyed(b_recs.ctypes.data, b_slots.ctypes.data, q, bm_k)))
out["burst_generic_p50_us"], out["burst_generic_p99_us"] = lat(lambda: sbv._check(lib.sbv_secp256k1_verify_batch(b_tup.ctypes.data, q, bm_g)))
out["burst_verdicts_equal"] = bm_k.raw == bm_g.raw
sbv.secp256k1_clear_keys()
print(json.dumps(out))
