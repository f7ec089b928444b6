#!/usr/bin/env python3
"""Registered Ed25519 keys (include/sbv.h: sbv_ed25519_register_keys) against the generic Ed25519 entry, one MI355X.  One JSON line.

On one seeded set of 2^20 signatures over 16 keys (every 8th with a bit of R | S flipped):
  keyed_narrow / keyed_wide   sbv_ed25519_verify_batch_keyed_dev on device-resident records, 8-bit combs and then after widen_keys;
  generic_cold / generic_hot  sbv_ed25519_verify_batch_dev on the same signatures as 128-byte tuples, with the scheme's key-table cache
                              off (every step builds every comb) and on after the hot-key pool has settled;
  burst                       the N = 16 commit quorum: 15 signatures through sbv_ed25519_verify_batch_keyed and through
                              sbv_ed25519_verify_batch, p50 / p99 of the host-side call time over `--calls` calls.
Steps are timed with device events around each call; the figures are medians.  Usage: bench_ed25519_keyed.py [--steps K] [--calls C]"""
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
ap.add_argument("--settle", type=int, default=24, help="generic steps before the hot figure (hot-key pool promotion)")
args = ap.parse_args()
n, nk = args.n, args.keys

sbv.init(0)
h = hostlib.load()
tuples = np.zeros(n * 128, dtype=np.uint8)
expect = np.zeros((n + 7) // 8, dtype=np.uint8)
h.sbvh_ed25519_gen_batch(0xED5EED, n, nk, 0, tuples.ctypes.data, expect.ctypes.data, min(16, os.cpu_count() or 1))
t = tuples.reshape(n, 128)
idx = np.arange(7, n, 8)
t[idx, (idx * 7919) % 64] ^= (1 << (idx % 8)).astype(np.uint8)
encs = [t[i, 64:96].tobytes() for i in range(nk)]                  # tuple i is signed by key i % nk
recs = np.ascontiguousarray(np.concatenate([t[:, :64], t[:, 96:]], axis=1))
sbv.ed25519_clear_keys()
slots_of_key = sbv.ed25519_register_keys(encs)
slots = np.array([slots_of_key[i % nk] for i in range(n)], dtype=np.uint32)

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
    sbv.ed25519_verify_batch_keyed_dev(d_r.data_ptr(), d_s.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)


def generic():
    sbv.ed25519_verify_batch_dev(d_t.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)


out = {"tool": "bench_ed25519_keyed", "n": n, "keys": nk, "steps": args.steps}
res = {}
out["keyed_narrow_ms"], res["narrow"] = timed(keyed, args.steps)
t0 = time.perf_counter()
sbv.ed25519_widen_keys(slots_of_key)
out["widen_s"] = round(time.perf_counter() - t0, 3)
out["wide_slots"] = sbv.ed25519_wide_key_stats()[0]
out["keyed_wide_ms"], res["wide"] = timed(keyed, args.steps)
sbv.key_cache(False, 0, sbv.SCHEME_ED25519)
out["generic_cold_ms"], res["cold"] = timed(generic, args.steps)
sbv.key_cache(True, 0, sbv.SCHEME_ED25519)
out["generic_hot_ms"], res["hot"] = timed(generic, args.steps, warmup=args.settle)
out["ed_hot_key_stats"] = list(sbv.ed_hot_key_stats())
for k in ("keyed_narrow_ms", "keyed_wide_ms", "generic_cold_ms", "generic_hot_ms"):
    out[k.replace("_ms", "_Mps")] = round(n / (out[k] * 1e3), 1)
    out[k] = round(out[k], 3)
out["verdicts_equal"] = len(set(res.values())) == 1
out["accepted"] = int(sum(bin(b).count("1") for b in res["narrow"]))

# the commit quorum at N = 16: 15 votes by 15 consenters
lib = sbv.load()
lib.sbv_ed25519_verify_batch_keyed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
lib.sbv_ed25519_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
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


out["burst_keyed_p50_us"], out["burst_keyed_p99_us"] = lat(lambda: sbv._check(lib.sbv_ed25519_verify_batch_keyed(b_recs.ctypes.data, b_slots.ctypes.data, q, bm_k)))
out["burst_generic_p50_us"], out["burst_generic_p99_us"] = lat(lambda: sbv._check(lib.sbv_ed25519_verify_batch(b_tup.ctypes.data, q, bm_g)))
out["burst_verdicts_equal"] = bm_k.raw == bm_g.raw
sbv.ed25519_clear_keys()
print(json.dumps(out))
