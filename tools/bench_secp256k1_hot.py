#!/usr/bin/env python3
"""secp256k1 hot keys (include/sbv.h: sbv_secp256k1_hot_keys) inside the generic grouped step, one MI355X, one process.  One JSON line
per signer count.

On a seeded set of 2^20 signatures (every 8th with a bit of r | s | hash flipped) over 16, 1 024 and 2 048 keys, through
sbv_secp256k1_verify_batch_dev on device-resident tuples:
  cold      the curve's key-table cache off: every step builds every comb;
  warm      the cache on and holding the keys, the pool off — what the library does by default;
  settled   the pool on (at most 1 024 combs: the 2 048-signer point is the half-hot one) once every comb it can hand out is built and
            the wide pass serves the same number of tuples as in the call before; `calls_until_settled` counts the calls from the
            cold cache to that state;
  promoting the median step while the promoted count was still rising (a batch's promotions are built behind its verdicts: their cost
            shows in the step that follows).
Steps are timed with device events around each call; the figures are medians of `--steps` steps.  Every bitmap is compared with the
generator's.  Usage: bench_secp256k1_hot.py [--steps K] [--keys 16,1024,2048] [--pool 1024]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import consensus_amd as sbv  # noqa: E402
import hostlib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", default="16,1024,2048")
ap.add_argument("--pool", type=int, default=1024)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--settle", type=int, default=3, help="steps before the warm figure (the key-table cache fills in the first)")
ap.add_argument("--max-calls", type=int, default=96, help="calls the pool may take to settle")
args = ap.parse_args()
n = args.n

sbv.init(0)
h = hostlib.load()
V = ctypes.c_void_p
h.sbvh_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, V, V, ctypes.c_int]
K = sbv.SCHEME_SECP256K1
stream = torch.cuda.current_stream()
d_b = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")


def step(d_t):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    sbv.secp256k1_verify_batch_dev(d_t.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def timed(d_t, want, steps, warmup):
    for _ in range(warmup):
        step(d_t)
    ms = [step(d_t) for _ in range(steps)]
    return float(np.median(ms)), d_b.cpu().numpy().tobytes() == want


for nk in [int(x) for x in args.keys.split(",")]:
    tuples = np.zeros(n * 160, dtype=np.uint8)
    expect = np.zeros((n + 7) // 8, dtype=np.uint8)
    h.sbvh_k256_gen_batch(0x6B5EED + nk, n, nk, 0, tuples.ctypes.data, expect.ctypes.data, min(16, os.cpu_count() or 1))
    t = tuples.reshape(n, 160)
    idx = np.arange(7, n, 8)
    t[idx, (idx * 7919) % 96] ^= (1 << (idx % 8)).astype(np.uint8)
    expect[idx >> 3] &= ~(1 << (idx & 7)).astype(np.uint8)            # the generator's bitmap with the corrupted tuples rejected
    want = expect.tobytes()
    d_t = torch.from_numpy(tuples).cuda()
    pool = min(nk, args.pool)
    out = {"tool": "bench_secp256k1_hot", "n": n, "keys": nk, "pool_asked": pool, "steps": args.steps}
    ok = {}
    sbv.k256_hot_keys(0, 0)
    sbv.key_cache(False, 0, K)
    out["cold_ms"], ok["cold"] = timed(d_t, want, args.steps, 1)
    sbv.key_cache(True, 4096, K)
    out["warm_pool_off_ms"], ok["warm"] = timed(d_t, want, args.steps, args.settle)
    out["key_cache_stats"] = list(sbv.key_cache_stats(K))
    sbv.k256_hot_keys(pool, 0)                                         # another pool size: the scheme's cache starts cold again
    calls, rising, prev, settled = 0, [], (-1, -1), False
    while calls < args.max_calls and not settled:
        ms = step(d_t)
        calls += 1
        ok["call%d" % calls] = d_b.cpu().numpy().tobytes() == want
        promoted, cap, wide, min_hits = sbv.k256_hot_key_stats()
        if prev[0] >= 0 and promoted > prev[0]:
            rising.append(ms)
        settled = cap > 0 and promoted == min(cap, nk) and wide == prev[1] and wide > 0
        prev = (promoted, wide)
    out["pool"], out["min_hits"], out["promoted"], out["wide_tuples"] = cap, min_hits, promoted, wide
    out["settled"], out["calls_until_settled"] = settled, calls
    out["promoting_ms"] = round(float(np.median(rising)), 3) if rising else None
    out["settled_pool_on_ms"], ok["settled"] = timed(d_t, want, args.steps, 0)
    out["promoted_after"], _, out["wide_tuples_after"], _ = sbv.k256_hot_key_stats()
    for k in ("cold_ms", "warm_pool_off_ms", "settled_pool_on_ms"):
        out[k.replace("_ms", "_Mps")] = round(n / (out[k] * 1e3), 1)
        out[k] = round(out[k], 3)
    out["settled_over_warm"] = round(out["settled_pool_on_ms"] / out["warm_pool_off_ms"], 3)
    out["bitmaps_equal_generator"] = all(ok.values())
    print(json.dumps(out), flush=True)
    del d_t
sbv.k256_hot_keys(0, 0)
sbv.key_cache(True, 1024, K)
