#!/usr/bin/env python3
"""Raw-message ECDSA signing on one MI355X (include/sbv.h: sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs), one process, 3 warm calls and
10 timed ones per figure, medians with ranges.  One JSON line.

1. Per curve and message size (64 / 200 / 1 024 bytes; 2^18 messages, 1 024 keys): the host-pointer entry and its _stream form against
   the host route it replaces — sbv_sha256_batch on 16 CPU threads, the sign_batch entry, DER item by item on the host — with the
   sign_batch_dev / _stream call alone as the floor.  Every signature of the entry is compared with the host route's before timing.
2. The loader: k_sha256_msgs built on sha256_msg_words and on sha256_msg (tools/shaloader.hip), alternating in the same run at the
   three sizes, with the arithmetic floor from compressions per message.

    python tools/bench_ecdsa_sign_msgs.py [n] [n_keys]"""
import concurrent.futures
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import consensus_amd as sbv  # noqa: E402

WARM, TIMED, THREADS = 3, 10, 16
SIZES = (64, 200, 1024)
ORDERS = {"p256": 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551,
          "k256": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141}
V, S, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32


def _spread(times, n=None):
    med = statistics.median(times)
    out = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times)}
    if n:
        out["per_s"] = n / med
    return out


def _timed(fn, sync=lambda: None):
    out = []
    for rep in range(WARM + TIMED):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep >= WARM:
            out.append(time.perf_counter() - t0)
    return out


def entry_against_host_route(curve, size, n, n_keys, host):
    import torch
    lib = sbv.load()
    rng = np.random.default_rng(size + len(curve))
    keys = np.frombuffer(b"".join((int.from_bytes(hashlib.sha256(b"bench-sign-msgs %s %d" % (curve.encode(), i)).digest(), "big") % (ORDERS[curve] - 1) + 1)
                                  .to_bytes(32, "big") for i in range(n_keys)), dtype=np.uint8).copy()
    msgs = rng.integers(0, 256, size * n, dtype=np.uint8)
    moff = np.arange(n + 1, dtype=np.uint64) * size
    sigs, soff, ok, rid = np.zeros(72 * n, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data                                                                  # noqa: E731
    if curve == "p256":
        lib.sbv_p256_sign_msgs.argtypes = [V, U32, V, V, V, S, U32, V, V, V]
        lib.sbv_p256_sign_batch.argtypes = [V, U32, V, V, S, V, V]
        entry = lambda: lib.sbv_p256_sign_msgs(p(keys), n_keys, None, p(msgs), p(moff), n, 0, p(sigs), p(soff), p(ok))          # noqa: E731
        batch = lambda d, o: lib.sbv_p256_sign_batch(p(keys), n_keys, None, p(d), n, p(o), p(ok))                                 # noqa: E731
    else:
        lib.sbv_secp256k1_sign_msgs.argtypes = [V, U32, V, V, V, S, U32, V, V, V, V]
        lib.sbv_secp256k1_sign_batch.argtypes = [V, U32, V, V, S, U32, V, V, V]
        entry = lambda: lib.sbv_secp256k1_sign_msgs(p(keys), n_keys, None, p(msgs), p(moff), n, 0, p(sigs), p(soff), p(rid), p(ok))   # noqa: E731
        batch = lambda d, o: lib.sbv_secp256k1_sign_batch(p(keys), n_keys, None, p(d), n, 0, p(o), p(rid), p(ok))                 # noqa: E731
    lib.sbv_sha256_batch.argtypes = [V, V, S, V]
    host.sbvh_der_encode_batch.argtypes = [V, S, V, V]
    host.sbvh_der_encode_batch.restype = None
    dig, rs = np.zeros(32 * n, dtype=np.uint8), np.zeros(64 * n, dtype=np.uint8)
    hsig, hoff = np.zeros(72 * n, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    step = (n + THREADS - 1) // THREADS
    pool = concurrent.futures.ThreadPoolExecutor(THREADS)

    def sha_part(t):
        lo, hi = t * step, min(n, (t + 1) * step)
        sub = moff[lo:hi + 1] - moff[lo]
        assert lib.sbv_sha256_batch(p(msgs) + int(moff[lo]), p(sub), hi - lo, p(dig) + 32 * lo) == 0

    def host_route():
        list(pool.map(sha_part, range(THREADS)))
        assert batch(dig, rs) == 0
        host.sbvh_der_encode_batch(p(rs), n, p(hsig), p(hoff))

    assert entry() == 0
    host_route()
    same = bool((soff == hoff).all()) and bool((sigs[:int(soff[n])] == hsig[:int(hoff[n])]).all()) and bool(ok.all())
    if not same:
        sys.exit("%s, %d-byte messages: the entry's signatures differ from the host route's: nothing timed" % (curve, size))
    t_entry = _timed(lambda: entry())
    t_route = _timed(host_route)
    t_sha = _timed(lambda: list(pool.map(sha_part, range(THREADS))))
    t_der = _timed(lambda: host.sbvh_der_encode_batch(p(rs), n, p(hsig), p(hoff)))
    pool.shutdown()
    # the _stream form and the floor: device-resident buffers
    dev = lambda a: torch.from_numpy(a).cuda()                                                  # noqa: E731
    d_keys, d_msgs, d_off, d_dig = dev(keys), dev(msgs), dev(moff.view(np.int64)), dev(dig)
    d_rec, d_len, d_rid, d_ok = (torch.empty(k * n, dtype=torch.uint8, device="cuda") for k in (72, 1, 1, 1))
    d_work, d_rs = torch.empty(sbv.ecdsa_sign_msgs_workspace(n), dtype=torch.uint8, device="cuda"), torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.Stream().cuda_stream
    head = (d_keys.data_ptr(), n_keys, 0, d_msgs.data_ptr(), d_off.data_ptr(), n, d_rec.data_ptr(), d_len.data_ptr())
    if curve == "p256":
        stream = lambda: sbv.p256_sign_msgs_stream(*head, d_ok.data_ptr(), d_work.data_ptr(), stream=sp)                           # noqa: E731
        floor = lambda: sbv.sign_batch_dev(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_rs.data_ptr(), d_ok.data_ptr(), sp)  # noqa: E731
    else:
        stream = lambda: sbv.secp256k1_sign_msgs_stream(*head, d_rid.data_ptr(), d_ok.data_ptr(), d_work.data_ptr(), stream=sp)    # noqa: E731
        floor = lambda: sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_rs.data_ptr(), d_rid.data_ptr(),   # noqa: E731
                                                        d_ok.data_ptr(), stream=sp)
    # the _stream form's records, cut to their lengths, are the entry's packed signatures byte for byte: checked before timing
    stream()
    torch.cuda.synchronize()
    lens, recs = d_len.cpu().numpy(), d_rec.cpu().numpy().reshape(n, 72)
    stream_same = bool((np.cumsum(lens.astype(np.uint64)) == soff[1:]).all()) and bool(d_ok.cpu().numpy().all()) and \
        bool((recs[np.arange(72)[None, :] < lens[:, None]] == sigs[:int(soff[n])]).all()) and not recs[np.arange(72)[None, :] >= lens[:, None]].any()
    if not stream_same:
        sys.exit("%s, %d-byte messages: the _stream form's records differ from the entry's signatures: nothing timed" % (curve, size))
    t_stream = _timed(stream, torch.cuda.synchronize)
    t_floor = _timed(floor, torch.cuda.synchronize)
    return {"curve": curve, "message_bytes": size, "n": n, "n_keys": n_keys, "entry_equals_host_route": same, "stream_records_equal": stream_same,
            "entry_host_pointers": _spread(t_entry, n), "entry_stream": _spread(t_stream, n), "host_route": _spread(t_route, n),
            "host_route_sha256_16_threads": _spread(t_sha), "host_route_der": _spread(t_der), "sign_kernel_alone": _spread(t_floor, n)}


def loader(n):
    """k_sha256_msgs on either loader, alternating call by call on the same buffers; unaligned too: the messages start at offset 1"""
    import torch
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), "libsbv_shaloader.so"])      # measurement-only: built on demand
    lb = ctypes.CDLL(os.path.join(ROOT, "tools", "libsbv_shaloader.so"))
    lb.sbvlb_sha256_msgs.argtypes = [ctypes.c_int, V, V, S, ctypes.c_uint64, V, V]
    out = []
    for size in SIZES:
        for shift in (0, 1):
            msgs = np.random.default_rng(size).integers(0, 256, size * n + shift, dtype=np.uint8)
            moff = np.arange(n + 1, dtype=np.uint64) * size + shift
            d_msgs, d_off = torch.from_numpy(msgs).cuda(), torch.from_numpy(moff.view(np.int64)).cuda()
            d_dig = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            want = b"".join(hashlib.sha256(msgs[shift + size * i:shift + size * (i + 1)].tobytes()).digest() for i in range(0, n, max(1, n // 256)))
            for words in (0, 1):                     # both loaders against hashlib on a sample of the lanes, and against each other, before timing
                assert lb.sbvlb_sha256_msgs(words, d_msgs.data_ptr(), d_off.data_ptr(), n, len(msgs), d_dig[words].data_ptr(), None) == 0
            torch.cuda.synchronize()
            got = d_dig[1].cpu().numpy().reshape(n, 32)[::max(1, n // 256)].tobytes()
            if not torch.equal(d_dig[0], d_dig[1]) or got != want:
                sys.exit("%d-byte messages at offset %d: the loaders disagree or differ from hashlib: nothing timed" % (size, shift))
            times = {0: [], 1: []}
            for rep in range(WARM + TIMED):
                for words in (0, 1):
                    torch.cuda.synchronize()
                    a.record()
                    assert lb.sbvlb_sha256_msgs(words, d_msgs.data_ptr(), d_off.data_ptr(), n, len(msgs), d_dig[words].data_ptr(), None) == 0
                    b.record()
                    torch.cuda.synchronize()
                    if rep >= WARM:
                        times[words].append(a.elapsed_time(b) / 1e3)
            agree = bool(torch.equal(d_dig[0], d_dig[1]))
            blocks = (size + 9 + 63) // 64
            out.append({"message_bytes": size, "first_byte_offset": shift, "compressions_per_message": blocks, "loaders_agree": agree,
                        "byte_loader": _spread(times[0], n), "word_loader": _spread(times[1], n),
                        "word_over_byte": statistics.median(times[0]) / statistics.median(times[1]),
                        "byte_loader_spread": (max(times[0]) - min(times[0])) / statistics.median(times[0])})
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    import hostlib
    sbv.init(0)
    host = hostlib.load()
    r = {"entries": [entry_against_host_route(c, size, n, n_keys, host) for c in ("p256", "k256") for size in SIZES], "loader": loader(n)}
    r["metric"] = "raw-message ECDSA signatures/s through the host-pointer entry, P-256, 64-byte messages, batch=%d" % n
    r["value"] = r["entries"][0]["entry_host_pointers"]["per_s"]
    r["unit"] = "signatures/s"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
