#!/usr/bin/env python3
"""secp256k1 batch signing on one MI355X: signatures/s through sbv_secp256k1_sign_batch_stream (device-resident buffers) and through
the host-pointer entry sbv_secp256k1_sign_batch, public keys/s through sbv_secp256k1_pubkeys_stream at n_keys and at n keys, read
against the host signer (consensus_amd/host: k256_sign_rfc6979, one thread and 16) and the P-256 device signer on the same machine.
Workload: 2^18 digests, 1 024 keys; 3 warm calls and 10 timed ones, median and spread (min .. max).  One JSON line.

    python tools/bench_secp256k1_sign.py [n] [n_keys]"""
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
import numpy as np  # noqa: E402

import consensus_amd as sbv  # noqa: E402

WARM, TIMED = 3, 10
ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def _spread(times, n, unit="signatures_per_s"):
    med = statistics.median(times)
    return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times), unit: n / med}


def _timed(fn, sync, warm=WARM, timed=TIMED):
    out = []
    for rep in range(warm + timed):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep >= warm:
            out.append(time.perf_counter() - t0)
    return out


def workload(n, n_keys):
    keys = b"".join((int.from_bytes(hashlib.sha256(b"bench-k256-sign%d" % i).digest(), "big") % (ORDER - 1) + 1).to_bytes(32, "big")
                    for i in range(max(n_keys, 1)))
    digests = np.random.default_rng(0x256C1).integers(0, 256, 32 * n, dtype=np.uint8)
    return keys, digests


def device_rates(n=1 << 18, n_keys=1024, warm=WARM, timed=TIMED):
    """-> dict: the stream form, the host-pointer form, public keys at n_keys and at n, and the signatures with their ok bytes"""
    import torch
    keys, digests = workload(n, n_keys)
    many = np.frombuffer(b"".join(hashlib.sha256(b"bench-k256-pub%d" % i).digest() for i in range(n)), dtype=np.uint8)    # below n but for ~2^-128
    d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
    d_many = torch.from_numpy(many.copy()).cuda()
    d_dig = torch.from_numpy(digests).cuda()
    d_sig = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    d_rid, d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_pub, d_pok = torch.empty(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    torch.cuda.synchronize()
    t_sign = _timed(lambda: sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_sig.data_ptr(), d_rid.data_ptr(),
                                                            d_ok.data_ptr(), low_s=True, stream=sp), torch.cuda.synchronize, warm, timed)
    t_pub_few = _timed(lambda: sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), n_keys, d_pub.data_ptr(), d_pok.data_ptr(), sp),
                       torch.cuda.synchronize, warm, timed)
    few_ok = bool(d_pok[:n_keys].all().item())
    t_pub_many = _timed(lambda: sbv.secp256k1_pubkeys_stream(d_many.data_ptr(), n, d_pub.data_ptr(), d_pok.data_ptr(), sp),
                        torch.cuda.synchronize, warm, timed)
    lib = sbv.load()
    lib.sbv_secp256k1_sign_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    h_keys = np.frombuffer(keys, dtype=np.uint8).copy()
    h_sig, h_rid, h_ok = np.zeros(64 * n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

    def host_form():
        rc = lib.sbv_secp256k1_sign_batch(h_keys.ctypes.data, n_keys, None, digests.ctypes.data, n, 1, h_sig.ctypes.data, h_rid.ctypes.data,
                                          h_ok.ctypes.data)
        assert rc == 0, rc
    t_host = _timed(host_form, lambda: None, warm, timed)
    sigs = d_sig.cpu().numpy()
    return {"n": n, "n_keys": n_keys, "flags": "SBV_K256_SIGN_LOW_S",
            "stream_form": _spread(t_sign, n), "host_pointer_form": _spread(t_host, n),
            "pubkeys_stream_n_keys": _spread(t_pub_few, n_keys, "keys_per_s"), "pubkeys_stream_n": _spread(t_pub_many, n, "keys_per_s"),
            "ok_all_ones": bool(d_ok.all().item()) and bool(h_ok.all()) and few_ok and bool(d_pok.all().item()),
            "forms_agree": bool((sigs == h_sig).all()) and bool((d_rid.cpu().numpy() == h_rid).all()),
            "_sigs": sigs, "_keys": keys, "_digests": digests}


def cpu_rates(keys, digests, n_keys, count=1 << 13, threads=16):
    """the host signer (k256_sign_rfc6979 behind sbvh_k256_sign_rfc6979) on `count` of the digests: one thread, then `threads`; raw
    RFC 6979 signatures (no low-S rule)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostlib
    h = hostlib.load()
    h.sbvh_k256_sign_rfc6979.argtypes = [ctypes.c_char_p] * 3
    blob = digests.tobytes()
    sigs = [None] * count

    def work(lo, hi):
        out = ctypes.create_string_buffer(64)
        for i in range(lo, hi):
            k = i % n_keys
            h.sbvh_k256_sign_rfc6979(keys[32 * k:32 * k + 32], blob[32 * i:32 * i + 32], out)
            sigs[i] = out.raw
    work(0, 8)                                       # builds the host comb
    t0 = time.perf_counter()
    work(0, count // 8)
    one = (count // 8) / (time.perf_counter() - t0)
    step = (count + threads - 1) // threads
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda t: work(t * step, min(count, (t + 1) * step)), range(threads)))
        many = count / (time.perf_counter() - t0)
    return one, many, sigs


def p256_rate(n, n_keys, warm=WARM, timed=TIMED):
    import torch
    order = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
    rng = np.random.default_rng(7)
    keys = b"".join(int.to_bytes(int.from_bytes(rng.bytes(32), "big") % (order - 1) + 1, 32, "big") for _ in range(n_keys))
    d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
    d_dig = torch.from_numpy(np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy()).cuda()
    d_sig, d_ok = torch.empty(64 * n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    t = _timed(lambda: sbv.sign_batch_dev(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_sig.data_ptr(), d_ok.data_ptr(), st.cuda_stream),
               torch.cuda.synchronize, warm, timed)
    return _spread(t, n)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    sbv.init(0)
    r = device_rates(n, n_keys)
    sigs, keys, digests = r.pop("_sigs"), r.pop("_keys"), r.pop("_digests")
    count = min(n, 1 << 13)
    one, many, host_sigs = cpu_rates(keys, digests, n_keys, count)
    half = (ORDER - 1) // 2

    def low(rs):
        s = int.from_bytes(rs[32:], "big")
        return rs[:32] + (ORDER - s if s > half else s).to_bytes(32, "big")
    r["device_equals_host_signer"] = all(sigs[64 * i:64 * i + 64].tobytes() == low(host_sigs[i]) for i in range(count))
    r["host_signer"] = {"one_thread_signatures_per_s": one, "sixteen_threads_signatures_per_s": many, "digests": count,
                        "note": "16 Python threads around a C call that releases the interpreter lock"}
    r["p256_device_signer"] = p256_rate(n, n_keys)
    r["stream_form_over_16_host_threads"] = r["stream_form"]["signatures_per_s"] / many
    r["stream_form_over_p256_device_signer"] = r["stream_form"]["signatures_per_s"] / r["p256_device_signer"]["signatures_per_s"]
    r["metric"] = "secp256k1 signatures/s, device-resident, batch=%d" % n
    r["value"] = r["stream_form"]["signatures_per_s"]
    r["unit"] = "signatures/s"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
