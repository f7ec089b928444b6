#!/usr/bin/env python3
"""Ed25519 batch signing on one MI355X: signatures/s through sbv_ed25519_sign_msgs_stream (device-resident buffers) and through the
host-pointer entry sbv_ed25519_sign_msgs, read against the host signer (consensus_amd/host, one thread and 16) and the P-256 device
signer on the same machine.  Workload: 2^18 signatures, 64-byte messages, 1 024 keys; 3 warm calls and 10 timed ones, median and
spread (min .. max).  One JSON line.

    python tools/bench_ed25519_sign.py [n] [n_keys]

tests/test_gpu_ed25519_sign.py imports device_rates() for the rate it prints."""
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

WARM, TIMED, MSG_BYTES = 3, 10, 64


def _spread(times, n):
    med = statistics.median(times)
    return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times), "signatures_per_s": n / med}


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
    seeds = b"".join(hashlib.sha256(b"bench-ed-sign%d" % i).digest() for i in range(n_keys))
    msgs = np.random.default_rng(0xED5161).integers(0, 256, n * MSG_BYTES, dtype=np.uint8)
    offs = np.arange(n + 1, dtype=np.uint64) * MSG_BYTES
    return seeds, msgs, offs


def device_rates(n=1 << 18, n_keys=1024, warm=WARM, timed=TIMED):
    """-> dict: the stream form (expand and sign timed apart), the host-pointer form, and the signatures with their ok bytes"""
    import torch
    seeds, msgs, offs = workload(n, n_keys)
    d_seeds = torch.from_numpy(np.frombuffer(seeds, dtype=np.uint8).copy()).cuda()
    d_msgs = torch.from_numpy(msgs).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_exp = torch.empty(96 * n_keys, dtype=torch.uint8, device="cuda")
    d_pks = torch.empty(32 * n_keys, dtype=torch.uint8, device="cuda")
    d_sig = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    t_exp = _timed(lambda: sbv.ed25519_expand_keys_stream(d_seeds.data_ptr(), n_keys, d_exp.data_ptr(), d_pks.data_ptr(), sp),
                   torch.cuda.synchronize, warm, timed)
    t_sign = _timed(lambda: sbv.ed25519_sign_msgs_stream(d_exp.data_ptr(), n_keys, 0, d_msgs.data_ptr(), d_offs.data_ptr(), n,
                                                         d_sig.data_ptr(), d_ok.data_ptr(), sp), torch.cuda.synchronize, warm, timed)
    lib = sbv.load()
    lib.sbv_ed25519_sign_msgs.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p, ctypes.c_void_p]
    exp = d_exp.cpu().numpy()
    h_sig, h_ok = np.zeros(64 * n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

    def host_form():
        rc = lib.sbv_ed25519_sign_msgs(exp.ctypes.data, n_keys, None, msgs.ctypes.data, offs.ctypes.data, n, h_sig.ctypes.data, h_ok.ctypes.data)
        assert rc == 0, rc
    t_host = _timed(host_form, lambda: None, warm, timed)
    sigs = d_sig.cpu().numpy()
    med_e, med_s = statistics.median(t_exp), statistics.median(t_sign)
    return {"n": n, "n_keys": n_keys, "message_bytes": MSG_BYTES,
            "stream_form": _spread(t_sign, n), "expand_keys": _spread(t_exp, n_keys),
            "expand_share_of_expand_plus_sign": med_e / (med_e + med_s),
            "host_pointer_form": _spread(t_host, n),
            "ok_all_ones": bool(d_ok.all().item()) and bool(h_ok.all()), "forms_agree": bool((sigs == h_sig).all()),
            "_sigs": sigs, "_seeds": seeds, "_msgs": msgs}


def cpu_rates(seeds, msgs, n_keys, count=1 << 14, threads=16):
    """the host signer (consensus_amd/host: ed25519_sign behind sbvh_sign) on `count` of the messages: one thread, then `threads`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostlib
    h = hostlib.load()
    signers = [h.sbvh_signer_new_scheme(1, 1, seeds[32 * k:32 * k + 32]) for k in range(n_keys)]
    blob = msgs.tobytes()
    sigs = [None] * count

    def work(lo, hi):
        out = ctypes.create_string_buffer(80)
        for i in range(lo, hi):
            h.sbvh_sign(signers[i % n_keys], blob[MSG_BYTES * i:MSG_BYTES * (i + 1)], MSG_BYTES, out, 80)
            sigs[i] = out.raw[:64]
    t0 = time.perf_counter()
    work(0, count // 8)
    one = (count // 8) / (time.perf_counter() - t0)
    step = (count + threads - 1) // threads
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda t: work(t * step, min(count, (t + 1) * step)), range(threads)))
        many = count / (time.perf_counter() - t0)
    for s in signers:
        h.sbvh_signer_free(s)
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
    t = _timed(lambda: sbv.sign_batch_dev(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_sig.data_ptr(), d_ok.data_ptr(), st.cuda_stream),
               torch.cuda.synchronize, warm, timed)
    return _spread(t, n)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    sbv.init(0)
    r = device_rates(n, n_keys)
    sigs, seeds, msgs = r.pop("_sigs"), r.pop("_seeds"), r.pop("_msgs")
    count = min(n, 1 << 14)
    one, many, host_sigs = cpu_rates(seeds, msgs, n_keys, count)
    r["device_equals_host_signer"] = all(sigs[64 * i:64 * i + 64].tobytes() == host_sigs[i] for i in range(count))
    r["host_signer"] = {"one_thread_signatures_per_s": one, "sixteen_threads_signatures_per_s": many, "messages": count,
                        "note": "16 Python threads around a C call that releases the interpreter lock"}
    r["p256_device_signer"] = p256_rate(n, n_keys)
    r["stream_form_over_16_host_threads"] = r["stream_form"]["signatures_per_s"] / many
    r["metric"] = "Ed25519 signatures/s, device-resident, batch=%d" % n
    r["value"] = r["stream_form"]["signatures_per_s"]
    r["unit"] = "signatures/s"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
