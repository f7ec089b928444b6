#!/usr/bin/env python3
"""secp256k1 public-key recovery on one MI355X: keys/s through sbv_secp256k1_recover_stream (device-resident buffers and workspace) and
through the host-pointer entry sbv_secp256k1_recover, read against the yardstick measured beside them in the same run — the one-lane
generic verifier (sbv_secp256k1_verify_batch_dev with grouping off) on the same signatures: recovery is its walk plus one square root,
the scalar inversion it already pays, and one field inversion — and against the host form (consensus_amd/host: k256_recover, one
thread and 16).  Workload: 2^18 signatures under 1 024 keys, signed on the device in low-S form; every result is compared with the
signers' keys before it is timed; 3 warm calls and 10 timed ones, median and spread (min .. max).  One JSON line.

    python tools/bench_secp256k1_recover.py [n] [n_keys]"""
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


def _spread(times, n, unit="keys_per_s"):
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


def device_rates(n=1 << 18, n_keys=1024, warm=WARM, timed=TIMED):
    import torch
    keys = b"".join((int.from_bytes(hashlib.sha256(b"bench-k256-recover%d" % i).digest(), "big") % (ORDER - 1) + 1).to_bytes(32, "big")
                    for i in range(n_keys))
    digests = np.random.default_rng(0x2EC0).integers(0, 256, 32 * n, dtype=np.uint8)
    d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
    d_dig = torch.from_numpy(digests).cuda()
    d_sig = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    d_rid, d_sok = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_kpub, d_kok = torch.empty(64 * n_keys, dtype=torch.uint8, device="cuda"), torch.zeros(n_keys, dtype=torch.uint8, device="cuda")
    d_pub, d_ok = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    wb = sbv.secp256k1_recover_workspace(n)
    d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    torch.cuda.synchronize()
    # the workload: signatures and recovery ids from the device signer (key i % n_keys), and the signers' keys
    sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_sig.data_ptr(), d_rid.data_ptr(), d_sok.data_ptr(), low_s=True, stream=sp)
    sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), n_keys, d_kpub.data_ptr(), d_kok.data_ptr(), sp)
    torch.cuda.synchronize()
    assert bool(d_sok.all().item()) and bool(d_kok.all().item())
    want = d_kpub.view(n_keys, 64)[torch.arange(n, device="cuda") % n_keys].contiguous()

    def stream_form():
        sbv.secp256k1_recover_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_pub.data_ptr(), d_ok.data_ptr(), d_work.data_ptr(), wb,
                                     low_s=True, stream=sp)
    stream_form()
    torch.cuda.synchronize()
    assert bool(d_ok.all().item()) and torch.equal(d_pub.view(n, 64), want), "recovery: not the signers' keys"
    t_stream = _timed(stream_form, torch.cuda.synchronize, warm, timed)

    lib = sbv.load()
    lib.sbv_secp256k1_recover.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    h_sig, h_rid = d_sig.cpu().numpy(), d_rid.cpu().numpy()
    h_pub, h_ok = np.zeros(64 * n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

    def host_form():
        rc = lib.sbv_secp256k1_recover(h_sig.ctypes.data, h_rid.ctypes.data, digests.ctypes.data, n, 1, h_pub.ctypes.data, h_ok.ctypes.data)
        assert rc == 0, rc
    host_form()
    assert bool(h_ok.all()) and bool((h_pub == want.cpu().numpy().reshape(-1)).all()), "recovery, host pointers: not the signers' keys"
    t_host = _timed(host_form, lambda: None, warm, timed)

    # the yardstick: the one-lane generic verifier on the same signatures with their keys, grouping off
    d_tup = torch.cat([d_sig.view(n, 64), d_dig.view(n, 32), want], dim=1).contiguous()
    d_bm = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sbv.set_grouping(False)
    try:
        def verify():
            sbv.secp256k1_verify_batch_dev(d_tup.data_ptr(), n, d_bm.data_ptr(), sp)
        verify()
        torch.cuda.synchronize()
        bits = np.unpackbits(d_bm.cpu().numpy(), bitorder="little")[:n]
        assert bool(bits.all()), "the generic verifier refuses a signature of the workload"
        t_verify = _timed(verify, torch.cuda.synchronize, warm, timed)
    finally:
        sbv.set_grouping(True)
    return {"n": n, "n_keys": n_keys, "flags": "SBV_K256_RECOVER_LOW_S", "workspace_bytes": wb,
            "stream_form": _spread(t_stream, n), "host_pointer_form": _spread(t_host, n),
            "one_lane_generic_verifier_grouping_off": _spread(t_verify, n, "verifies_per_s"),
            "_sigs": h_sig, "_rid": h_rid, "_digests": digests, "_want": want.cpu().numpy()}


def cpu_rates(sigs, rid, digests, want, count=1 << 13, threads=16):
    """the host form (k256_recover behind sbvh_k256_recover) on `count` of the signatures: one thread, then `threads`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostlib
    h = hostlib.load()
    h.sbvh_k256_recover.argtypes = [ctypes.c_char_p, ctypes.c_uint8, ctypes.c_char_p, ctypes.c_char_p]
    sb, db = sigs.tobytes(), digests.tobytes()
    good = [True] * count

    def work(lo, hi):
        out = ctypes.create_string_buffer(64)
        for i in range(lo, hi):
            rc = h.sbvh_k256_recover(sb[64 * i:64 * i + 64], int(rid[i]), db[32 * i:32 * i + 32], out)
            good[i] = rc == 0 and out.raw == want[i].tobytes()
    work(0, 8)                                       # builds the host comb
    t0 = time.perf_counter()
    work(0, count // 8)
    one = (count // 8) / (time.perf_counter() - t0)
    step = (count + threads - 1) // threads
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda t: work(t * step, min(count, (t + 1) * step)), range(threads)))
        many = count / (time.perf_counter() - t0)
    assert all(good), "the host form: not the signers' keys"
    return one, many


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    sbv.init(0)
    r = device_rates(n, n_keys)
    sigs, rid, digests, want = r.pop("_sigs"), r.pop("_rid"), r.pop("_digests"), r.pop("_want")
    count = min(n, 1 << 13)
    one, many = cpu_rates(sigs, rid, digests, want, count)
    r["host_form"] = {"one_thread_keys_per_s": one, "sixteen_threads_keys_per_s": many, "signatures": count,
                      "note": "16 Python threads around a C call that releases the interpreter lock"}
    r["recover_time_over_verify_time"] = r["stream_form"]["median_ms"] / r["one_lane_generic_verifier_grouping_off"]["median_ms"]
    r["stream_form_over_16_host_threads"] = r["stream_form"]["keys_per_s"] / many
    r["metric"] = "secp256k1 recovered keys/s, device-resident, batch=%d" % n
    r["value"] = r["stream_form"]["keys_per_s"]
    r["unit"] = "keys/s"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
