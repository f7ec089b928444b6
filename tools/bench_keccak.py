#!/usr/bin/env python3
"""Keccak-256 and Ethereum-style addresses on one MI355X, every yardstick in the same run:

  * sbv_secp256k1_recover_addresses_stream against sbv_secp256k1_recover_stream alone and against the composition it replaces,
    recover_stream followed by sbv_secp256k1_addresses_stream on one stream (through a device-resident key plane);
  * sbv_keccak256_msgs_stream at 32-, 64-, 136- and 200-byte messages: messages/s and input bytes/s, against a device-to-device copy of
    the same bytes and against the host form (consensus_amd/host: keccak256) on one thread and on 16;
  * sbv_secp256k1_addresses_stream at the same number of keys, with sbv_secp256k1_pubkeys_stream's time beside it for scale.

Workload: 2^18 items; the signatures under 1 024 keys, signed on the device in low-S form.  Every output is compared before it is
timed: digests and addresses with the host form (itself held to the Python model by tests/test_keccak_cpu.py) and a sample with the
model of tests/keccak_cases.py; recovered addresses with the addresses of the signers' keys.  3 warm calls and 10 timed ones, median
and spread (min .. max).  One JSON line.

    python tools/bench_keccak.py [n] [n_keys]"""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import consensus_amd as sbv  # noqa: E402

WARM, TIMED = 3, 10
ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SIZES = (32, 64, 136, 200)


def _spread(times, n, unit):
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


def _host():
    import hostlib
    h = hostlib.load()
    h.sbvh_keccak256_range.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    h.sbvh_keccak256_range.restype = None
    return h


def _host_digests(h, msgs, offs, n, threads):
    """(digests, seconds) of the host form over n messages on `threads` threads (the C loop releases the interpreter lock)"""
    out = np.zeros(32 * n, dtype=np.uint8)
    step = (n + threads - 1) // threads
    t0 = time.perf_counter()
    if threads == 1:
        h.sbvh_keccak256_range(msgs.ctypes.data, offs.ctypes.data, 0, n, out.ctypes.data)
    else:
        with concurrent.futures.ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda t: h.sbvh_keccak256_range(msgs.ctypes.data, offs.ctypes.data, t * step, min(n, (t + 1) * step), out.ctypes.data),
                        range(threads)))
    return out, time.perf_counter() - t0


def message_rates(torch, h, n, sp):
    import keccak_cases as kc
    out = {}
    sync = torch.cuda.synchronize
    for size in SIZES:
        msgs = np.random.default_rng(0xCECC + size).integers(0, 256, size * n, dtype=np.uint8)
        offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
        want, t_one = _host_digests(h, msgs, offs, n, 1)
        want16, t_many = _host_digests(h, msgs, offs, n, 16)
        assert bool((want == want16).all())
        for i in range(0, n, max(1, n // 64)):                                   # a sample against the Python model
            assert want[32 * i:32 * i + 32].tobytes() == kc.keccak256(msgs[size * i:size * i + size].tobytes()), (size, i)
        d_msgs, d_off = torch.from_numpy(msgs).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
        d_dig, d_copy = torch.zeros(32 * n, dtype=torch.uint8, device="cuda"), torch.empty_like(d_msgs)
        sync()

        def hash_call():
            sbv.keccak256_msgs_stream(d_msgs.data_ptr(), d_off.data_ptr(), n, d_dig.data_ptr(), sp)
        hash_call()
        sync()
        assert bool((d_dig.cpu().numpy() == want).all()), "keccak256_msgs_stream: not the host form's digests at %d bytes" % size
        t_hash = _timed(hash_call, sync)
        st = torch.cuda.ExternalStream(sp)

        def copy_call():
            with torch.cuda.stream(st):
                d_copy.copy_(d_msgs, non_blocking=True)
        t_copy = _timed(copy_call, sync)
        r = _spread(t_hash, n, "messages_per_s")
        r["input_bytes_per_s"] = size * n / statistics.median(t_hash)
        r["device_to_device_copy_of_the_same_bytes"] = _spread(t_copy, size * n, "bytes_per_s")
        r["host_form"] = {"one_thread_messages_per_s": n / t_one, "sixteen_threads_messages_per_s": n / t_many}
        out["%d_bytes" % size] = r
    return out


def recovery_rates(torch, n, n_keys, sp):
    sync = torch.cuda.synchronize
    keys = b"".join((int.from_bytes(hashlib.sha256(b"bench-keccak%d" % i).digest(), "big") % (ORDER - 1) + 1).to_bytes(32, "big")
                    for i in range(n_keys))
    digests = np.random.default_rng(0x2EC0).integers(0, 256, 32 * n, dtype=np.uint8)
    d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
    d_dig = torch.from_numpy(digests).cuda()
    d_sig = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    d_rid, d_sok = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_kpub, d_kok = torch.empty(64 * n_keys, dtype=torch.uint8, device="cuda"), torch.zeros(n_keys, dtype=torch.uint8, device="cuda")
    d_kaddr = torch.zeros(20 * n_keys, dtype=torch.uint8, device="cuda")
    d_pub, d_ok = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_addr, d_addr2 = torch.zeros(20 * n, dtype=torch.uint8, device="cuda"), torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
    wb = sbv.secp256k1_recover_workspace(n)
    d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    sync()
    sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), n_keys, 0, d_dig.data_ptr(), n, d_sig.data_ptr(), d_rid.data_ptr(), d_sok.data_ptr(), low_s=True, stream=sp)
    sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), n_keys, d_kpub.data_ptr(), d_kok.data_ptr(), sp)
    sbv.secp256k1_addresses_stream(d_kpub.data_ptr(), n_keys, d_kaddr.data_ptr(), sp)
    sync()
    assert bool(d_sok.all().item()) and bool(d_kok.all().item())
    # the signers' addresses by the host form
    import hostlib
    h = hostlib.load()
    h.sbvh_k256_address.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    h.sbvh_k256_address.restype = None
    kpub, a = d_kpub.cpu().numpy().tobytes(), ctypes.create_string_buffer(20)
    host_addrs = b""
    for i in range(n_keys):
        h.sbvh_k256_address(kpub[64 * i:64 * i + 64], a)
        host_addrs += a.raw
    assert d_kaddr.cpu().numpy().tobytes() == host_addrs, "addresses_stream: not the host form's addresses"
    pick = torch.arange(n, device="cuda") % n_keys
    want_addr = d_kaddr.view(n_keys, 20)[pick].contiguous()
    want_pub = d_kpub.view(n_keys, 64)[pick].contiguous()

    def fused():
        sbv.secp256k1_recover_addresses_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_addr.data_ptr(), d_ok.data_ptr(), d_work.data_ptr(),
                                               wb, low_s=True, stream=sp)

    def recover_only():
        sbv.secp256k1_recover_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_pub.data_ptr(), d_ok.data_ptr(), d_work.data_ptr(), wb,
                                     low_s=True, stream=sp)

    def composition():
        recover_only()
        sbv.secp256k1_addresses_stream(d_pub.data_ptr(), n, d_addr2.data_ptr(), sp)

    def addresses_only():
        sbv.secp256k1_addresses_stream(want_pub.data_ptr(), n, d_addr2.data_ptr(), sp)

    def pubkeys():
        sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), n_keys, d_kpub.data_ptr(), d_kok.data_ptr(), sp)
    fused()
    sync()
    assert bool(d_ok.all().item()) and torch.equal(d_addr.view(n, 20), want_addr), "recover_addresses: not the signers' addresses"
    composition()
    sync()
    assert bool(d_ok.all().item()) and torch.equal(d_addr2.view(n, 20), want_addr) and torch.equal(d_pub.view(n, 64), want_pub)
    # alternating, so that a drift of the machine touches all three alike
    t = {"fused": [], "recover": [], "composition": []}
    for rnd in range(2):
        for name, fn in (("fused", fused), ("recover", recover_only), ("composition", composition)):
            t[name] += _timed(fn, sync, WARM, TIMED // 2)
    d_keys_n = d_keys.repeat((n + n_keys - 1) // n_keys)[:32 * n].contiguous()
    d_pub_n, d_ok_n = torch.empty(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")

    def pubkeys_n():
        sbv.secp256k1_pubkeys_stream(d_keys_n.data_ptr(), n, d_pub_n.data_ptr(), d_ok_n.data_ptr(), sp)
    r = {"n": n, "n_keys": n_keys, "flags": "SBV_K256_RECOVER_LOW_S", "workspace_bytes": wb,
         "recover_addresses_stream": _spread(t["fused"], n, "addresses_per_s"),
         "recover_stream": _spread(t["recover"], n, "keys_per_s"),
         "recover_stream_then_addresses_stream": _spread(t["composition"], n, "addresses_per_s"),
         "addresses_stream": _spread(_timed(addresses_only, sync), n, "addresses_per_s"),
         "pubkeys_stream_same_count": _spread(_timed(pubkeys_n, sync), n, "keys_per_s")}
    # the rule of DESIGN.md section 4.8.8: the fused entry may trail the composition by no more than the range of the composition's own calls
    comp = r["recover_stream_then_addresses_stream"]
    r["fused_minus_composition_median_ms"] = r["recover_addresses_stream"]["median_ms"] - comp["median_ms"]
    r["composition_range_ms"] = comp["max_ms"] - comp["min_ms"]
    r["fused_no_slower_than_the_composition"] = r["fused_minus_composition_median_ms"] <= r["composition_range_ms"]
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    import torch
    sbv.init(0)
    st = torch.cuda.Stream()
    r = recovery_rates(torch, n, n_keys, st.cuda_stream)
    r["keccak256_msgs_stream"] = message_rates(torch, _host(), n, st.cuda_stream)
    r["metric"] = "secp256k1 recovered addresses/s, device-resident, batch=%d" % n
    r["value"] = r["recover_addresses_stream"]["addresses_per_s"]
    r["unit"] = "addresses/s"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
