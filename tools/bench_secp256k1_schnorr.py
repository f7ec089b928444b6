#!/usr/bin/env python3
"""BIP-340 Schnorr over secp256k1 on one MI355X: verifications/s through sbv_secp256k1_schnorr_verify_stream (device-resident buffers
and workspace) and through the host-pointer entry, signatures/s through sbv_secp256k1_schnorr_sign_stream, and the key expansion per
n_keys and per n, read against the yardsticks measured beside them in the same run: sbv_secp256k1_recover_stream on ECDSA signatures of
the same keys (a Schnorr verify lane is recovery's work minus a scalar inversion plus two compressions), the one-lane generic ECDSA
verifier with grouping off, the ECDSA device signer and k_k256_pubkeys (a Schnorr sign lane is its work plus five compressions).
Workload: 2^18 messages under 1 024 keys.  Every result is checked before it is timed: the signatures verify on the device, a spoiled
third does not, the expanded public keys are the x of k_k256_pubkeys' and the first signatures equal the Python model's.  3 warm calls
and 10 timed ones, median and spread (min .. max).  One JSON line.

    python tools/bench_secp256k1_schnorr.py [n] [n_keys]"""
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


def _model_check(keys, msgs, aux, sigs, count=4):
    """the first signatures against the Python model of tests/k256_schnorr_cases.py"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import k256_schnorr_cases as model
    for i in range(count):
        rec, _, ok = model.expand(int.from_bytes(keys[32 * i:32 * i + 32], "big"))
        assert ok and model.sign(rec, msgs[32 * i:32 * i + 32], aux[32 * i:32 * i + 32]) == (sigs[64 * i:64 * i + 64], 1), "signature %d is not the model's" % i


def rates(n=1 << 18, n_keys=1024, warm=WARM, timed=TIMED):
    import torch
    keys = b"".join((int.from_bytes(hashlib.sha256(b"bench-k256-schnorr%d" % i).digest(), "big") % (ORDER - 1) + 1).to_bytes(32, "big")
                    for i in range(n_keys))
    rng = np.random.default_rng(0xB340)
    msgs, aux = rng.integers(0, 256, 32 * n, dtype=np.uint8), rng.integers(0, 256, 32 * n, dtype=np.uint8)
    u8 = lambda k, fill=torch.zeros: fill(k, dtype=torch.uint8, device="cuda")
    d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
    d_msg, d_aux = torch.from_numpy(msgs).cuda(), torch.from_numpy(aux).cuda()
    d_rec, d_pk, d_eok = u8(64 * n_keys), u8(32 * n_keys), u8(n_keys)
    d_sig, d_sok, d_vok = u8(64 * n), u8(n), u8(n)
    wb = sbv.secp256k1_schnorr_verify_workspace(n)
    d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    sync = torch.cuda.synchronize
    sync()

    # expand, sign (key i % n_keys), verify; a copy with every third signature spoiled in one bit
    def expand():
        sbv.secp256k1_schnorr_expand_keys_stream(d_keys.data_ptr(), n_keys, d_rec.data_ptr(), d_pk.data_ptr(), d_eok.data_ptr(), sp)

    def sign():
        sbv.secp256k1_schnorr_sign_stream(d_rec.data_ptr(), n_keys, 0, d_msg.data_ptr(), d_aux.data_ptr(), n, d_sig.data_ptr(), d_sok.data_ptr(), sp)
    expand()
    sign()
    sync()
    assert bool(d_eok.all().item()) and bool(d_sok.all().item())
    d_pks = d_pk.view(n_keys, 32)[torch.arange(n, device="cuda") % n_keys].contiguous()

    def verify(sig=d_sig):
        sbv.secp256k1_schnorr_verify_stream(d_pks.data_ptr(), d_msg.data_ptr(), sig.data_ptr(), n, d_vok.data_ptr(), d_work.data_ptr(), wb, sp)
    verify()
    sync()
    assert bool(d_vok.all().item()), "a signature of the workload does not verify"
    d_bad = d_sig.clone()
    d_bad.view(n, 64)[2::3, 40] ^= 4
    sync()
    verify(d_bad)
    sync()
    assert bool((d_vok.view(-1) == (torch.arange(n, device="cuda") % 3 != 2).to(torch.uint8)).all().item()), "a spoiled signature verifies"
    _model_check(keys, msgs.tobytes(), aux.tobytes(), d_sig[:256].cpu().numpy().tobytes())
    t_verify = _timed(verify, sync, warm, timed)
    t_sign = _timed(sign, sync, warm, timed)
    t_expand = _timed(expand, sync, warm, timed)
    # expansion of n keys: the key set repeated
    d_keys_n = d_keys.view(n_keys, 32)[torch.arange(n, device="cuda") % n_keys].contiguous()
    d_rec_n, d_eok_n = u8(64 * n), u8(n)
    sync()

    def expand_n():
        sbv.secp256k1_schnorr_expand_keys_stream(d_keys_n.data_ptr(), n, d_rec_n.data_ptr(), 0, d_eok_n.data_ptr(), sp)
    expand_n()
    sync()
    assert torch.equal(d_rec_n.view(n, 64)[:n_keys], d_rec.view(n_keys, 64)) and bool(d_eok_n.all().item())
    t_expand_n = _timed(expand_n, sync, warm, timed)

    lib = sbv.load()
    lib.sbv_secp256k1_schnorr_verify.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    h_pk, h_sig, h_ok = d_pks.cpu().numpy().reshape(-1), d_sig.cpu().numpy(), np.zeros(n, dtype=np.uint8)

    def host_form():
        rc = lib.sbv_secp256k1_schnorr_verify(h_pk.ctypes.data, msgs.ctypes.data, h_sig.ctypes.data, n, h_ok.ctypes.data)
        assert rc == 0, rc
    host_form()
    assert bool(h_ok.all()), "verify, host pointers: a signature of the workload does not verify"
    t_host = _timed(host_form, lambda: None, warm, timed)

    # the yardsticks of the same run: ECDSA under the same keys and messages-as-digests
    e_sig, e_rid, e_sok = u8(64 * n), u8(n), u8(n)
    e_kpub, e_kok = u8(64 * n_keys), u8(n_keys)
    e_pub, e_rok = u8(64 * n), u8(n)
    sync()

    def ecdsa_sign():
        sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), n_keys, 0, d_msg.data_ptr(), n, e_sig.data_ptr(), e_rid.data_ptr(), e_sok.data_ptr(), low_s=True, stream=sp)

    def pubkeys():
        sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), n_keys, e_kpub.data_ptr(), e_kok.data_ptr(), sp)

    def recover():
        sbv.secp256k1_recover_stream(e_sig.data_ptr(), e_rid.data_ptr(), d_msg.data_ptr(), n, e_pub.data_ptr(), e_rok.data_ptr(), d_work.data_ptr(), wb,
                                     low_s=True, stream=sp)
    ecdsa_sign()
    pubkeys()
    recover()
    sync()
    want = e_kpub.view(n_keys, 64)[torch.arange(n, device="cuda") % n_keys].contiguous()
    assert bool(e_sok.all().item()) and bool(e_kok.all().item()) and bool(e_rok.all().item()) and torch.equal(e_pub.view(n, 64), want)
    assert torch.equal(e_kpub.view(n_keys, 64)[:, :32].contiguous().view(-1), d_pk), "the expanded public keys are not the x of d G"
    t_recover = _timed(recover, sync, warm, timed)
    t_esign = _timed(ecdsa_sign, sync, warm, timed)
    t_pub = _timed(pubkeys, sync, warm, timed)
    d_keys_pub_n, e_kok_n = u8(64 * n), u8(n)
    sync()

    def pubkeys_n():
        sbv.secp256k1_pubkeys_stream(d_keys_n.data_ptr(), n, d_keys_pub_n.data_ptr(), e_kok_n.data_ptr(), sp)
    pubkeys_n()
    sync()
    t_pub_n = _timed(pubkeys_n, sync, warm, timed)
    d_tup = torch.cat([e_sig.view(n, 64), d_msg.view(n, 32), want], dim=1).contiguous()
    d_bm = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
    sync()
    sbv.set_grouping(False)
    try:
        def ecdsa_verify():
            sbv.secp256k1_verify_batch_dev(d_tup.data_ptr(), n, d_bm.data_ptr(), sp)
        ecdsa_verify()
        sync()
        assert bool(np.unpackbits(d_bm.cpu().numpy(), bitorder="little")[:n].all()), "the generic verifier refuses a signature of the workload"
        t_everify = _timed(ecdsa_verify, sync, warm, timed)
    finally:
        sbv.set_grouping(True)
    r = {"n": n, "n_keys": n_keys, "workspace_bytes": wb,
         "verify_stream_form": _spread(t_verify, n, "verifies_per_s"), "verify_host_pointer_form": _spread(t_host, n, "verifies_per_s"),
         "sign_stream_form": _spread(t_sign, n, "signatures_per_s"),
         "expand_n_keys": _spread(t_expand, n_keys, "keys_per_s"), "expand_n": _spread(t_expand_n, n, "keys_per_s"),
         "yardstick_ecdsa_recover_stream": _spread(t_recover, n, "keys_per_s"),
         "yardstick_one_lane_generic_verifier_grouping_off": _spread(t_everify, n, "verifies_per_s"),
         "yardstick_ecdsa_sign_stream": _spread(t_esign, n, "signatures_per_s"),
         "yardstick_pubkeys_n_keys": _spread(t_pub, n_keys, "keys_per_s"), "yardstick_pubkeys_n": _spread(t_pub_n, n, "keys_per_s")}
    med = lambda k: r[k]["median_ms"]
    r["verify_time_over_recover_time"] = med("verify_stream_form") / med("yardstick_ecdsa_recover_stream")
    r["recover_spread_over_its_median"] = (r["yardstick_ecdsa_recover_stream"]["max_ms"] - r["yardstick_ecdsa_recover_stream"]["min_ms"]) / med("yardstick_ecdsa_recover_stream")
    r["verify_time_over_generic_verifier_time"] = med("verify_stream_form") / med("yardstick_one_lane_generic_verifier_grouping_off")
    r["sign_time_over_pubkeys_n_time"] = med("sign_stream_form") / med("yardstick_pubkeys_n")
    r["sign_time_over_ecdsa_sign_time"] = med("sign_stream_form") / med("yardstick_ecdsa_sign_stream")
    r["expand_n_time_over_pubkeys_n_time"] = med("expand_n") / med("yardstick_pubkeys_n")
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    sbv.init(0)
    r = rates(n, n_keys)
    r["metric"] = "BIP-340 verifications/s, device-resident, batch=%d" % n
    r["value"] = r["verify_stream_form"]["verifies_per_s"]
    r["unit"] = "verifies/s"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
