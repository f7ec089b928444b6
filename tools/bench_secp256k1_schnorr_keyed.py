#!/usr/bin/env python3
"""BIP-340 Schnorr against registered secp256k1 keys on one MI355X: verifications/s through sbv_secp256k1_schnorr_verify_keyed_stream
(device-resident buffers) on 8-bit combs and with the keys widened to 16-bit combs, and through the host-pointer entry, read against
the yardsticks measured beside them in the same run: sbv_secp256k1_schnorr_verify_stream on the same items (the generic verifier: the
keyed one does strictly less work of every kind and must be faster), sbv_secp256k1_verify_batch_keyed_dev on ECDSA signatures of the
same keys, narrow and wide (a Schnorr keyed lane has no stage A and no shared scalar inversion, but two compressions and a field
inversion of its own), and sbv_secp256k1_schnorr_lift_keys per n_keys.
Workload: 2^18 messages under 1 024 registered keys (registered as the ECDSA public keys Qx | Qy: both parities occur).  Every verdict
is compared with the generic verifier's before anything is timed: the signatures verify, a spoiled third does not.  3 warm calls and
10 timed ones, median and spread (min .. max).  One JSON line.

    python tools/bench_secp256k1_schnorr_keyed.py [n] [n_keys]"""
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


def rates(n=1 << 18, n_keys=1024, warm=WARM, timed=TIMED):
    import torch
    keys = b"".join((int.from_bytes(hashlib.sha256(b"bench-k256-schnorr-keyed%d" % i).digest(), "big") % (ORDER - 1) + 1).to_bytes(32, "big")
                    for i in range(n_keys))
    rng = np.random.default_rng(0xB341)
    msgs, aux = rng.integers(0, 256, 32 * n, dtype=np.uint8), rng.integers(0, 256, 32 * n, dtype=np.uint8)
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")
    d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
    d_msg, d_aux = torch.from_numpy(msgs).cuda(), torch.from_numpy(aux).cuda()
    d_rec, d_pk, d_eok = u8(64 * n_keys), u8(32 * n_keys), u8(n_keys)
    d_sig, d_sok, d_vok, d_kok = u8(64 * n), u8(n), u8(n), u8(n)
    wb = sbv.secp256k1_schnorr_verify_workspace(n)
    d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    sync = torch.cuda.synchronize
    sync()

    # the workload: BIP-340 and ECDSA signatures of the same messages under the same keys (key i % n_keys)
    sbv.secp256k1_schnorr_expand_keys_stream(d_keys.data_ptr(), n_keys, d_rec.data_ptr(), d_pk.data_ptr(), d_eok.data_ptr(), sp)
    sbv.secp256k1_schnorr_sign_stream(d_rec.data_ptr(), n_keys, 0, d_msg.data_ptr(), d_aux.data_ptr(), n, d_sig.data_ptr(), d_sok.data_ptr(), sp)
    e_sig, e_rid, e_sok = u8(64 * n), u8(n), u8(n)
    e_kpub, e_kok = u8(64 * n_keys), u8(n_keys)
    sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), n_keys, 0, d_msg.data_ptr(), n, e_sig.data_ptr(), e_rid.data_ptr(), e_sok.data_ptr(), low_s=True, stream=sp)
    sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), n_keys, e_kpub.data_ptr(), e_kok.data_ptr(), sp)
    sync()
    assert all(bool(t.all().item()) for t in (d_eok, d_sok, e_sok, e_kok))
    pubs = e_kpub.cpu().numpy().tobytes()
    odd = sum(pubs[64 * i + 63] & 1 for i in range(n_keys))

    # the registry: the ECDSA public keys as they are; lifting the x-only keys gives the same x and the even y
    sbv.secp256k1_clear_keys()
    slots = sbv.secp256k1_register_keys([pubs[64 * i:64 * i + 64] for i in range(n_keys)])
    assert len(set(slots)) == n_keys
    d_slot = torch.from_numpy(np.array(slots, dtype=np.uint32).view(np.int32)).cuda()[torch.arange(n, device="cuda") % n_keys].contiguous()
    d_pks = d_pk.view(n_keys, 32)[torch.arange(n, device="cuda") % n_keys].contiguous()
    d_k64, d_lok = u8(64 * n_keys), u8(n_keys)
    sync()

    def lift():
        sbv.secp256k1_schnorr_lift_keys_stream(d_pk.data_ptr(), n_keys, d_k64.data_ptr(), d_lok.data_ptr(), sp)
    lift()
    sync()
    lifted = d_k64.cpu().numpy().tobytes()
    assert bool(d_lok.all().item())
    for i in range(n_keys):
        q, k = pubs[64 * i:64 * i + 64], lifted[64 * i:64 * i + 64]
        assert k[:32] == q[:32] and k[63] & 1 == 0 and (k == q or int.from_bytes(k[32:], "big") + int.from_bytes(q[32:], "big") == (1 << 256) - (1 << 32) - 977)

    def keyed(sig=d_sig, out=d_kok):
        sbv.secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), sig.data_ptr(), d_slot.data_ptr(), n, out.data_ptr(), sp)

    def generic(sig=d_sig, out=d_vok):
        sbv.secp256k1_schnorr_verify_stream(d_pks.data_ptr(), d_msg.data_ptr(), sig.data_ptr(), n, out.data_ptr(), d_work.data_ptr(), wb, sp)
    d_bad = d_sig.clone()
    d_bad.view(n, 64)[2::3, 40] ^= 4
    want_bad = (torch.arange(n, device="cuda") % 3 != 2).to(torch.uint8)
    sync()

    def check(what):
        """every verdict of the keyed verifier against the generic verifier's, on the signatures and on the spoiled copy"""
        for sig, all_good in ((d_sig, True), (d_bad, False)):
            keyed(sig)
            generic(sig)
            sync()
            assert torch.equal(d_kok, d_vok), what + ": the keyed verifier disagrees with the generic verifier"
            assert bool(d_kok.all().item()) if all_good else torch.equal(d_kok, want_bad), what + ": a verdict is wrong"

    # ECDSA keyed, the yardstick: 96-byte records r | s | hash against the same slots
    d_recs = torch.cat([e_sig.view(n, 64), d_msg.view(n, 32)], dim=1).contiguous()
    d_bm = torch.zeros((n + 7) // 8 + 16, dtype=torch.uint8, device="cuda")
    assert d_recs.data_ptr() % 16 == 0

    def ecdsa_keyed():
        sbv.secp256k1_verify_batch_keyed_dev(d_recs.data_ptr(), d_slot.data_ptr(), n, d_bm.data_ptr(), sp)

    def check_ecdsa(what):
        ecdsa_keyed()
        sync()
        assert bool(np.unpackbits(d_bm.cpu().numpy(), bitorder="little")[:n].all()), what + ": the ECDSA keyed verifier refuses a signature of the workload"

    lib = sbv.load()
    lib.sbv_secp256k1_schnorr_verify_keyed.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    h_sig, h_slot, h_ok = d_sig.cpu().numpy(), d_slot.cpu().numpy(), np.zeros(n, dtype=np.uint8)

    def host_form():
        rc = lib.sbv_secp256k1_schnorr_verify_keyed(msgs.ctypes.data, h_sig.ctypes.data, h_slot.ctypes.data, n, h_ok.ctypes.data)
        assert rc == 0, rc

    # narrow: every slot on its 8-bit comb
    assert sbv.secp256k1_wide_key_stats()[0] == 0
    check("8-bit combs")
    check_ecdsa("8-bit combs")
    host_form()
    assert bool(h_ok.all()), "host pointers: a signature of the workload does not verify"
    t_keyed = _timed(keyed, sync, warm, timed)
    t_generic = _timed(generic, sync, warm, timed)
    t_ecdsa = _timed(ecdsa_keyed, sync, warm, timed)
    t_host = _timed(host_form, lambda: None, warm, timed)
    t_lift = _timed(lift, sync, warm, timed)

    # wide: as many keys as sbv_secp256k1_wide_keys allows (4 096), which is all of them at the default workload
    n_wide = min(n_keys, 4096)
    t0 = time.perf_counter()
    sbv.secp256k1_wide_keys(n_wide)
    sbv.secp256k1_widen_keys(slots[:n_wide])
    widen_s = time.perf_counter() - t0
    widened = sbv.secp256k1_wide_key_stats()[0]
    try:
        check("16-bit combs")
        check_ecdsa("16-bit combs")
        t_keyed_w = _timed(keyed, sync, warm, timed)
        t_ecdsa_w = _timed(ecdsa_keyed, sync, warm, timed)
        t_generic2 = _timed(generic, sync, warm, timed)
    finally:
        sbv.secp256k1_wide_keys(0)
        sbv.secp256k1_wide_keys(64)
        sbv.secp256k1_clear_keys()
    r = {"n": n, "n_keys": n_keys, "keys_with_odd_y": odd, "widened_keys": widened, "widen_seconds": widen_s,
         "keyed_stream_form_8_bit": _spread(t_keyed, n, "verifies_per_s"), "keyed_stream_form_16_bit": _spread(t_keyed_w, n, "verifies_per_s"),
         "keyed_host_pointer_form_8_bit": _spread(t_host, n, "verifies_per_s"),
         "yardstick_generic_schnorr_verify_stream": _spread(t_generic, n, "verifies_per_s"),
         "yardstick_generic_schnorr_verify_stream_again": _spread(t_generic2, n, "verifies_per_s"),
         "yardstick_ecdsa_keyed_dev_8_bit": _spread(t_ecdsa, n, "verifies_per_s"), "yardstick_ecdsa_keyed_dev_16_bit": _spread(t_ecdsa_w, n, "verifies_per_s"),
         "lift_n_keys": _spread(t_lift, n_keys, "keys_per_s")}
    med = lambda k: r[k]["median_ms"]
    r["keyed_8_bit_time_over_generic_time"] = med("keyed_stream_form_8_bit") / med("yardstick_generic_schnorr_verify_stream")
    r["keyed_16_bit_time_over_generic_time"] = med("keyed_stream_form_16_bit") / med("yardstick_generic_schnorr_verify_stream")
    r["keyed_8_bit_time_over_ecdsa_keyed_time"] = med("keyed_stream_form_8_bit") / med("yardstick_ecdsa_keyed_dev_8_bit")
    r["keyed_16_bit_time_over_ecdsa_keyed_time"] = med("keyed_stream_form_16_bit") / med("yardstick_ecdsa_keyed_dev_16_bit")
    r["keyed_is_faster_than_generic"] = max(t_keyed) < min(t_generic) and max(t_keyed_w) < min(t_generic)
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
    n_keys = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    sbv.init(0)
    r = rates(n, n_keys)
    r["metric"] = "BIP-340 verifications/s against registered keys, device-resident, 8-bit combs, batch=%d" % n
    r["value"] = r["keyed_stream_form_8_bit"]["verifies_per_s"]
    r["unit"] = "verifies/s"
    print(json.dumps(r))
    assert r["keyed_is_faster_than_generic"], "the keyed verifier is not faster than the generic one"


if __name__ == "__main__":
    main()
