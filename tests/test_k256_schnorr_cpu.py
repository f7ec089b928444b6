"""CPU tier of the BIP-340 Schnorr entries over secp256k1 (include/sbv.h: sbv_secp256k1_schnorr_verify, _expand_keys, _sign;
consensus_amd/csrc/k256_schnorr.h).

tests/emul/k256_schnorr_emul.cc compiles the lanes the kernels are made of with g++, contract assertions on, and runs them as the
kernels do, the capped grid included (a few lanes over many items, so that strips are reused).  Every verdict, record and signature is
held byte for byte to the Python model of tests/k256_schnorr_cases.py, which reproduces the two known answers of
tests/golden/bip340.json; the host forms (k256_schnorr_*, sbvh_k256_schnorr_*, Verifier::VerifySchnorr and the backend's signer on the
CPU backend) are held to the same cases.  The same source, built as a program of its own with AddressSanitizer and UBSan, runs the
cases once."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import pytest

import hostlib
import k256_py as kp
import k256_schnorr_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "k256_schnorr_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
N, P = cases.N, cases.P


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


class Emul:
    """the emulator library behind the calling conventions of consensus_amd's wrappers"""

    def __init__(self):
        so = os.path.join(HERE, "emul", "libsbv_k256_schnorr_emul.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", "-DSBV_K256_CHECK",
                                   EMUL_SRC, "-o", so])
        lib = ctypes.CDLL(so)
        V, S, U, C = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p
        lib.sbvk256sch_verify.argtypes = [C, C, C, S, S, V]
        lib.sbvk256sch_verify.restype = None
        lib.sbvk256sch_expand.argtypes = [C, S, V, V, V]
        lib.sbvk256sch_expand.restype = None
        lib.sbvk256sch_sign.argtypes = [C, U, V, C, C, S, V, V]
        lib.sbvk256sch_sign.restype = None
        lib.sbvk256sch_op.argtypes = [ctypes.c_int, ctypes.c_int, C, V, S]
        self.lib = lib

    def verify(self, pks, msgs, sigs, lanes=1 << 17):
        n = len(sigs) // 64
        ok = ctypes.create_string_buffer(max(1, n))
        self.lib.sbvk256sch_verify(pks, msgs, sigs, n, lanes, ok)
        return ok.raw[:n]

    def expand(self, keys, want_pks=True):
        m = len(keys) // 32
        exp, pks, ok = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(32 * m), ctypes.create_string_buffer(m)
        self.lib.sbvk256sch_expand(keys, m, exp, pks if want_pks else None, ok)
        return exp.raw, pks.raw if want_pks else None, ok.raw

    def sign(self, expanded, msgs, aux=None, key_index=None):
        n = len(msgs) // 32
        sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
        idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
        self.lib.sbvk256sch_sign(expanded, len(expanded) // 64, idx, msgs, aux, n, sigs, ok)
        return sigs.raw, ok.raw

    def op(self, op, records, recovery=0):
        n = len(records)
        out = ctypes.create_string_buffer(cases.OP_OUT * n)
        assert self.lib.sbvk256sch_op(recovery, op, b"".join(records), out, n) == 0
        return [out.raw[cases.OP_OUT * i:cases.OP_OUT * (i + 1)] for i in range(n)]


@pytest.fixture(scope="module")
def emul():
    return Emul()


@pytest.fixture(scope="module")
def host():
    lib = hostlib.load()
    C = ctypes.c_char_p
    lib.sbvh_k256_schnorr_expand.argtypes = [C, C]
    lib.sbvh_k256_schnorr_sign.argtypes = [C, C, C, C]
    lib.sbvh_k256_schnorr_verify.argtypes = [C, C, C]
    lib.sbvh_verify_schnorr.argtypes = [hostlib.V, C, C, C, ctypes.c_size_t, C]
    lib.sbvh_sign_schnorr.argtypes = [hostlib.V, C, ctypes.c_uint32, ctypes.c_void_p, C, C, ctypes.c_size_t, C, C]
    return lib


def _bad_verdicts(got):
    exp = cases.expected_all()
    return [(i, cases.cases()[i][0]) for i in range(len(exp)) if got[i] != exp[i]]


# ---- the model and the case set -------------------------------------------------------------------------------------------------------
def test_the_model_reproduces_the_known_answers():
    vs = cases.vectors()
    assert len(vs) == 2
    for v in vs:
        rec, pk, ok = cases.expand(int.from_bytes(v["d"], "big"))
        assert ok == 1 and pk == v["pk"] == rec[32:]
        assert cases.sign(rec, v["msg"], v["aux"]) == (v["sig"], 1)
        assert cases.verify(v["pk"], v["msg"], v["sig"]) == 1
    h = hashlib.sha256(b"BIP0340/challenge").digest()
    assert h.hex().startswith("7bb52d7a9fef5832") and h.hex().endswith("6d48d37c")
    assert cases.tagged("BIP0340/challenge", b"abc") == hashlib.sha256(h + h + b"abc").digest()


def test_the_models_ladder_equals_the_oracles_multiplication():
    rng = random.Random(0x1ADDE2)
    for k in [1, 2, N - 1, 15, 16, 2**252] + [rng.randrange(1, N) for _ in range(12)]:
        pt = kp.pt_mul(rng.randrange(1, N), kp.G)
        assert cases.mul(k, pt) == kp.pt_mul(k, pt) and kp.on_curve(*cases.mul(k, pt))
    assert cases.mul(0, kp.G) is None and cases.mul(N, kp.G) is None and cases.gmul(6)[1] % 2 == 1


def test_the_case_set_has_every_category_and_every_parity():
    """the minimum counts of the categories: the set cannot degenerate silently"""
    tr = cases.triples()
    keys = [d for d, _, _ in tr]
    assert len(tr) == 300 and all(k in keys for k in cases.EDGE_KEYS + cases.REFUSED_KEYS)
    assert any(m == bytes(32) and a == bytes(32) for _, m, a in tr) and any(m == cases.FF and a == cases.FF for _, m, a in tr)
    assert cases.parity_coverage() == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert [ok for _, _, ok in cases.expanded()].count(0) == 3 and [ok for _, ok in cases.signed()].count(0) == 3
    c = cases.category_counts()
    assert c["valid"] == [0, 297] and c["vector"] == [0, 2] and c["vector_spoiled"] == [2, 0]
    for cat in ("msg_bit", "r_bit", "s_bit", "other_key", "neg_s"):
        assert c[cat] == [297, 0], cat
    assert c["parity"][1] == 0 and c["parity"][0] >= 100
    assert c["infinity"] == [4, 0] and c["r_off_curve"] == [4, 0] and c["s_zero"] == [1, 0] and c["range"] == [10, 0]
    assert c["pk_off_curve"] == [8, 0]
    assert sum(v[0] + v[1] for v in c.values()) == len(cases.cases())


def test_parity_and_infinity_cases_fail_for_their_reason_alone():
    """the model's R: the right x under an odd y for "parity"; no point at all for "infinity"; a point for the other rejected twins"""
    seen = {"parity": 0, "infinity": 0}
    for cat, pk, m, sig in cases.cases():
        if cat in seen:
            kind, R = cases.final_point(pk, m, sig)
            assert kind == "point"
            if cat == "parity":
                assert R[0] == int.from_bytes(sig[:32], "big") and R[1] % 2 == 1
            else:
                assert R is None
            seen[cat] += 1
    assert seen["parity"] >= 100 and seen["infinity"] == 4
    assert cases.lift_x(0) is None and pow(7, (P - 1) // 2, P) == P - 1          # pk = 0: 7 is a non-residue


# ---- the emulated lanes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1 << 17, 7, 64])
def test_emulated_verifier_equals_the_model(emul, lanes):
    bad = _bad_verdicts(emul.verify(*cases.arrays(), lanes))
    assert not bad, (len(bad), bad[:8])


def test_emulated_expansion_equals_the_model(emul):
    exp, pks, ok = emul.expand(cases.key_blob())
    want = cases.expanded()
    assert exp == b"".join(w[0] for w in want) and pks == b"".join(w[1] for w in want) and ok == bytes(w[2] for w in want)
    assert emul.expand(cases.key_blob(), want_pks=False)[0] == exp
    refused = [i for i, w in enumerate(want) if not w[2]]
    assert len(refused) == 3 and all(exp[64 * i:64 * i + 64] == bytes(64) for i in refused)


def test_emulated_signer_equals_the_model(emul):
    tr = cases.triples()
    recs = b"".join(w[0] for w in cases.expanded())
    msgs, aux = b"".join(t[1] for t in tr), b"".join(t[2] for t in tr)
    sigs, ok = emul.sign(recs, msgs, aux)
    assert sigs == b"".join(s for s, _ in cases.signed()) and ok == bytes(o for _, o in cases.signed())
    # aux = NULL is the zero aux, and differs from a given aux
    sigs0, ok0 = emul.sign(recs, msgs, None)
    assert sigs0 == b"".join(s for s, _ in cases.signed(True)) and ok0 == ok and sigs0 == emul.sign(recs, msgs, bytes(len(aux)))[0] and sigs0 != sigs
    # the index rule: explicit indices, an index out of range, fewer keys than messages
    idx, m2, a2, s2, o2 = cases.tiled_sign(337, 5)
    assert emul.sign(recs, m2, a2, idx) == (s2, o2)
    idx[3], idx[100] = len(tr), 2**32 - 1
    s3, o3 = emul.sign(recs, m2, a2, idx)
    assert o3[3] == o3[100] == 0 and s3[64 * 3:64 * 4] == s3[6400:6464] == bytes(64)
    assert s3[:192] == s2[:192] and s3[256:6400] == s2[256:6400] and s3[6464:] == s2[6464:]
    few = recs[64 * 8:64 * 11]
    s4, o4 = emul.sign(few, msgs[:32 * 10], aux[:32 * 10])
    for i in range(10):
        assert (s4[64 * i:64 * i + 64], o4[i]) == cases.sign(few[64 * (i % 3):64 * (i % 3) + 64], msgs[32 * i:32 * i + 32], aux[32 * i:32 * i + 32])


def test_known_answers_through_every_form(emul, host):
    for v in cases.vectors():
        exp, pks, ok = emul.expand(v["d"])
        assert ok == b"\x01" and pks == v["pk"]
        assert emul.sign(exp, v["msg"], v["aux"]) == (v["sig"], b"\x01")
        assert emul.verify(v["pk"], v["msg"], v["sig"], 1) == b"\x01"
        spoiled = v["sig"][:5] + bytes([v["sig"][5] ^ 0x10]) + v["sig"][6:]
        assert emul.verify(v["pk"], v["msg"], spoiled, 1) == b"\x00"
        rec, sig = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        assert host.sbvh_k256_schnorr_expand(v["d"], rec) == 0 and rec.raw == exp
        assert host.sbvh_k256_schnorr_sign(rec.raw, v["msg"], v["aux"], sig) == 0 and sig.raw == v["sig"]
        assert host.sbvh_k256_schnorr_verify(v["pk"], v["msg"], v["sig"]) == 0
        assert host.sbvh_k256_schnorr_verify(v["pk"], v["msg"], spoiled) == -1
    v = cases.vectors()[0]                         # vector 0 has the zero aux: the null pointer signs the same bytes
    rec, sig = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    assert host.sbvh_k256_schnorr_expand(v["d"], rec) == 0 and host.sbvh_k256_schnorr_sign(rec.raw, v["msg"], None, sig) == 0 and sig.raw == v["sig"]


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_unit_operations_against_python(emul, op):
    ins, want = cases.all_op_cases()[op]
    got = emul.op(op, ins)
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (op, len(bad), bad[:8])
    assert emul.lib.sbvk256sch_op(0, 4, ins[0], ctypes.create_string_buffer(cases.OP_OUT), 1) != 0
    assert emul.lib.sbvk256sch_op(0, -1, ins[0], ctypes.create_string_buffer(cases.OP_OUT), 1) != 0


def test_the_unit_operation_cases_have_both_sides():
    for op, (ins, outs) in enumerate(cases.all_op_cases()):
        n_ok = sum(o[-1] for o in outs)
        assert n_ok >= 20 and (op == 0 or len(outs) - n_ok >= 3), (op, n_ok, len(outs))
    ins, outs = cases.walk_cases()
    assert sum(1 - o[-1] for o in outs) == 6 and len(outs) == 48


def test_the_walk_with_a_zero_scalar(emul):
    """op 2 of the recovery's unit operations: u2 = 0 (new with this scheme), u1 = 0, and both (infinity)"""
    ins, want = cases.walk_cases()
    got = emul.op(2, ins, recovery=1)
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


# ---- the host forms -------------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_model(host):
    rec, sig = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    for (d, m, a), (wrec, _, wok), (wsig, wsok), (wsig0, _) in zip(cases.triples(), cases.expanded(), cases.signed(), cases.signed(True)):
        rc = host.sbvh_k256_schnorr_expand(cases.be32(d), rec)
        assert (rec.raw, 1 if rc == 0 else 0) == (wrec, wok), d
        rc = host.sbvh_k256_schnorr_sign(rec.raw, m, a, sig)
        assert (sig.raw, 1 if rc == 0 else 0) == (wsig, wsok), d
        rc = host.sbvh_k256_schnorr_sign(rec.raw, m, None, sig)
        assert (sig.raw, 1 if rc == 0 else 0) == (wsig0, wsok), d
    exp = cases.expected_all()
    seen = [0, 0]
    for i, (cat, pk, m, s) in enumerate(cases.cases()):
        assert (1 if host.sbvh_k256_schnorr_verify(pk, m, s) == 0 else 0) == exp[i], (i, cat)
        seen[exp[i]] += 1
    assert seen[1] >= 299 and seen[0] >= 1600


def test_verify_schnorr_and_the_signer_on_the_cpu_backend(host):
    """Verifier::VerifySchnorr and Backend::schnorr_sign_k256 on a backend without a device: the CPU loop; only under Scheme::SECP256K1"""
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    pks, msgs, sigs = cases.arrays()
    n = len(sigs) // 64
    h = host.sbvh_verifier_new_scheme(2, 1, 0, cb, None, 64, 50, 0)
    try:
        ok = ctypes.create_string_buffer(n)
        assert host.sbvh_verify_schnorr(h, pks, msgs, sigs, n, ok) == hostlib.OK
        assert not _bad_verdicts(ok.raw)
        assert host.sbvh_verify_schnorr(h, pks, msgs, sigs, 0, ok) == hostlib.OK
        assert host.sbvh_verify_schnorr(h, None, msgs, sigs, 1, ok) == hostlib.INVALID
        recs = b"".join(w[0] for w in cases.expanded())
        idx, m2, a2, s2, o2 = cases.tiled_sign(700, 3)
        idx[9] = 300
        out, sok = ctypes.create_string_buffer(64 * 700), ctypes.create_string_buffer(700)
        assert host.sbvh_sign_schnorr(h, recs, 300, (ctypes.c_uint32 * 700)(*idx), m2, a2, 700, out, sok) == 0
        assert out.raw[:576] == s2[:576] and out.raw[576:640] == bytes(64) and sok.raw[9] == 0 and out.raw[640:] == s2[640:]
        assert sok.raw[:9] == o2[:9] and sok.raw[10:] == o2[10:]
        assert host.sbvh_sign_schnorr(h, recs, 0, None, m2, a2, 700, out, sok) != 0
        msgs0 = b"".join(t[1] for t in cases.triples())                # no index, no aux: key i % n_keys and the zero aux
        assert host.sbvh_sign_schnorr(h, recs, 300, None, msgs0, None, 300, out, sok) == 0
        assert out.raw[:64 * 300] == b"".join(s for s, _ in cases.signed(True)) and sok.raw[:300] == bytes(o for _, o in cases.signed(True))
    finally:
        host.sbvh_verifier_free(h)
    h = host.sbvh_verifier_new_scheme(0, 1, 0, cb, None, 64, 50, 0)      # a P-256 Verifier has no Schnorr entry
    try:
        assert host.sbvh_verify_schnorr(h, pks, msgs, sigs, 1, ctypes.create_string_buffer(1)) == hostlib.INVALID
    finally:
        host.sbvh_verifier_free(h)


# ---- the layers above -----------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("sbv_secp256k1_schnorr_verify", "sbv_secp256k1_schnorr_verify_workspace", "sbv_secp256k1_schnorr_verify_stream",
               "sbv_secp256k1_schnorr_expand_keys", "sbv_secp256k1_schnorr_expand_keys_stream", "sbv_secp256k1_schnorr_sign",
               "sbv_secp256k1_schnorr_sign_stream", "sbv_debug_secp256k1_schnorr_op")


def test_header_declares_the_entries_and_the_wrappers_exist():
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    for name in NEW_ENTRIES:
        assert "\n" + name + "(" in hdr, name                          # the return type stands on a line of its own
    assert hdr.count("int sbv_secp256k1_") == 12                       # what tests/test_k256_keyed_cpu.py counts: one-line prototypes
    assert "_schnorr_verify_dev" not in hdr and "_schnorr_sign_dev" not in hdr
    assert "AS SECRET AS ITS KEY" in hdr and "can leak d" in hdr and "NOT constant-time" in hdr
    import consensus_amd as sbv
    for name in NEW_ENTRIES:
        py = name[4:] if not name.startswith("sbv_debug") else name[4:]
        assert callable(getattr(sbv, py)), py
    api = open(os.path.join(CSRC, "sbv_api.hip")).read()
    for name in NEW_ENTRIES:
        assert 'extern "C"' in api and name + "(" in api, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(BUILD)/k256_schnorr_kernels.o" in mk
    lib = sbv.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name                                # exported by the built library


def test_cgo_call_sites_match_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    seen, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    called = {name for fn in os.listdir(go) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(go, fn)).read())}
    assert {"sbv_secp256k1_schnorr_verify", "sbv_secp256k1_schnorr_expand_keys", "sbv_secp256k1_schnorr_sign"} <= called
    u8, u32, V, S = ("uint8_t", True), ("uint32_t", False), ("void", True), ("size_t", False)
    assert protos["sbv_secp256k1_schnorr_verify"] == [u8, u8, u8, S, u8]
    assert protos["sbv_secp256k1_schnorr_verify_workspace"] == [S]
    assert protos["sbv_secp256k1_schnorr_verify_stream"] == [V, V, V, S, V, V, S, V]
    assert protos["sbv_secp256k1_schnorr_expand_keys"] == [u8, S, u8, u8, u8]
    assert protos["sbv_secp256k1_schnorr_expand_keys_stream"] == [V, S, V, V, V, V]
    assert protos["sbv_secp256k1_schnorr_sign"] == [u8, u32, ("uint32_t", True), u8, u8, S, u8, u8]
    assert protos["sbv_secp256k1_schnorr_sign_stream"] == [V, u32, V, V, V, S, V, V, V]
    assert protos["sbv_debug_secp256k1_schnorr_op"] == [("int", False), u8, u8, S]
    src = open(os.path.join(go, "backend.go")).read()
    assert "type K256Schnorr interface" in src and "VerifyBatchSchnorr(" in src and "SignBatchSchnorr(" in src


def test_every_new_entry_refuses_without_a_device():
    import consensus_amd as sbv
    lib = sbv.load()
    assert lib.sbv_init(0) == -1                    # SBV_ENODEV: after it every entry refuses as its siblings do
    buf = ctypes.create_string_buffer(192)
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_verify(bytes(32), bytes(32), bytes(64))
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_verify_stream(ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf), 1, ctypes.addressof(buf),
                                            ctypes.addressof(buf), 1536)
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_expand_keys(bytes(31) + b"\x01")
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_expand_keys_stream(ctypes.addressof(buf), 1, ctypes.addressof(buf), 0, ctypes.addressof(buf))
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_sign(bytes(64), bytes(32))
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_sign_stream(ctypes.addressof(buf), 1, 0, ctypes.addressof(buf), 0, 1, ctypes.addressof(buf), ctypes.addressof(buf))
    with pytest.raises(sbv.SbvError):
        sbv.debug_secp256k1_schnorr_op(0, [bytes(192)])
    # the workspace size needs no device: min(n, LANES) strips of 1 536 bytes
    assert [sbv.secp256k1_schnorr_verify_workspace(n) for n in (0, 1, 1000, 1 << 17, (1 << 17) + 1, 1 << 20)] == \
        [0, 1536, 1536000, 1536 << 17, 1536 << 17, 1536 << 17]


def test_sanitizer_build_runs_the_cases_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan: every verification case with 5 lanes (strips reused) and with
    one lane per case, on exactly allocated strips; every triple expanded, signed (aux given, zero and null) and verified; one run"""
    exe = str(tmp_path / "k256_schnorr_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-DSBV_K256_CHECK", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    rows = ["V %s %s %s %02x" % (pk.hex(), m.hex(), s.hex(), ok) for (_, pk, m, s), ok in zip(cases.cases(), cases.expected_all())]
    for (d, m, a), (rec, _, ok), (sig, _) in zip(cases.triples(), cases.expanded(), cases.signed()):
        rows.append("S %s %s %s %s %s" % (cases.be32(d).hex(), m.hex(), a.hex(), rec.hex() if ok else "-", sig.hex() if ok else "-"))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(rows) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases," % len(rows) in r.stdout and " 0 differ" in r.stdout, r.stdout + r.stderr
