"""CPU tier of the secp256k1 public-key recovery (include/sbv.h: sbv_secp256k1_recover; consensus_amd/csrc/k256_recover.h).

tests/emul/k256_recover_emul.cc compiles the lanes the kernels are made of with g++, contract assertions on, and runs them as the
kernels do, the capped grid included (a few lanes over many items, so that strips are reused).  Every key is held byte for byte to the
Python-integer model of tests/k256_recover_cases.py; the host form (k256_recover, sbvh_k256_recover, Verifier::RecoverSigners on the
CPU backend) is held to the same cases; the C oracle and OpenSSL accept every recovered key with its signature.  The same source,
built as a program of its own with AddressSanitizer and UBSan, runs the cases once."""
import ctypes
import os
import subprocess
import sys

import pytest

import hostlib
import k256_py as kp
import k256_recover_cases as cases
import k256_sign_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "k256_recover_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
N, P, LOW_S = cases.N, cases.P, cases.LOW_S


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


class Emul:
    """the emulator library behind the calling conventions of consensus_amd's wrappers"""

    def __init__(self):
        so = os.path.join(HERE, "emul", "libsbv_k256_recover_emul.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", "-DSBV_K256_CHECK",
                                   EMUL_SRC, "-o", so])
        lib = ctypes.CDLL(so)
        V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        lib.sbvk256rec_recover.argtypes = [ctypes.c_char_p] * 3 + [S, U, S, V, V]
        lib.sbvk256rec_recover.restype = None
        lib.sbvk256rec_op.argtypes = [ctypes.c_int, ctypes.c_char_p, V, S]
        self.lib = lib

    def recover(self, sigs, recid, digests, flags=0, lanes=1 << 17):
        n = len(recid)
        pubs, ok = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
        self.lib.sbvk256rec_recover(sigs, recid, digests, n, flags, lanes, pubs, ok)
        return pubs.raw[:64 * n], ok.raw[:n]

    def op(self, op, records):
        n = len(records)
        out = ctypes.create_string_buffer(cases.OP_OUT * n)
        assert self.lib.sbvk256rec_op(op, b"".join(records), out, n) == 0
        return [out.raw[cases.OP_OUT * i:cases.OP_OUT * (i + 1)] for i in range(n)]


@pytest.fixture(scope="module")
def emul():
    return Emul()


def _differ(idx, pubs, ok):
    exp = cases.expected_all()
    return [(i, cases.cases()[i][0]) for k, i in enumerate(idx) if (pubs[64 * k:64 * k + 64], ok[k]) != exp[i]]


def test_the_case_set_has_every_category_on_both_sides():
    """the minimum counts of the categories: the set cannot degenerate silently"""
    c = cases.category_counts()
    m = len(sc.sign_cases())
    assert m == 320 and c["signed"] == [0, 2 * m] and c["twin"] == [0, 2 * m]
    assert c["refused"][1] == 0 and c["refused"][0] >= 7 + 5 + 50 + 4
    assert c["high_s_allowed"] == [0, 4]
    assert c["plus_n"][0] == 0 and c["plus_n"][1] >= 9
    assert c["infinity"] == [4, 0] and c["near_infinity"] == [0, 12]
    assert c["digest_edge"] == [0, 2 * len(sc.EDGE_DIGESTS)]
    assert c["scalar_edge"][0] == 2 and c["scalar_edge"][1] >= 6 + 12 + 6 + 8          # refused: s = n - 1 and (n + 1) / 2 under low-S
    for flags in (0, LOW_S):                                                          # both calls see both verdicts
        oks = [cases.expected_all()[i][1] for i in cases.by_flags(flags)[0]]
        assert min(oks) == 0 and max(oks) == 1
    for op, (ins, outs) in enumerate(cases.all_op_cases()):
        n_ok = sum(o[-1] for o in outs)
        assert n_ok >= 10 and len(outs) - n_ok >= 10, (op, n_ok, len(outs))
    ins, outs = cases.op0_cases()
    assert sum(o[-1] for o in outs) >= 50 + 5 and sum(1 - o[-1] for o in outs) >= 50


def test_signed_cases_recover_the_signers_key_and_twins_another():
    """the model itself: d G from every signature and its id, and under the other parity a different key (that it verifies too is
    test_the_c_oracle_and_openssl_accept_every_recovered_key)"""
    cs, exp, pubs = cases.cases(), cases.expected_all(), cases.signer_pubs()
    m = len(pubs)
    k = 0
    for i, c in enumerate(cs):
        if c[0] == "signed":
            assert exp[i] == (pubs[k % m], 1), i
            assert cs[i + 1][0] == "twin" and exp[i + 1][1] == 1 and exp[i + 1][0] != pubs[k % m], i
            k += 1
    assert k == 2 * m


@pytest.mark.parametrize("flags", [0, LOW_S])
@pytest.mark.parametrize("lanes", [1 << 17, 7, 64])
def test_emulator_equals_the_model(emul, flags, lanes):
    idx, sigs, rid, digs = cases.by_flags(flags)
    pubs, ok = emul.recover(sigs, rid, digs, flags, lanes)
    bad = _differ(idx, pubs, ok)
    assert not bad, (len(bad), bad[:8])


def test_refused_lanes_write_zeros(emul):
    idx, sigs, rid, digs = cases.by_flags(0)
    pubs, ok = emul.recover(sigs, rid, digs, 0, 5)
    refused = [k for k in range(len(idx)) if not ok[k]]
    assert len(refused) >= 60 and all(pubs[64 * k:64 * k + 64] == bytes(64) for k in refused)


@pytest.mark.parametrize("op", [0, 1, 2])
def test_unit_operations_against_python(emul, op):
    ins, want = cases.all_op_cases()[op]
    got = emul.op(op, ins)
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (op, len(bad), bad[:8])
    assert emul.lib.sbvk256rec_op(3, ins[0], ctypes.create_string_buffer(cases.OP_OUT), 1) != 0
    assert emul.lib.sbvk256rec_op(-1, ins[0], ctypes.create_string_buffer(cases.OP_OUT), 1) != 0


def test_sqrt_returns_a_root_of_every_residue_and_refuses_the_rest(emul):
    """independent of the model's choice of root: y^2 = a, and ok exactly for the squares"""
    ins, _ = cases.op0_cases()
    for rec, out in zip(ins, emul.op(0, ins)):
        a = int.from_bytes(rec[:32], "big") % P
        y = int.from_bytes(out[:32], "big")
        if pow(a, (P - 1) // 2, P) in (0, 1):
            assert out[-1] == 1 and y < P and y * y % P == a
        else:
            assert out == bytes(cases.OP_OUT)


def test_host_form_equals_the_model():
    host = hostlib.load()
    host.sbvh_k256_recover.argtypes = [ctypes.c_char_p, ctypes.c_uint8, ctypes.c_char_p, ctypes.c_char_p]
    q = ctypes.create_string_buffer(64)
    exp = cases.expected_all()
    seen = [0, 0]
    for i, (cat, rs, rid, h, flags) in enumerate(cases.cases()):
        if flags:
            continue                                                    # the host form has no low-S rule: flags = 0
        rc = host.sbvh_k256_recover(rs, min(rid, 255), h, q)
        assert (q.raw, 1 if rc == 0 else 0) == exp[i], (i, cat)
        seen[exp[i][1]] += 1
    assert seen[0] >= 60 and seen[1] >= 600


def test_recover_signers_on_the_cpu_backend():
    """Verifier::RecoverSigners: 65-byte r | s | v with v as 0..3 and as 27..30, any other v refused; only under Scheme::SECP256K1"""
    host = hostlib.load()
    host.sbvh_recover_signers.argtypes = [hostlib.V, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    idx, sigs, rid, digs = cases.by_flags(0)
    exp = cases.expected_all()
    n = len(idx)
    for shift in (0, 27):
        blob = b"".join(sigs[64 * k:64 * k + 64] + bytes([rid[k] + shift if rid[k] <= 3 else rid[k]]) for k in range(n))
        h = host.sbvh_verifier_new_scheme(2, 1, 0, cb, None, 64, 50, 0)
        try:
            pubs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
            assert host.sbvh_recover_signers(h, blob, digs, n, pubs, ok) == hostlib.OK
            assert not _differ(idx, pubs.raw, ok.raw)
            for v in (4, 26, 31, 200):                                  # a valid signature under a v that names no id
                one = sigs[:64] + bytes([v])
                assert host.sbvh_recover_signers(h, one, digs[:32], 1, pubs, ok) == hostlib.OK and ok.raw[0] == 0 and pubs.raw[:64] == bytes(64)
            assert host.sbvh_recover_signers(h, blob, digs, 0, pubs, ok) == hostlib.OK
        finally:
            host.sbvh_verifier_free(h)
    h = host.sbvh_verifier_new_scheme(0, 1, 0, cb, None, 64, 50, 0)      # a P-256 Verifier has no recovery
    try:
        assert host.sbvh_recover_signers(h, sigs[:64] + b"\x00", digs[:32], 1, ctypes.create_string_buffer(64), ctypes.create_string_buffer(1)) == hostlib.INVALID
    finally:
        host.sbvh_verifier_free(h)


def test_the_c_oracle_and_openssl_accept_every_recovered_key(emul, oracle, openssl_check):
    """every recovered key with its signature, twins, the + n branch and the edges included; and not under another digest"""
    oracle.sbvo_k256_verify_tuple.argtypes = [ctypes.c_char_p]
    openssl_check.sbvssl_k256_verify_tuple.argtypes = [ctypes.c_char_p]
    checked = 0
    for flags in (0, LOW_S):
        idx, sigs, rid, digs = cases.by_flags(flags)
        pubs, ok = emul.recover(sigs, rid, digs, flags, 11)
        for k, i in enumerate(idx):
            if not ok[k]:
                continue
            t = sigs[64 * k:64 * k + 64] + digs[32 * k:32 * k + 32] + pubs[64 * k:64 * k + 64]
            assert oracle.sbvo_k256_verify_tuple(t) == 1 and openssl_check.sbvssl_k256_verify_tuple(t) == 1, (i, cases.cases()[i][0])
            if k % 8 == 0:
                h2 = bytes([t[64] ^ 1]) + t[65:96]
                assert oracle.sbvo_k256_verify_tuple(t[:64] + h2 + t[96:]) == 0, i
            checked += 1
    assert checked >= 1300


def test_plus_n_cases_take_the_verifiers_wraps_branch():
    """r + n < p, and the x of the verifier's point is r + n: the model's verifier accepts only through R.x mod n = r with R.x >= n"""
    seen = 0
    for (cat, rs, rid, h, _), (pub, ok) in zip(cases.cases(), cases.expected_all()):
        if cat != "plus_n":
            continue
        r, s = int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big")
        assert ok and rid & 2 and r + N < P
        q = (int.from_bytes(pub[:32], "big"), int.from_bytes(pub[32:], "big"))
        w = pow(s, -1, N)
        R = kp.pt_add(kp.pt_mul(int.from_bytes(h, "big") % N * w % N, kp.G), kp.pt_mul(r * w % N, q))
        assert R[0] == r + N
        seen += 1
    assert seen >= 9


def test_header_declares_the_entries_and_the_wrappers_exist():
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    for name in ("sbv_secp256k1_recover(", "sbv_secp256k1_recover_workspace(", "sbv_secp256k1_recover_stream(", "sbv_debug_secp256k1_recover_op(",
                 "SBV_K256_RECOVER_LOW_S 1u", "SBV_K256_RECOVER_LANES"):
        assert name in hdr, name
    assert hdr.count("int sbv_secp256k1_") == 12                        # what tests/test_k256_keyed_cpu.py counts: one-line prototypes
    import consensus_amd as sbv
    for name in ("secp256k1_recover", "secp256k1_recover_workspace", "secp256k1_recover_stream", "debug_secp256k1_recover_op"):
        assert callable(getattr(sbv, name)), name
    assert sbv.K256_RECOVER_LOW_S == 1
    api = open(os.path.join(CSRC, "sbv_api.hip")).read()
    for name in ("sbv_secp256k1_recover", "sbv_secp256k1_recover_workspace", "sbv_secp256k1_recover_stream", "sbv_debug_secp256k1_recover_op"):
        assert 'extern "C"' in api and name + "(" in api, name


def test_cgo_call_site_matches_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    seen, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    called = {name for fn in os.listdir(go) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(go, fn)).read())}
    assert "sbv_secp256k1_recover" in called
    u8, u32, V, S = ("uint8_t", True), ("uint32_t", False), ("void", True), ("size_t", False)
    assert protos["sbv_secp256k1_recover"] == [u8, u8, u8, S, u32, u8, u8]
    assert protos["sbv_secp256k1_recover_workspace"] == [S]
    assert protos["sbv_secp256k1_recover_stream"] == [V, V, V, S, u32, V, V, V, S, V]
    assert protos["sbv_debug_secp256k1_recover_op"] == [("int", False), u8, u8, S]
    src = open(os.path.join(go, "backend.go")).read()
    assert "type K256BatchRecoverer interface" in src and "RecoverBatchSecp256k1(" in src


def test_sanitizer_build_recovers_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan: every case with 5 lanes (strips reused) and with one lane per
    case, on exactly allocated strips, and the unit operations, one run"""
    exe = str(tmp_path / "k256_recover_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-DSBV_K256_CHECK", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    rows = []
    for (cat, rs, rid, h, flags), (pub, ok) in zip(cases.cases(), cases.expected_all()):
        rows.append((rs.hex(), "%02x" % min(rid, 255), h.hex(), "%02x" % flags, pub.hex() if ok else "-"))
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(r) + "\n" for r in rows))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases," % len(rows) in r.stdout and " 0 differ" in r.stdout, r.stdout + r.stderr
