"""CPU tier of the SEC1 key decoders (include/sbv.h: sbv_p256_decode_keys, sbv_secp256k1_decode_keys, the _sec1 verify entries;
consensus_amd/csrc/sec1_keys.h).

tests/emul/sec1_emul.cc compiles the lanes the kernels are made of with g++, the contract assertions of both fields on
(-DSBV_F29_CHECK: every operand of every f29 product along the 253-deep squaring chain; -DSBV_K256_CHECK), and runs them as the kernels
do.  Every key is held byte for byte to the Python-integer model of tests/sec1_cases.py, in both packings and under offset tables with
spoiled entries; the host forms (p256_sec1_decode, k256_sec1_decode, Verifier::DecodeKeys and the SEC1 registration path) are held to
the same cases; OpenSSL decodes every case that starts with 02 / 03 / 04 to the same point or refuses it too, and the C oracles and
OpenSSL judge the verify cases under the decoded keys.  The same source, built as a program of its own with AddressSanitizer and UBSan,
decodes every key from a heap block of exactly its length."""
import ctypes
import ctypes.util
import os
import subprocess
import sys

import pytest

import frontend_cases as fc
import hostlib
import msgs_generic_cases as mg
import sec1_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "sec1_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
IDS = [c.name for c in cases.CURVES]
CHECKS = ["-DSBV_K256_CHECK", "-DSBV_F29_CHECK"]


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


class Emul:
    def __init__(self):
        so = os.path.join(HERE, "emul", "libsbv_sec1_emul.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation"] + CHECKS + [EMUL_SRC, "-o", so])
        lib = ctypes.CDLL(so)
        C, V, S = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t
        lib.sbvsec1_decode.argtypes = [ctypes.c_int, C, V, ctypes.c_uint64, S, V, V]
        lib.sbvsec1_decode_one.argtypes = [ctypes.c_int, C, S, V]
        lib.sbvsec1_op.argtypes = [ctypes.c_int, ctypes.c_int, C, V, S]
        self.lib = lib

    def decode(self, cv, blob, off, m, key_bytes=None, want_ok=True):
        ko = (ctypes.c_uint64 * (m + 1))(*off) if off is not None else None
        keys64, ok = ctypes.create_string_buffer(max(1, 64 * m)), ctypes.create_string_buffer(max(1, m))
        assert self.lib.sbvsec1_decode(cv.id, blob, ko, len(blob) if key_bytes is None else key_bytes, m, keys64, ok if want_ok else None) == 0
        return keys64.raw[:64 * m], ok.raw[:m]

    def op(self, cv, op, records):
        n = len(records)
        out = ctypes.create_string_buffer(cases.OP_OUT * n)
        assert self.lib.sbvsec1_op(cv.id, op, b"".join(records), out, n) == 0
        return [out.raw[cases.OP_OUT * i:cases.OP_OUT * (i + 1)] for i in range(n)]


@pytest.fixture(scope="module")
def emul():
    return Emul()


def _differ(cv, idx, keys64, ok):
    cs, ex = cases.cases(cv), cases.expected(cv)
    return [(i, cs[i][0]) for k, i in enumerate(idx) if (keys64[64 * k:64 * k + 64], ok[k]) != ex[i]]


# ---- the case set and the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_the_case_set_has_every_category_on_both_sides(cv):
    cs, ex = cases.cases(cv), cases.expected(cv)
    by = dict(zip((n for n, _ in cs), ex))
    pts, non = cases.drawn(cv)
    assert len(pts) == 300 and len(non) >= 200                                  # both kinds of x, decided by the model
    for i in range(300):
        a, b, c = by["pt%d_02" % i], by["pt%d_03" % i], by["pt%d_04" % i]
        assert a[1] == b[1] == c[1] == 1 and a[0][:32] == b[0][:32] == c[0][:32]
        ya, yb = int.from_bytes(a[0][32:], "big"), int.from_bytes(b[0][32:], "big")
        assert ya % 2 == 0 and yb % 2 == 1 and ya + yb == cv.p and c[0] in (a[0], b[0])          # the wrong prefix: the negated y, not a refusal
    assert all(by["non%d_%s" % (i, pre)] == (cases.ZERO64, 0) for i in range(len(non)) for pre in ("02", "03"))
    for x in (cv.p, cv.p + 1, 2**256 - 1):
        assert all(by["x_edge_%x_%s" % (x, pre)][1] == 0 for pre in ("02", "03", "04"))
    assert {by["x_edge_%x_02" % x][1] for x in (0, 1, 2, 3, cv.p - 2, cv.p - 1)} == {0, 1}
    assert all(by["pt%d_y_negated" % i][1] == 1 and by["pt%d_y_plus_1" % i][1] == 0 for i in range(40))
    assert by["y_eq_1"][1] == 1 and by["y_eq_1_plus_p"] == (cases.ZERO64, 0) and by["y_eq_1_compressed"] == by["y_eq_1"]
    assert all(by["small%d_04" % i][1] == 1 and by["small%d_x_plus_p_04" % i][1] == 0 and by["small%d_x_plus_p_02" % i][1] == 0 for i in range(12))
    assert [pre for pre in range(256) if by["prefix_%02x_len33" % pre][1]] == [2, 3]
    assert [pre for pre in range(256) if by["prefix_%02x_len65" % pre][1]] == [4]
    assert [n for n in range(71) if by["len%d_02" % n][1]] == [33] and [n for n in range(71) if by["len%d_04" % n][1]] == [65]
    assert by["zero_zero"] == (cases.ZERO64, 0) and by["infinity"] == (cases.ZERO64, 0)
    assert all(xy == cases.ZERO64 for xy, ok in ex if not ok) and len(cs) <= 8229
    # every wavefront of the mixed packing holds all three kinds
    idx = cases.mixed(cv)[0]
    kinds = [cases.kind(cs[i][1]) for i in idx]
    assert sorted(idx) == list(range(len(cs))) and all(set(kinds[w:w + 64]) == {0, 1, 2} for w in range(0, len(kinds) - 63))
    for op in (0, 1):
        outs = cases.op_cases(cv, op)[1]
        assert sum(o[-1] for o in outs) >= 100 and sum(1 - o[-1] for o in outs) >= 100


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_known_answers_against_the_model_and_the_python_twins(cv):
    g = cases.golden_cases(cv)
    assert len(g) == (4 if cv.name == "p256" else 6)
    for name, key, xy in g:
        assert cases.decode(cv, key) == (xy, 1), name
        assert fc.CURVES[cv.name].mod.on_curve(int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big")), name
    by = {k["name"]: k for k in cases.golden()}
    assert by["p256_base_point"]["compressed"][:2] == "03" and by["k256_base_point"]["compressed"][:2] == "02"
    mod = fc.CURVES["k256"].mod
    for d in (1, 2, 3):
        x, y = mod.pt_mul(d, mod.G)
        k = by["k256_base_point" if d == 1 else "k256_d%d" % d]
        assert (int(k["x"], 16), int(k["y"], 16)) == (x, y)
    import json
    rfc = json.load(open(os.path.join(HERE, "golden", "rfc6979_p256.json")))
    assert (by["rfc6979_a25"]["x"], by["rfc6979_a25"]["y"]) == (rfc["qx"].lower(), rfc["qy"].lower())


# ---- the lanes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_emulator_equals_the_model_in_both_packings(emul, cv):
    idx, blob, off = cases.mixed(cv)
    keys64, ok = emul.decode(cv, blob, off, len(idx))
    bad = _differ(cv, idx, keys64, ok)
    assert not bad, (len(bad), bad[:8])
    assert emul.decode(cv, blob, off, len(idx), want_ok=False)[0] == keys64
    idx, blob = cases.stride(cv)
    keys64, ok = emul.decode(cv, blob, None, len(idx))
    bad = _differ(cv, idx, keys64, ok)
    assert not bad, (len(bad), bad[:8])
    # the stride against a key_bytes that ends inside key 100
    n, cover = 130, 100 * 33 + 32
    assert emul.decode(cv, blob[:33 * n], None, n, key_bytes=cover) == cases.decode_packed(cv, blob[:33 * n], None, n, key_bytes=cover, stride33=True)


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_bad_offset_pairs_refuse_their_lanes_and_no_other(emul, cv):
    blob, off, spoiled = cases.broken_offsets(cv)
    m = len(off) - 1
    want = cases.decode_packed(cv, blob, off, m)
    assert [i for i in range(m) if not want[1][i]] == list(spoiled)
    assert emul.decode(cv, blob, off, m) == want


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_unit_operations_against_python(emul, cv, op):
    ins, want = cases.op_cases(cv, op)
    got = emul.op(cv, op, ins)
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (cv.name, op, len(bad), bad[:8])
    out = ctypes.create_string_buffer(cases.OP_OUT)
    for curve, o in ((cv.id, 2), (cv.id, -1), (2, 0), (-1, 0)):
        assert emul.lib.sbvsec1_op(curve, o, ins[0], out, 1) != 0


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_sqrt_returns_a_root_of_every_residue_and_refuses_the_rest(emul, cv):
    """independent of the model's choice of root: y^2 = a, and ok exactly for the squares (Euler's criterion)"""
    ins, _ = cases.op_cases(cv, 0)
    for rec, out in zip(ins, emul.op(cv, 0, ins)):
        a = int.from_bytes(rec[:32], "big") % cv.p
        y = int.from_bytes(out[:32], "big")
        if pow(a, (cv.p - 1) // 2, cv.p) in (0, 1):
            assert out[-1] == 1 and y < cv.p and y * y % cv.p == a
        else:
            assert out == bytes(cases.OP_OUT)


# ---- the host forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_host_forms_equal_the_model(cv):
    host = hostlib.load()
    fn = host.sbvh_p256_sec1_decode if cv.name == "p256" else host.sbvh_k256_sec1_decode
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    out = ctypes.create_string_buffer(64)
    for (name, key), want in zip(cases.cases(cv), cases.expected(cv)):
        rc = fn(key, len(key), out)
        assert (out.raw, 1 if rc == 0 else 0) == want, name
    assert fn(None, 0, out) == -1 and out.raw == cases.ZERO64


def _oracle_callback(scheme, seen):
    o = fc.oracle()
    fn = getattr(o, "sbvo_%s_verify_tuple" % scheme)
    fn.argtypes = [ctypes.c_char_p]

    def cb(tuples, n, bitmap, user):
        raw = ctypes.string_at(tuples, 160 * n)
        out = bytearray((n + 7) // 8)
        for i in range(n):
            seen.append(raw[160 * i + 96:160 * i + 160])
            if fn(raw[160 * i:160 * i + 160]) == 1:
                out[i >> 3] |= 1 << (i & 7)
        ctypes.memmove(bitmap, bytes(out), len(out))
        return 0
    return hostlib.BACKEND_FN(cb)


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_verifier_decodes_and_registers_sec1_keys_on_the_cpu_backend(cv):
    """Verifier::DecodeKeys on every case (the CPU loop of Backend::decode_keys), and RegisterConsenterSec1 / RegisterClientSec1: a
    signature verifies under the key registered from its compressed and from its uncompressed form, a refused key registers nothing"""
    host = hostlib.load()
    C, S, U64P = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
    host.sbvh_decode_keys.argtypes = [hostlib.V, C, U64P, S, C, C]
    host.sbvh_register_consenter_sec1.argtypes = [hostlib.V, ctypes.c_uint64, C, S]
    host.sbvh_register_client_sec1.argtypes = [hostlib.V, C, C, S]
    seen = []
    cb = _oracle_callback(cv.name, seen)
    h = host.sbvh_verifier_new_scheme(0 if cv.name == "p256" else 2, 1, 0, cb, None, 64, 50, 0)
    try:
        idx, blob, off = cases.mixed(cv)
        m = len(idx)
        keys64, ok = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(m)
        assert host.sbvh_decode_keys(h, blob, (ctypes.c_uint64 * (m + 1))(*off), m, keys64, ok) == hostlib.OK
        assert not _differ(cv, idx, keys64.raw, ok.raw)
        idx, blob = cases.stride(cv)
        m = len(idx)
        assert host.sbvh_decode_keys(h, blob, None, m, keys64, None) == hostlib.OK
        assert not _differ(cv, idx, keys64.raw, bytes(cases.expected(cv)[i][1] for i in idx))
        bad = (ctypes.c_uint64 * 3)(0, 40, 33)
        assert host.sbvh_decode_keys(h, blob, bad, 2, keys64, None) == hostlib.INVALID
        assert host.sbvh_decode_keys(h, None, None, 1, keys64, None) == hostlib.INVALID and host.sbvh_decode_keys(h, None, None, 0, None, None) == hostlib.OK
        # registration from both encodings
        msg = b"signed by a consenter whose key arrived as a SEC1 octet string"
        for ident, form in ((7, cases.compress), (8, cases.uncompressed)):
            key = fc.signer(cv.name, ident)[1]
            sig = fc.sign(cv.name, ident, msg)
            assert host.sbvh_verify_signature(h, ident, sig, len(sig), msg, len(msg)) != hostlib.OK          # not registered yet
            assert host.sbvh_register_consenter_sec1(h, ident, form(key), len(form(key))) == 0
            seen.clear()
            assert host.sbvh_verify_signature(h, ident, sig, len(sig), msg, len(msg)) == hostlib.OK
            assert seen == [key]
            assert host.sbvh_verify_signature(h, ident, sig, len(sig), msg + b"!", len(msg) + 1) != hostlib.OK
        key = fc.signer(cv.name, 9)[1]
        hybrid = bytes([6 + (key[63] & 1)]) + key
        assert host.sbvh_register_consenter_sec1(h, 9, hybrid, 65) == -1 and host.sbvh_register_consenter_sec1(h, 9, cases.compress(key)[:32], 32) == -1
        sig = fc.sign(cv.name, 9, msg)
        assert host.sbvh_verify_signature(h, 9, sig, len(sig), msg, len(msg)) != hostlib.OK
        assert host.sbvh_register_client_sec1(h, b"client-a", cases.compress(key), 33) == 0 and host.sbvh_register_client_sec1(h, b"client-b", hybrid, 65) == -1
    finally:
        host.sbvh_verifier_free(h)
    # Ed25519 has no SEC1 keys
    h = host.sbvh_verifier_new_scheme(1, 1, 0, cb, None, 64, 50, 0)
    try:
        assert host.sbvh_decode_keys(h, b"\x02" + bytes(32), None, 1, ctypes.create_string_buffer(64), None) == hostlib.INVALID
        assert host.sbvh_register_consenter_sec1(h, 1, b"\x02" + bytes(32), 33) == -1
    finally:
        host.sbvh_verifier_free(h)


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_verifier_raw_message_route_with_sec1_keys_on_the_cpu_backend(scheme):
    """Verifier::VerifyMsgsSec1 over the default Backend::verify_msgs_sec1 (decode, then the raw-message stand-in and the oracle)"""
    host = hostlib.load()
    C, S, U64P = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
    host.sbvh_verify_msgs_sec1.argtypes = [hostlib.V, C, U64P, C, U64P, C, U64P, S, C]
    fams = mg.families(scheme)
    vcs = cases.verify_cases(scheme, [c for f in "bcde" for c in fams[f]] + mg.key_cases(scheme) + mg.empty_batch(scheme) + mg.filler(scheme)[:40])
    n = len(vcs)
    table = lambda parts: (ctypes.c_uint64 * (len(parts) + 1))(*cases.offsets_of(parts))
    msgs, sigs, keys = [c.msg for c in vcs], [c.sig for c in vcs], [c.key for c in vcs]
    seen = []
    cb = _oracle_callback(scheme, seen)                                 # held here: the Verifier keeps only the function pointer
    h = host.sbvh_verifier_new_scheme(0 if scheme == "p256" else 2, 1, 0, cb, None, 64, 50, 0)
    try:
        out = ctypes.create_string_buffer((n + 7) // 8)
        args = [b"".join(msgs), table(msgs), b"".join(sigs), table(sigs), b"".join(keys), table(keys), n, out]
        assert host.sbvh_verify_msgs_sec1(h, *args) == hostlib.OK
        got = [bool(out.raw[i >> 3] >> (i & 7) & 1) for i in range(n)]
        assert got == [c.want for c in vcs], [c.name for c, g in zip(vcs, got) if g != c.want][:12]
        assert seen == [c.key64 for c in vcs] and got.count(True) >= 40 and got.count(False) >= 20
        dec = table(keys)
        dec[3] = dec[2] - 1
        args[5] = dec
        assert host.sbvh_verify_msgs_sec1(h, *args) == hostlib.INVALID
        args[5], args[6] = table(keys), (1 << 21) + 1
        assert host.sbvh_verify_msgs_sec1(h, *args) == hostlib.INVALID
        assert host.sbvh_verify_msgs_sec1(h, None, None, None, None, None, None, 0, None) == hostlib.OK
    finally:
        host.sbvh_verifier_free(h)


# ---- other opinions ----------------------------------------------------------------------------------------------------------------------
def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
    except OSError:
        return None
    V, C, S = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
    for fn, res, args in (("EC_GROUP_new_by_curve_name", V, [ctypes.c_int]), ("EC_POINT_new", V, [V]), ("EC_POINT_free", None, [V]),
                          ("EC_GROUP_free", None, [V]), ("BN_new", V, []), ("BN_free", None, [V]), ("EC_POINT_oct2point", ctypes.c_int, [V, V, C, S, V]),
                          ("EC_POINT_get_affine_coordinates", ctypes.c_int, [V, V, V, V, V]), ("BN_bn2binpad", ctypes.c_int, [V, C, ctypes.c_int]),
                          ("ERR_clear_error", None, [])):
        if not hasattr(lib, fn):
            return None
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
    return lib


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_openssl_decodes_every_02_03_04_case_to_the_same_point(cv):
    """EC_POINT_oct2point on every case whose first byte is 02, 03 or 04 (OpenSSL also takes the hybrid forms, which SEC1 as Go applies
    it does not: those prefixes are the model's alone)"""
    lib = _libcrypto()
    if lib is None:
        pytest.skip("libcrypto did not load")
    group = lib.EC_GROUP_new_by_curve_name(415 if cv.name == "p256" else 714)          # NID_X9_62_prime256v1, NID_secp256k1
    assert group
    pt, x, y = lib.EC_POINT_new(group), lib.BN_new(), lib.BN_new()
    checked = [0, 0]
    try:
        for (name, key), (xy, ok) in zip(cases.cases(cv), cases.expected(cv)):
            if not key or key[0] not in (2, 3, 4):
                continue
            good = lib.EC_POINT_oct2point(group, pt, key, len(key), None) == 1
            lib.ERR_clear_error()
            assert good == bool(ok), name
            if good:
                bx, by = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
                assert lib.EC_POINT_get_affine_coordinates(group, pt, x, y, None) == 1
                assert lib.BN_bn2binpad(x, bx, 32) == 32 and lib.BN_bn2binpad(y, by, 32) == 32
                assert bx.raw + by.raw == xy, name
            checked[ok] += 1
    finally:
        lib.BN_free(x)
        lib.BN_free(y)
        lib.EC_POINT_free(pt)
        lib.EC_GROUP_free(group)
    assert checked[0] >= 700 and checked[1] >= 900


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_the_oracles_judge_the_verify_cases_under_the_decoded_keys(emul, scheme):
    """want of every verify case = the generic want AND the key decodes; the C oracle and OpenSSL say the same under the 64 bytes the
    emulator decodes"""
    cv = cases.BY_NAME[scheme]
    fams = mg.families(scheme)
    pool = mg.ladder(scheme)[0] + [c for f in "bcde" for c in fams[f]] + mg.key_cases(scheme) + mg.empty_batch(scheme)
    vcs = cases.verify_cases(scheme, pool)
    keys = [c.key for c in vcs]
    keys64, ok = emul.decode(cv, b"".join(keys), cases.offsets_of(keys), len(keys))
    assert keys64 == b"".join(c.key64 for c in vcs)
    assert [c.want for c in vcs] == [g.want and bool(ok[i]) for i, g in enumerate(pool)]
    assert {len(c.key) for c in vcs} >= {1, 32, 33, 65, 66} and sum(1 for c in vcs if c.want) >= 100
    for i, c in enumerate(vcs):
        assert fc.judge(scheme, c.key64, c.msg, c.sig) == c.want, c.name
        third = fc.judge_openssl(scheme, c.key64, c.msg, c.sig)
        assert third is None or third == c.want, c.name
    tail = cases.verify_cases(scheme, mg.long_tail(scheme))
    assert len(tail) == mg.MAIN and [c.want for c in tail] == [i % 5 != 4 and i % 7 != 6 for i in range(mg.MAIN)]


# ---- header, wrappers, cgo ---------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("sbv_p256_decode_keys", "sbv_secp256k1_decode_keys", "sbv_p256_decode_keys_stream", "sbv_secp256k1_decode_keys_stream",
               "sbv_p256_verify_msgs_sec1", "sbv_secp256k1_verify_msgs_sec1", "sbv_debug_sec1_op")


def test_header_declares_the_entries_and_the_wrappers_exist():
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    api = open(os.path.join(CSRC, "sbv_api.hip")).read()
    for name in NEW_ENTRIES:
        assert name + "(" in hdr and name + "(" in api, name
    assert "_decode_keys_dev" not in hdr and "_sec1_dev" not in hdr          # device-pointer forms end in _stream
    import consensus_amd as sbv
    for name in ("p256_decode_keys", "secp256k1_decode_keys", "p256_decode_keys_stream", "secp256k1_decode_keys_stream",
                 "p256_verify_msgs_sec1", "secp256k1_verify_msgs_sec1", "debug_sec1_op"):
        assert callable(getattr(sbv, name)), name
    with pytest.raises(ValueError):
        sbv.p256_decode_keys(bytes(34))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "sec1_keys_kernels.o" in mk


def test_cgo_call_sites_match_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    seen, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    called = {name for fn in os.listdir(go) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(go, fn)).read())}
    assert {"sbv_p256_decode_keys", "sbv_secp256k1_decode_keys"} <= called
    u8, u64, V, S, I = ("uint8_t", True), ("uint64_t", True), ("void", True), ("size_t", False), ("int", False)
    for curve in ("p256", "secp256k1"):
        assert protos["sbv_%s_decode_keys" % curve] == [u8, u64, S, u8, u8]
        assert protos["sbv_%s_decode_keys_stream" % curve] == [V, V, S, S, V, V, V]
        assert protos["sbv_%s_verify_msgs_sec1" % curve] == [u8, u64, u8, u64, u8, u64, S, u8]
    assert protos["sbv_debug_sec1_op"] == [I, I, u8, u8, S]
    src = open(os.path.join(go, "backend.go")).read()
    assert "type SEC1KeyDecoder interface" in src and "DecodeKeysSEC1(" in src


# ---- the sanitizer build -----------------------------------------------------------------------------------------------------------------
def test_sanitizer_build_decodes_every_key_from_a_block_of_exactly_its_length(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan: only key[0 .. len) may be read"""
    exe = str(tmp_path / "sec1_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-Wno-misleading-indentation"] + CHECKS + [EMUL_SRC, "-o", exe])
    rows = []
    for cv in cases.CURVES:
        for (_, key), (xy, ok) in zip(cases.cases(cv), cases.expected(cv)):
            rows.append("%d %s %s\n" % (cv.id, key.hex() or "-", xy.hex() if ok else "-"))
    path = tmp_path / "cases.txt"
    path.write_text("".join(rows))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases," % len(rows) in r.stdout and " 0 differ" in r.stdout, r.stdout + r.stderr
