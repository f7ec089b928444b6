"""CPU tier of the raw-message ECDSA signers (include/sbv.h: sbv_sha256_msgs, sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs and their
_stream forms; consensus_amd/csrc/ecdsa_sign_msgs.h).

tests/emul/ecdsa_sign_msgs_emul.cc compiles the lanes the gfx950 kernels are built from with g++, the header's contract assertions
on, and runs them as the kernels do.  Every case of tests/ecdsa_sign_msgs_cases.py goes through them and is held to the model there
(Python integers, hashlib, hmac), to the host library (der_encode_sig, Signer::Sign) and, where a verdict is wanted, to the C oracle
and OpenSSL.  The same source as a program of its own under AddressSanitizer and UBSan holds the loader's rule that no byte outside
msg[0 .. len) is read."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest

import ecdsa_sign_msgs_cases as cases
import frontend_cases as fc
import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "ecdsa_sign_msgs_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
C, S, U8P = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8)
ENTRIES = ("sbv_sha256_msgs", "sbv_sha256_msgs_stream", "sbv_p256_sign_msgs", "sbv_secp256k1_sign_msgs", "sbv_ecdsa_sign_msgs_workspace",
           "sbv_p256_sign_msgs_stream", "sbv_secp256k1_sign_msgs_stream", "sbv_debug_ecdsa_der_op")


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in ("ecdsa_sign_msgs.h", "sha256_dev.h", "sbv_common.h", "p256_sign.h", "k256_sign.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "emul", "libsbv_ecdsa_sign_msgs_emul.so")
    if _stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", EMUL_SRC, "-o", so])
    lib = ctypes.CDLL(so)
    U64P = ctypes.POINTER(ctypes.c_uint64)
    lib.sbvesm_sha256.argtypes = [ctypes.c_int, ctypes.c_void_p, S, C]
    lib.sbvesm_sha256.restype = None
    lib.sbvesm_sha256_msgs.argtypes = [C, U64P, S, ctypes.c_uint64, ctypes.c_int, C]
    lib.sbvesm_sha256_msgs.restype = None
    lib.sbvesm_low_s.argtypes = [ctypes.c_int, C]
    lib.sbvesm_finish.argtypes = [ctypes.c_int, C, ctypes.c_int, ctypes.c_int, C, C, C]
    lib.sbvesm_finish.restype = None
    lib.sbvesm_der_parse.argtypes = [C, S, C]
    lib.sbvesm_frontend_tuple.argtypes = [C, S, C, S, C, C]
    lib.sbvesm_frontend_tuple.restype = None
    lib.sbvesm_k256_sign.argtypes = [C, C, ctypes.c_uint32, C, C]
    lib.sbvesm_sign_msgs.argtypes = [ctypes.c_int, C, ctypes.c_uint32, ctypes.c_void_p, C, U64P, ctypes.c_uint64, S, ctypes.c_uint32,
                                     ctypes.c_int, C, C, C, C]
    lib.sbvesm_sign_msgs.restype = None
    return lib


def finish(emul, curve, rs, ok=1, low_s=0, recid=0):
    rec, ln, rid = ctypes.create_string_buffer(72), ctypes.create_string_buffer(1), ctypes.create_string_buffer(bytes([recid]), 1)
    emul.sbvesm_finish(cases.CURVE_ID[curve], rs, ok, low_s, rec, ln, rid)
    return rec.raw, ln.raw[0], rid.raw[0]


def sign_msgs(emul, curve, keys, msgs, key_index=None, flags=0, offsets=None, mbytes=None, words=1):
    """the emulated call: (records, lens, recid, ok)"""
    blob = b"".join(msgs) if offsets is None else msgs
    offs = cases.offsets_of(msgs) if offsets is None else offsets
    n = len(offs) - 1
    rec, ln, rid, ok = (ctypes.create_string_buffer(max(1, k * n)) for k in (72, 1, 1, 1))
    idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
    emul.sbvesm_sign_msgs(cases.CURVE_ID[curve], keys, len(keys) // 32, idx, blob, (ctypes.c_uint64 * (n + 1))(*offs),
                          len(blob) if mbytes is None else mbytes, n, flags, words, rec, ln, rid, ok)
    return [rec.raw[72 * i:72 * i + 72] for i in range(n)], list(ln.raw[:n]), list(rid.raw[:n]), list(ok.raw[:n])


def case_keys(curve):
    """the keys of the signing cases, one per case (an out-of-range scalar is stored modulo 2^256 as it is: n fits 32 bytes)"""
    return b"".join(cases.be32(c.d) for c in cases.sign_cases(curve))


# ---- the cases themselves -----------------------------------------------------------------------------------------------------------
def test_der_cases_cover_every_length_and_every_count_of_leading_zero_bytes():
    vals = cases.der_values()
    assert {1, 0x7F, 0x80, 0xFF, 0x100, (1 << 255) - 1, 1 << 255, cases.kc.N - 1} <= set(vals)
    shapes = {(cases.leading_zero_bytes(v), bool((v >> (8 * (31 - cases.leading_zero_bytes(v)))) & 0x80)) for v in vals}
    assert {(z, top) for z in range(1, 32) for top in (False, True)} <= shapes
    cs = cases.der_cases()
    assert len(cs) == len(vals) ** 2 and {len(c[2]) for c in cs} == set(range(8, 73))


@pytest.mark.parametrize("curve", cases.CURVES)
def test_known_answers_are_what_the_model_signs(curve):
    """RFC 6979 A.2.5 ("sample", "test" under SHA-256) as published; the secp256k1 community answers in their low-S form"""
    known = cases.known_answers(curve)
    assert len(known) >= 2
    for c in cases.sign_cases(curve):
        if c.name in known:
            r, s, _ = cases.sign_model(curve, c.d, c.msg, low_s=(curve == "k256"))
            assert (r, s) == known[c.name], c.name


def test_order_halves_of_the_header_are_the_curves():
    src = open(os.path.join(CSRC, "ecdsa_sign_msgs.h")).read()
    for name, value in (("n_p", cases.pc.N), ("h_p", (cases.pc.N - 1) // 2), ("n_k", cases.kc.N), ("h_k", (cases.kc.N - 1) // 2)):
        m = re.search(r"const u256 %s = \{\{([^}]*)\}\}" % name, src)
        limbs = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
        assert sum(v << (32 * i) for i, v in enumerate(limbs)) == value, name


# ---- DER ----------------------------------------------------------------------------------------------------------------------------
def test_record_is_the_models_and_the_hosts_encoding_and_parses_back(emul):
    """every pair: the 72-byte record is the model's DER, zero behind it; der_encode_sig of the host library gives the same bytes; the
    device parser der_parse_sig returns r | s from it"""
    host = hostlib.load()
    host.sbvh_der_encode_sig.argtypes = [C, C, S]
    host.sbvh_der_encode_sig.restype = S
    out, back = ctypes.create_string_buffer(80), ctypes.create_string_buffer(64)
    for r, s, der in cases.der_cases():
        rs = cases.be32(r) + cases.be32(s)
        rec, ln, _ = finish(emul, "p256", rs)
        assert ln == len(der) and rec == der + bytes(72 - ln), (r, s)
        assert host.sbvh_der_encode_sig(rs, out, 80) == ln and out.raw[:ln] == der, (r, s)
        assert emul.sbvesm_der_parse(rec[:ln], ln, back) == 1 and back.raw == rs, (r, s)
    assert finish(emul, "k256", bytes(63) + b"\x01", ok=0, recid=3) == (bytes(72), 0, 0)


# ---- low-S --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", cases.CURVES)
def test_low_s_at_the_edges(curve, emul):
    n = cases.order(curve)
    for s in cases.low_s_cases(curve):
        buf = ctypes.create_string_buffer(cases.be32(s), 32)
        neg = emul.sbvesm_low_s(cases.CURVE_ID[curve], buf)
        want, wneg = cases.low_s_model(curve, s)
        assert (int.from_bytes(buf.raw, "big"), bool(neg)) == (want, wneg) and want <= (n - 1) // 2, s
        rec, ln, rid = finish(emul, curve, cases.be32(7) + cases.be32(s), low_s=1, recid=2)
        assert rec[:ln] == cases.der_model(7, want) and rid == (3 if wneg else 2), s


def test_low_s_behind_the_secp256k1_signer_equals_its_own_flag(emul):
    """k256_sign_lane under flags = 0, then the finish lane's low-S with the recovery id: the signature and recid k256_sign_finish
    yields under SBV_K256_SIGN_LOW_S"""
    rs0, rs1, r0, r1 = (ctypes.create_string_buffer(k) for k in (64, 64, 1, 1))
    high = 0
    for c in cases.sign_cases("k256")[:80]:
        h = hashlib.sha256(c.msg).digest()
        assert emul.sbvesm_k256_sign(cases.be32(c.d), h, 0, rs0, r0) == 1 and emul.sbvesm_k256_sign(cases.be32(c.d), h, 1, rs1, r1) == 1
        rec, ln, rid = finish(emul, "k256", rs0.raw, low_s=1, recid=r0.raw[0])
        assert rec[:ln] == cases.der_model(int.from_bytes(rs1.raw[:32], "big"), int.from_bytes(rs1.raw[32:], "big")) and rid == r1.raw[0], c.name
        high += rs0.raw != rs1.raw
    assert 20 < high < 60


def test_low_s_p256_signatures_verify_under_the_oracle_and_openssl(emul, oracle, openssl_check):
    oracle.sbvo_p256_verify_tuple.argtypes = [C]
    oracle.sbvo_p256_pubkey.argtypes = [C, C]
    openssl_check.sbvssl_p256_verify_tuple.argtypes = [C]
    cs = cases.sign_cases("p256")[:60]
    keys = b"".join(cases.be32(c.d) for c in cs)
    recs, lens, _, ok = sign_msgs(emul, "p256", keys, [c.msg for c in cs], flags=cases.LOW_S)
    plain = sign_msgs(emul, "p256", keys, [c.msg for c in cs], flags=0)[0]
    q = ctypes.create_string_buffer(64)
    assert ok == [1] * len(cs) and 10 < sum(a != b for a, b in zip(recs, plain)) < 50
    for c, rec, ln in zip(cs, recs, lens):
        rs = fc.strict_rs(rec[:ln])
        assert int.from_bytes(rs[32:], "big") <= (cases.pc.N - 1) // 2, c.name
        oracle.sbvo_p256_pubkey(cases.be32(c.d), q)
        t = rs + hashlib.sha256(c.msg).digest() + q.raw
        assert oracle.sbvo_p256_verify_tuple(t) == 1 and openssl_check.sbvssl_p256_verify_tuple(t) == 1, c.name


# ---- hash ---------------------------------------------------------------------------------------------------------------------------
def test_word_loader_equals_hashlib_and_the_byte_loader_at_every_alignment(emul):
    out = ctypes.create_string_buffer(32)
    for m in cases.hash_messages():
        want = hashlib.sha256(m).digest()
        for a in range(4):
            buf = ctypes.create_string_buffer(bytes(a) + m, a + len(m) + 8)          # 8-byte aligned base: the message starts at a mod 4
            base = ctypes.addressof(buf)
            assert base % 4 == 0
            for words in (1, 0):
                emul.sbvesm_sha256(words, base + a, len(m), out)
                assert out.raw == want, (len(m), a, words)
    emul.sbvesm_sha256(1, None, 0, out)
    assert out.raw == hashlib.sha256(b"").digest()


@pytest.mark.parametrize("shuffled", [False, True])
def test_kernel_model_hashes_a_packed_batch_and_empties_a_refused_slice(shuffled, emul):
    msgs, starts = cases.pack_at_alignments(cases.hash_messages(), shuffled)
    want = {(len(m), a) for m in cases.hash_messages() for a in range(4)}
    assert want <= {(len(m), s % 4) for m, s in zip(msgs, starts)} and starts == cases.offsets_of(msgs)[:-1]
    blob, n = b"".join(msgs), len(msgs)
    digs = ctypes.create_string_buffer(32 * n)
    for words in (1, 0):
        emul.sbvesm_sha256_msgs(blob, (ctypes.c_uint64 * (n + 1))(*cases.offsets_of(msgs)), n, len(blob), words, digs)
        assert digs.raw == b"".join(hashlib.sha256(m).digest() for m in msgs), words
    out, empty = ctypes.create_string_buffer(32), hashlib.sha256(b"").digest()
    for a, b, size in ((9, 8, len(blob)), (0, len(blob) + 1, len(blob)), (2 ** 63, 5, len(blob))):
        emul.sbvesm_sha256_msgs(blob, (ctypes.c_uint64 * 2)(a, b), 1, size, 1, out)
        assert out.raw == empty, (a, b)


# ---- the whole lane -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def signed(emul):
    """{(curve, flags): (records, lens, recid, ok)} over the signing cases, case i under key i, plus one index out of range"""
    out = {}
    for curve in cases.CURVES:
        cs = cases.sign_cases(curve)
        for flags in (0, cases.LOW_S):
            out[curve, flags] = sign_msgs(emul, curve, case_keys(curve), [c.msg for c in cs], flags=flags)
    return out


@pytest.mark.parametrize("flags", [0, cases.LOW_S])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_lane_equals_the_model(curve, flags, signed):
    recs, lens, rid, ok = signed[curve, flags]
    want = cases.expected(curve, bool(flags))
    assert len(want) >= 305 and sum(1 for w in want if not w[2]) == 2
    for i, (der, wrid, wok) in enumerate(want):
        assert (recs[i], lens[i], ok[i]) == (der + bytes(72 - len(der)), len(der), wok), cases.sign_cases(curve)[i].name
        if curve == "k256":
            assert rid[i] == wrid, i


@pytest.mark.parametrize("scheme,curve", [(0, "p256"), (2, "k256")])
def test_lane_equals_the_host_signer_byte_for_byte(scheme, curve, signed):
    host = hostlib.load()
    recs, lens, _, ok = signed[curve, 0]
    out = ctypes.create_string_buffer(80)
    for i, c in enumerate(cases.sign_cases(curve)):
        if not ok[i]:
            continue
        s = host.sbvh_signer_new_scheme(scheme, 0, cases.be32(c.d))
        n = host.sbvh_sign(s, c.msg, len(c.msg), out, 80)
        host.sbvh_signer_free(s)
        assert out.raw[:n] == recs[i][:lens[i]], c.name


@pytest.mark.parametrize("flags", [0, cases.LOW_S])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_packed_output_goes_unchanged_through_the_verifiers_front_end(curve, flags, signed, emul, oracle):
    """the records packed as the host form packs them, fed with the messages and keys to msg_frontend_tuple_lane: every tuple of a
    produced signature is accepted by the C oracle"""
    oracle.sbvo_p256_verify_tuple.argtypes = [C]
    oracle.sbvo_k256_verify_raw.argtypes = [C] * 5
    pub = getattr(oracle, "sbvo_%s_pubkey" % curve)
    pub.argtypes = [C, C]
    recs, lens, _, ok = signed[curve, flags]
    packed = b"".join(r[:n] for r, n in zip(recs, lens))
    soff = cases.offsets_of([r[:n] for r, n in zip(recs, lens)])
    q, t = ctypes.create_string_buffer(64), ctypes.create_string_buffer(160)
    for i, c in enumerate(cases.sign_cases(curve)):
        sig = packed[soff[i]:soff[i + 1]]
        if not ok[i]:
            assert sig == b""
            continue
        pub(cases.be32(c.d), q)
        emul.sbvesm_frontend_tuple(c.msg, len(c.msg), sig, len(sig), q.raw, t)
        assert t.raw[64:96] == hashlib.sha256(c.msg).digest()
        if curve == "p256":
            assert oracle.sbvo_p256_verify_tuple(t.raw) == 1, c.name
        else:
            assert oracle.sbvo_k256_verify_raw(t.raw[:32], t.raw[32:64], t.raw[64:96], t.raw[96:128], t.raw[128:160]) == 1, c.name


@pytest.mark.parametrize("curve", cases.CURVES)
def test_refused_items_are_empty_and_leave_their_neighbours_alone(curve, emul, signed):
    cs = cases.sign_cases(curve)[:6]
    keys = b"".join(cases.be32(c.d) for c in cs)
    msgs = [c.msg for c in cs]
    honest = signed[curve, 0]
    recs, lens, rid, ok = sign_msgs(emul, curve, keys, msgs, key_index=[0, 1, 6, 3, 0xFFFFFFFF, 5])
    assert ok == [1, 1, 0, 1, 0, 1] and lens[2] == lens[4] == 0 and recs[2] == recs[4] == bytes(72) and rid[2] == rid[4] == 0
    for i in (0, 1, 3, 5):
        assert (recs[i], lens[i]) == (honest[0][i], honest[1][i])
    # a decreasing pair, and a pair behind the upload, in a table the _stream form would be handed
    blob, offs = b"".join(msgs), cases.offsets_of(msgs)
    bent = list(offs)
    bent[3] = offs[2] - 1
    recs, lens, rid, ok = sign_msgs(emul, curve, keys, blob, offsets=bent)
    assert ok[2] == 0 and lens[2] == 0 and recs[2] == bytes(72) and rid[2] == 0 and ok[:2] == [1, 1] and ok[4:] == [1, 1]
    recs, lens, rid, ok = sign_msgs(emul, curve, keys, blob, offsets=offs, mbytes=offs[-1] - 1)
    assert ok == [1, 1, 1, 1, 1, 0] and lens[5] == 0


# ---- the sanitizer program ----------------------------------------------------------------------------------------------------------
def test_sanitizer_build_runs_the_hash_and_der_cases_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan, run directly: every message in a heap block of exactly its
    length and at offsets 1, 2 and 3 of a block of len + offset bytes, through both loaders and the kernel's lane; every DER and low-S
    case through the finish lane"""
    exe = str(tmp_path / "ecdsa_sign_msgs_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    lines = ["H %s %s\n" % (m.hex() or "-", hashlib.sha256(m).hexdigest()) for m in cases.hash_messages()]
    ders = cases.der_cases()
    for r, s, der in ders:
        lines.append("D 0 0 %s %s 1 1\n" % ((cases.be32(r) + cases.be32(s)).hex(), der.hex()))
    lows = 0
    for curve in cases.CURVES:
        for s in cases.low_s_cases(curve):
            want, neg = cases.low_s_model(curve, s)
            lines.append("D %d 1 %s %s 2 %d\n" % (cases.CURVE_ID[curve], (cases.be32(5) + cases.be32(s)).hex(), cases.der_model(5, want).hex(), 3 if neg else 2))
            lows += 1
    path = tmp_path / "cases.txt"
    path.write_text("".join(lines))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "%d hash cases, %d DER cases, 0 mismatches" % (len(cases.HASH_LENGTHS), len(ders) + lows) in run.stdout


# ---- refused argument sets, exports, wrappers, the Go adapter ------------------------------------------------------------------------
def test_every_entry_refuses_before_sbv_init():
    """no device here: SBV_ENOTINIT whatever the arguments, good or bad"""
    import consensus_amd as sbv
    lib = sbv.load()
    lib.sbv_ecdsa_sign_msgs_workspace.restype = ctypes.c_size_t
    lib.sbv_ecdsa_sign_msgs_workspace.argtypes = [S]
    assert lib.sbv_ecdsa_sign_msgs_workspace(0) == 0 and lib.sbv_ecdsa_sign_msgs_workspace(8229) == 96 * 8229
    if sbv.device_count() > 0:
        return                                  # with a device the GPU tier holds the refusals (tests/test_gpu_ecdsa_sign_msgs.py)
    for call in (lambda: sbv.sha256_msgs([b"abc"]), lambda: sbv.p256_sign_msgs(cases.be32(1), [b"abc"]),
                 lambda: sbv.secp256k1_sign_msgs(cases.be32(1), [b"abc"], low_s=True), lambda: sbv.debug_ecdsa_der_op(0, [bytes(64)]),
                 lambda: sbv.sha256_msgs_stream(0, 0, 1, 0), lambda: sbv.p256_sign_msgs_stream(0, 0, 0, 0, 0, 1, 0, 0, 0, 0),
                 lambda: sbv.secp256k1_sign_msgs_stream(0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), lambda: sbv.p256_sign_msgs(b"", [], low_s=True)):
        with pytest.raises(sbv.SbvError) as ei:
            call()
        assert ei.value.code == -5


def test_library_exports_the_entries_and_the_header_keeps_its_counts():
    so = os.path.join(ROOT, "consensus_amd", "libsbv.so")
    assert os.path.exists(so), "libsbv.so is built by build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, re.M), name
        assert re.search(r"\b%s\(" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), name
        assert not name.endswith("_dev")
    assert hdr.count("int sbv_secp256k1_") == 12
    assert "#define SBV_ECDSA_SIGN_LOW_S 1u" in hdr and "#define SBV_ECDSA_DER_MAX 72" in hdr and "#define SBV_K256_SIGN_LOW_S 1u" in hdr
    kernels = open(os.path.join(CSRC, "ecdsa_sign_msgs_kernels.hip")).read()
    assert "k_sha256_msgs" in kernels and "k_ecdsa_sig_finish" in kernels and "ecdsa_sign_msgs_kernels.o" in open(os.path.join(CSRC, "Makefile")).read()


def test_python_wrappers_are_there():
    import consensus_amd as sbv
    for name in ("sha256_msgs", "sha256_msgs_stream", "p256_sign_msgs", "secp256k1_sign_msgs", "p256_sign_msgs_stream",
                 "secp256k1_sign_msgs_stream", "ecdsa_sign_msgs_workspace", "debug_ecdsa_der_op"):
        assert callable(getattr(sbv, name)), name
    assert sbv.ECDSA_SIGN_LOW_S == sbv.K256_SIGN_LOW_S == 1 and sbv.ECDSA_DER_MAX == 72


def test_go_adapter_has_the_optional_interface_and_its_calls_match_the_header():
    go = os.path.join(ROOT, "go", "gpuverifier")
    assert "type ECDSAMsgSigner interface" in open(os.path.join(go, "backend.go")).read()
    src = open(os.path.join(go, "backend_cgo.go")).read()
    assert "func (b *gpuBackend) SignMsgs(scheme Scheme, " in src
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    called = {name for name, _, _ in check_cgo.calls(src)}
    assert {"sbv_p256_sign_msgs", "sbv_secp256k1_sign_msgs"} <= called
    _, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    u8, u32, u64, sz = ("uint8_t", True), ("uint32_t", True), ("uint64_t", True), ("size_t", False)
    assert protos["sbv_p256_sign_msgs"] == [u8, ("uint32_t", False), u32, u8, u64, sz, ("uint32_t", False), u8, u64, u8]
    assert protos["sbv_secp256k1_sign_msgs"] == protos["sbv_p256_sign_msgs"][:9] + [u8, u8]


# ---- the host Signer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,curve", [(0, "p256"), (2, "k256")])
def test_sign_batch_equals_a_loop_over_sign_and_low_s_halves(scheme, curve):
    """no device here: SignBatch takes the host loop; with low_s every s is in the lower half and is the model's"""
    host = hostlib.load()
    host.sbvh_sign_batch.argtypes = [ctypes.c_void_p, C, ctypes.POINTER(ctypes.c_uint64), S, C, S]
    host.sbvh_sign_batch.restype = S
    host.sbvh_sign_batch_low_s.argtypes = [ctypes.c_void_p, C, ctypes.POINTER(ctypes.c_uint64), S, ctypes.c_int, C, S]
    host.sbvh_sign_batch_low_s.restype = S
    msgs = [c.msg for c in cases.sign_cases(curve)[:40]]
    d = cases.sign_cases(curve)[0].d
    offs = (ctypes.c_uint64 * (len(msgs) + 1))(*cases.offsets_of(msgs))
    s = host.sbvh_signer_new_scheme(scheme, 0, cases.be32(d))
    try:
        out, one = ctypes.create_string_buffer(72 * len(msgs)), ctypes.create_string_buffer(80)
        assert host.sbvh_sign_batch(s, b"".join(msgs), offs, len(msgs), out, 72) == len(msgs)
        for i, m in enumerate(msgs):
            n = host.sbvh_sign(s, m, len(m), one, 80)
            r, sv, _ = cases.sign_model(curve, d, m)
            assert out.raw[72 * i:72 * i + n] == one.raw[:n] == cases.der_model(r, sv), i
        for low in (0, 1):
            assert host.sbvh_sign_batch_low_s(s, b"".join(msgs), offs, len(msgs), low, out, 72) == len(msgs)
            for i, m in enumerate(msgs):
                r, sv, _ = cases.sign_model(curve, d, m, low_s=bool(low))
                der = cases.der_model(r, sv)
                assert out.raw[72 * i:72 * i + len(der)] == der, (low, i)
    finally:
        host.sbvh_signer_free(s)
