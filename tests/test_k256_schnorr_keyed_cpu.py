"""CPU tier of BIP-340 Schnorr verification against registered secp256k1 keys (include/sbv.h: sbv_secp256k1_schnorr_lift_keys,
sbv_secp256k1_schnorr_verify_keyed; consensus_amd/csrc/k256_schnorr_keyed.h).

tests/emul/k256_schnorr_keyed_emul.cc compiles the lanes the kernels are made of with g++, contract assertions on, and runs them as
the kernels do: 64-lane groups under the two ballots of the wave rule, over a registry from the host builders whose arrays are
allocated exactly.  Every verdict, lifted key and walk result is held byte for byte to tests/k256_schnorr_keyed_cases.py, which maps
the 1 967 cases of the generic Schnorr set onto slots of both parities; the host forms (k256_schnorr_lift, Verifier::RegisterSchnorrKey
and VerifySchnorrKeyed on the CPU backend) are held to the same cases.  The same source, built as a program of its own with
AddressSanitizer and UBSan, runs the cases once.  Only three keys are widened: a 16-bit comb costs the host builder a second."""
import ctypes
import os
import subprocess
import sys

import pytest

import hostlib
import k256_py as kp
import k256_schnorr_cases as sc
import k256_schnorr_keyed_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "k256_schnorr_keyed_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
N, P = cases.N, cases.P


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


class Emul:
    """the emulator library and one registry: the model's keys, wide_slots() widened"""

    def __init__(self):
        so = os.path.join(HERE, "emul", "libsbv_k256_schnorr_keyed_emul.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", "-DSBV_K256_CHECK",
                                   EMUL_SRC, "-o", so])
        lib = ctypes.CDLL(so)
        V, S, C, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int
        lib.sbvk256sk_registry_new.restype = V
        lib.sbvk256sk_registry_new.argtypes = [C, S, C]
        lib.sbvk256sk_registry_free.argtypes = [V]
        lib.sbvk256sk_registry_valid.argtypes = [V, V]
        lib.sbvk256sk_verify.restype = ctypes.c_ulong
        lib.sbvk256sk_verify.argtypes = [V, I, C, C, V, S, V]
        lib.sbvk256sk_lift.argtypes = [C, S, V, V]
        lib.sbvk256sk_lift.restype = None
        lib.sbvk256sk_op.restype = ctypes.c_long
        lib.sbvk256sk_op.argtypes = [V, I, I, C, V, V, S]
        self.lib = lib
        keys = cases.registry()[0]
        widen = bytearray(len(keys))
        for s in cases.wide_slots():
            widen[s] = 1
        self.reg = lib.sbvk256sk_registry_new(b"".join(keys), len(keys), bytes(widen))
        self.empty = lib.sbvk256sk_registry_new(b"", 0, None)

    def close(self):
        self.lib.sbvk256sk_registry_free(self.reg)
        self.lib.sbvk256sk_registry_free(self.empty)

    def valid(self):
        out = ctypes.create_string_buffer(len(cases.registry()[0]))
        self.lib.sbvk256sk_registry_valid(self.reg, out)
        return out.raw

    def verify(self, msgs, sigs, slots, wide, reg=None):
        n = len(slots)
        ok = ctypes.create_string_buffer(b"\xa5" * (n + 1))
        lanes = self.lib.sbvk256sk_verify(reg or self.reg, int(wide), msgs, sigs, (ctypes.c_uint32 * max(1, n))(*slots), n, ok)
        assert ok.raw[n] == 0xA5
        return ok.raw[:n], lanes

    def lift(self, pks, want_ok=True):
        m = len(pks) // 32
        keys, ok = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(m)
        self.lib.sbvk256sk_lift(pks, m, keys, ok if want_ok else None)
        return keys.raw, ok.raw

    def op(self, records, slots, wide, op=0):
        n = len(records)
        out = ctypes.create_string_buffer(cases.OP_OUT * n)
        lanes = self.lib.sbvk256sk_op(self.reg, int(wide), op, b"".join(records), (ctypes.c_uint32 * max(1, n))(*slots), out, n)
        return [out.raw[cases.OP_OUT * i:cases.OP_OUT * (i + 1)] for i in range(n)], lanes


@pytest.fixture(scope="module")
def emul():
    e = Emul()
    yield e
    e.close()


@pytest.fixture(scope="module")
def host():
    lib = hostlib.load()
    C = ctypes.c_char_p
    lib.sbvh_k256_schnorr_lift.argtypes = [C, C]
    lib.sbvh_register_schnorr_key.argtypes = [hostlib.V, C]
    lib.sbvh_register_schnorr_key.restype = ctypes.c_long
    lib.sbvh_backend_register_k256.argtypes = [hostlib.V, C]
    lib.sbvh_backend_register_k256.restype = ctypes.c_long
    lib.sbvh_verify_schnorr_keyed.argtypes = [hostlib.V, C, C, ctypes.c_void_p, ctypes.c_size_t, C]
    return lib


def _bad(got, its):
    return [(i, its[i][0], its[i][1]) for i in range(len(its)) if got[i] != its[i][5]]


# ---- the model and the case set -------------------------------------------------------------------------------------------------------
def test_the_registry_layout_and_the_case_set():
    keys, slot_of, valid = cases.registry()
    pks = cases.xonly_keys()
    refused = [pk for pk in pks if cases.lift_key(pk)[1] == 0]
    assert len(refused) >= 11 and any(int.from_bytes(pk, "big") >= P for pk in refused) and any(int.from_bytes(pk, "big") < P for pk in refused)
    assert len(keys) == 2 * (len(pks) - len(refused)) + len(refused) and valid.count(0) == len(refused)
    for pk in pks:
        a, b = slot_of[0][pk], slot_of[1][pk]
        if pk in refused:
            assert a == b and valid[a] == 0 and keys[a] == pk + bytes(32)
        else:
            (xa, ya), (xb, yb) = cases.point_of(a), cases.point_of(b)
            assert a != b and xa == xb == int.from_bytes(pk, "big") and ya % 2 == 0 and yb == P - ya and kp.on_curve(xa, ya) and kp.on_curve(xb, yb)
    its = cases.items()
    assert len(sc.cases()) == 1967 and len(its) == 2 * 1967 + 6
    assert [i[5] for i in its[:1967]] == [i[5] for i in its[1967:2 * 1967]] == list(sc.expected_all())
    assert sum(i[5] for i in its) == 2 * 299 and all(i[4] >= len(keys) and i[5] == 0 for i in its[2 * 1967:])
    # "another key" became "another slot": a valid slot that is not the signer's
    for parity in (0, 1):
        twins = [(v, o) for v, o in zip(its[parity * 1967:], its[parity * 1967 + 4:]) if v[0] == "valid" and o[0] == "other_key"]
        assert len(twins) >= 297 and all(v[4] != o[4] and valid[o[4]] and v[3] == o[3] for v, o in twins)


def test_the_keyed_model_equals_the_generic_model():
    """the direct model of the lane (u2 = n - e or e by the registered parity) gives the generic verdict, under both registrations"""
    keys = cases.registry()[0]
    its = cases.items()[:2 * 1967]
    picked = [i for k, i in enumerate(its) if k % 9 == 0 or i[0] in ("infinity", "parity", "vector", "vector_spoiled", "range", "s_zero")][:700]
    assert {i[1] for i in picked} == {0, 1} and {i[5] for i in picked} == {0, 1}
    for cat, parity, m, sig, slot, ok in picked:
        assert cases.verify_keyed(keys[slot], m, sig) == ok, (cat, parity, slot)


def test_the_walk_cases_cover_what_they_name():
    pk, d = cases.steer_key()
    assert sc.gmul(d) == cases.point_of(cases.registry()[1][0][pk]) and sc.gmul(N - d) == cases.point_of(cases.registry()[1][1][pk])
    ins, slots, outs, labels = cases.walk_cases()
    for (label, u1, u2, parity), out in zip(cases.walk_scalars(), outs):
        dq = d if parity == 0 else N - d
        q = sc.gmul((u1 + u2 * dq) % N)
        assert out == (cases.op_result(0) if q is None else cases.op_result(1, q[0], q[1])), label
        assert cases.digits_sum_8(u2) == u2 % N
        if label in ("cancel", "back") or (label == "pairs" and u1 == u2 == 0):
            assert label == "back" or out == bytes(cases.OP_OUT)
    assert sum(1 for o in outs if o == bytes(cases.OP_OUT)) >= 12 + 3 + 2 and labels.count("dead") == 3
    # the carry scalars do and do not reach window 32; the first terms are what they claim
    k = lambda u: u + int.from_bytes(b"\x80" * 32, "big")
    assert k(cases.CARRY_EDGE) >> 256 == 1 and k(cases.CARRY_EDGE - 1) >> 256 == 0 and k(cases.CARRY_ALL) >> 256 == 1
    assert cases.first_term_8(cases.CARRY_EDGE) == -128 and cases.first_term_8(1 << 64) == 1 << 64 and cases.first_term_8(N - 3) == -3
    assert cases.first_term_16(3) == 3 and cases.first_term_16(0x8000) == -0x8000 and cases.first_term_16(1 << 64) == 1 << 64
    for u in (5, 2**255 + 12345, cases.CARRY_ALL):
        pt = sc.gmul(7)
        assert kp.pt_add(sc.gmul(u), sc.mul(u, pt)) == kp.pt_mul((u + 7 * u) % N, kp.G)


def test_the_wide_batch_makes_the_four_compositions():
    its = cases.wide_batch()
    W = set(cases.wide_slots())
    waves = [its[k:k + 64] for k in range(0, 256, 64)]
    live = [[cases.is_live(i) for i in w] for w in waves]
    assert all(live[0]) and all(i[4] in W for i in waves[0])
    assert all(live[1]) and sum(1 for i in waves[1] if i[4] not in W) == 1
    assert live[2].count(False) == 1 and all(i[4] in W for i in waves[2])
    assert not any(live[3])
    assert cases.wide_lanes(its[:256], W) == 128 and cases.wide_lanes(its, ()) == 0
    assert len(its) == 256 + len(cases.items()) and len(W) == 3


# ---- the emulated lanes ---------------------------------------------------------------------------------------------------------------
def test_emulated_registry_marks_the_refused_keys_invalid(emul):
    assert emul.valid() == bytes(cases.registry()[2])


def test_emulated_lifting_equals_the_model(emul):
    pks = cases.xonly_keys() + [cases.be32(x) for x in (0, 1, 2, 3, 7, P - 1, P, P + 1, 2**256 - 1, kp.GX)]
    want = [cases.lift_key(pk) for pk in pks]
    keys, ok = emul.lift(b"".join(pks))
    assert keys == b"".join(w[0] for w in want) and ok == bytes(w[1] for w in want)
    assert emul.lift(b"".join(pks), want_ok=False)[0] == keys
    assert 0 in ok and 1 in ok


@pytest.mark.parametrize("wide", [False, True])
def test_emulated_verifier_equals_the_model(emul, wide):
    """every item in its own order: on 8-bit combs, and with three slots widened (wavefronts of mixed slots stay narrow)"""
    its = cases.items()
    got, lanes = emul.verify(*cases.arrays()[:3], wide)
    assert not _bad(got, its), _bad(got, its)[:8]
    assert lanes == cases.wide_lanes(its, cases.wide_slots() if wide else ())


def test_emulated_verifier_on_the_four_wavefront_compositions(emul):
    its = cases.wide_batch()
    msgs, sigs, slots, _ = cases.arrays(its)
    got, lanes = emul.verify(msgs, sigs, slots, True)
    assert not _bad(got, its), _bad(got, its)[:8]
    assert lanes == cases.wide_lanes(its, cases.wide_slots()) >= 128
    got0, lanes0 = emul.verify(msgs, sigs, slots, False)
    assert got0 == got and lanes0 == 0


def test_emulated_verifier_geometry_and_the_empty_registry(emul):
    for n in (1, 63, 64, 65, 255, 257):
        msgs, sigs, slots, ok = cases.tiled(n, 3 * n)
        assert emul.verify(msgs, sigs, slots, True)[0] == ok
    msgs, sigs, slots, ok = cases.tiled(130)
    assert emul.verify(msgs, sigs, slots, True, reg=emul.empty) == (bytes(130), 0)
    assert emul.verify(b"", b"", [], True) == (b"", 0)


@pytest.mark.parametrize("wide", [False, True])
def test_emulated_walk_equals_the_oracle(emul, wide):
    ins, slots, want, labels = cases.walk_cases()
    got, lanes = emul.op(ins, slots, wide)
    bad = [(i, labels[i]) for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
    assert lanes == (len(ins) if wide else 0)                      # every live lane's slot is widened: every group walks wide
    assert emul.lib.sbvk256sk_op(emul.reg, 1, 1, ins[0], (ctypes.c_uint32 * 1)(0), ctypes.create_string_buffer(128), 1) < 0


# ---- the host forms -------------------------------------------------------------------------------------------------------------------
def test_host_lift_equals_the_model(host):
    key = ctypes.create_string_buffer(64)
    for pk in cases.xonly_keys():
        wkey, wok = cases.lift_key(pk)
        assert ((host.sbvh_k256_schnorr_lift(pk, key) == 0), key.raw) == (wok == 1, wkey)


def test_verify_schnorr_keyed_on_the_cpu_backend(host):
    """RegisterSchnorrKey + VerifySchnorrKeyed on a callback backend with a registry: a loop over the host verifier under the slot's Qx;
    odd registrations go in through the backend's own register call; -2 (UNAVAILABLE) without a registry, INVALID under another scheme"""
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    keys, slot_of, valid = cases.registry()
    h = host.sbvh_verifier_new_scheme(2, 2, 0, cb, None, 64, 50, 0)
    try:
        # the registry in the model's order: even registrations through the Verifier (x-only), odd ones as 64-byte keys
        for s, k in enumerate(keys):
            even = valid[s] == 0 or k[63] % 2 == 0
            got = host.sbvh_register_schnorr_key(h, k[:32]) if even else host.sbvh_backend_register_k256(h, k)
            assert got == s, (s, got)
        assert host.sbvh_register_schnorr_key(h, keys[0][:32]) == 0          # a known key keeps its slot
        its = cases.wide_batch()
        msgs, sigs, slots, want = cases.arrays(its)
        n = len(its)
        ok = ctypes.create_string_buffer(n)
        assert host.sbvh_verify_schnorr_keyed(h, msgs, sigs, (ctypes.c_uint32 * n)(*slots), n, ok) == hostlib.OK
        assert not _bad(ok.raw, its), _bad(ok.raw, its)[:8]
        assert host.sbvh_verify_schnorr_keyed(h, msgs, sigs, None, 0, ok) == hostlib.OK
        assert host.sbvh_verify_schnorr_keyed(h, None, sigs, (ctypes.c_uint32 * n)(*slots), 1, ok) == hostlib.INVALID
    finally:
        host.sbvh_verifier_free(h)
    one = (ctypes.c_uint32 * 1)(0)
    h = host.sbvh_verifier_new_scheme(2, 1, 0, cb, None, 64, 50, 0)      # no registry
    try:
        assert host.sbvh_register_schnorr_key(h, keys[0][:32]) == -1
        assert host.sbvh_verify_schnorr_keyed(h, bytes(32), bytes(64), one, 1, ctypes.create_string_buffer(1)) == hostlib.UNAVAILABLE
    finally:
        host.sbvh_verifier_free(h)
    h = host.sbvh_verifier_new_scheme(0, 2, 0, cb, None, 64, 50, 0)      # a P-256 Verifier has no Schnorr entry
    try:
        assert host.sbvh_register_schnorr_key(h, keys[0][:32]) == -1
        assert host.sbvh_verify_schnorr_keyed(h, bytes(32), bytes(64), one, 1, ctypes.create_string_buffer(1)) == hostlib.INVALID
    finally:
        host.sbvh_verifier_free(h)


# ---- the layers above -----------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("sbv_secp256k1_schnorr_lift_keys", "sbv_secp256k1_schnorr_lift_keys_stream", "sbv_secp256k1_schnorr_verify_keyed",
               "sbv_secp256k1_schnorr_verify_keyed_stream", "sbv_debug_secp256k1_schnorr_keyed_op")


def test_header_declares_the_entries_and_the_wrappers_exist():
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    for name in NEW_ENTRIES:
        assert "\n" + name + "(" in hdr, name
    assert "_schnorr_verify_keyed_dev" not in hdr and "_schnorr_lift_keys_dev" not in hdr
    import consensus_amd as sbv
    for name in NEW_ENTRIES + ("sbv_secp256k1_schnorr_register_keys",):
        assert callable(getattr(sbv, name[4:])), name
    api = open(os.path.join(CSRC, "sbv_api.hip")).read()
    for name in NEW_ENTRIES:
        assert name + "(" in api, name
    assert "$(BUILD)/k256_schnorr_keyed_kernels.o" in open(os.path.join(CSRC, "Makefile")).read()
    lib = sbv.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    # one wave rule: the ECDSA keyed kernel and the kernels of this scheme call the same function
    rule = "k256_keyed_wave_wide(live, lane_wide)"
    assert open(os.path.join(CSRC, "k256_keyed_kernels.hip")).read().count(rule) == 1
    assert open(os.path.join(CSRC, "k256_schnorr_keyed_kernels.hip")).read().count(rule) == 2
    assert "__ballot" not in open(os.path.join(CSRC, "k256_schnorr_keyed_kernels.hip")).read().split("#include", 1)[1]


def test_cgo_call_sites_match_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    seen, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    called = {name for fn in os.listdir(go) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(go, fn)).read())}
    assert {"sbv_secp256k1_schnorr_lift_keys", "sbv_secp256k1_schnorr_verify_keyed", "sbv_secp256k1_register_keys"} <= called
    u8, u32p, V, S = ("uint8_t", True), ("uint32_t", True), ("void", True), ("size_t", False)
    assert protos["sbv_secp256k1_schnorr_lift_keys"] == [u8, S, u8, u8]
    assert protos["sbv_secp256k1_schnorr_lift_keys_stream"] == [V, S, V, V, V]
    assert protos["sbv_secp256k1_schnorr_verify_keyed"] == [u8, u8, u32p, S, u8]
    assert protos["sbv_secp256k1_schnorr_verify_keyed_stream"] == [V, V, V, S, V, V]
    assert protos["sbv_debug_secp256k1_schnorr_keyed_op"] == [("int", False), u8, u32p, u8, S]
    src = open(os.path.join(go, "backend.go")).read()
    assert "type K256SchnorrKeyed interface" in src and "RegisterSchnorrKeys(" in src and "VerifyBatchSchnorrKeyed(" in src


def test_every_new_entry_refuses_without_a_device():
    import consensus_amd as sbv
    lib = sbv.load()
    assert lib.sbv_init(0) == -1                    # SBV_ENODEV: after it every entry refuses as its siblings do
    buf = ctypes.create_string_buffer(192)
    p = ctypes.addressof(buf)
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_lift_keys(bytes(32))
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_lift_keys_stream(p, 1, p, p)
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_register_keys(bytes(32))
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_verify_keyed(bytes(32), bytes(64), [0])
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_schnorr_verify_keyed_stream(p, p, p, 1, p)
    with pytest.raises(sbv.SbvError):
        sbv.debug_secp256k1_schnorr_keyed_op(0, [bytes(192)], [0])
    with pytest.raises(ValueError):
        sbv.secp256k1_schnorr_verify_keyed(bytes(32), bytes(64), [0, 1])


def test_sanitizer_build_runs_the_cases_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan: the registry with three slots widened on exactly allocated
    arrays, the lifting cases, the batch of the four wavefront compositions and the walk cases, each with no slot wide and with the
    widened slots; one run"""
    exe = str(tmp_path / "k256_schnorr_keyed_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-DSBV_K256_CHECK", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    keys = cases.registry()[0]
    W = set(cases.wide_slots())
    rows = ["K %s %02x" % (k.hex(), 1 if s in W else 0) for s, k in enumerate(keys)]
    for pk in cases.xonly_keys():
        key, ok = cases.lift_key(pk)
        rows.append("L %s %s %02x" % (pk.hex(), key.hex(), ok))
    its = cases.wide_batch()
    rows += ["V %s %s %08x %02x" % (m.hex(), sig.hex(), slot, ok) for _, _, m, sig, slot, ok in its]
    ins, slots, outs, _ = cases.walk_cases()
    rows += ["W %s %08x %s" % (i.hex(), s, o.hex()) for i, s, o in zip(ins, slots, outs)]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(rows) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d records," % len(rows) in r.stdout and " 0 differ" in r.stdout, r.stdout + r.stderr
    assert "%d wide lanes" % cases.wide_lanes(its, W) in r.stdout
