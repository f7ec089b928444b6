"""consensus_amd — MI355X-native batch signature verification behind SmartBFT's api.Verifier.

This package is a thin ctypes binding over the product's C-ABI (include/sbv.h,
consensus_amd/libsbv.so).  It holds no verification logic and **no CPU fallback**: if the HIP
library is missing or no gfx950 device is usable, every compute call raises.

Reference seam: /root/reference/pkg/api/dependencies.go:54-71 (api.Verifier).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBV_LIB") or os.path.join(_HERE, "libsbv.so")      # SBV_LIB: A/B builds of the same ABI (tools/)
TUPLE_BYTES = 160

SBV_OK = 0
ERRORS = {-1: "SBV_ENODEV", -2: "SBV_EINVAL", -3: "SBV_ENOMEM", -4: "SBV_EDEVICE", -5: "SBV_ENOTINIT",
          -6: "SBV_EPARSE"}


class SbvError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        super().__init__(f"libsbv: {ERRORS.get(code, code)} {detail}".strip())


class Timing(ctypes.Structure):
    _fields_ = [("h2d_us", ctypes.c_double), ("prep_us", ctypes.c_double), ("verify_us", ctypes.c_double),
                ("d2h_us", ctypes.c_double), ("total_us", ctypes.c_double), ("n", ctypes.c_uint64)]


_lib: Optional[ctypes.CDLL] = None


def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (soname
    libamdhip64.so.7, same as /opt/rocm's).  If libsbv.so pulled in the system copy first and
    torch were imported later, the process would hold two HIP runtimes and torch would report
    "No HIP GPUs are available".  Loading torch's copy first (when torch is installed) makes
    libsbv's NEEDED libamdhip64.so.7 resolve to it by soname, whatever the import order.
    Without torch the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                      # torch already loaded its runtime; the soname match does the rest
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load() -> ctypes.CDLL:
    """Load libsbv.so (built by __graft_entry__.build() / consensus_amd/csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(the product has no CPU fallback)")
    _preload_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    lib.sbv_init.argtypes = [ctypes.c_int]
    lib.sbv_p256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sbv_p256_verify_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.sbv_p256_parse_der.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.sbv_sha256_batch.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_char_p]
    lib.sbv_p256_register_keys.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    lib.sbv_p256_verify_batch_keyed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sbv_p256_verify_batch_keyed_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                    ctypes.c_void_p]
    lib.sbv_ed25519_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sbv_ed25519_verify_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.sbv_secp256k1_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sbv_secp256k1_verify_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.sbv_ed25519_verify_msgs.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_size_t, ctypes.c_char_p]
    lib.sbv_ed25519_make_tuples.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_size_t, ctypes.c_char_p]
    lib.sbv_p256_verify_msgs_keyed.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p,
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sbv_p256_set_grouping.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]
    lib.sbv_last_timing.argtypes = [ctypes.POINTER(Timing)]
    lib.sbv_profile_enable.argtypes = [ctypes.c_int]
    lib.sbv_profile_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_uint64)]
    lib.sbv_profile_read_dominant.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    lib.sbv_p256_last_group_stats.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    lib.sbv_last_error.restype = ctypes.c_char_p
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != SBV_OK:
        raise SbvError(rc, load().sbv_last_error().decode(errors="replace"))


def init(device: int = 0) -> None:
    _check(load().sbv_init(device))


def shutdown() -> None:
    _check(load().sbv_shutdown())


def device_count() -> int:
    return load().sbv_device_count()


def verify_batch(tuples: bytes, n: Optional[int] = None) -> bytes:
    """Verify n 160-byte tuples held in host memory; returns the ceil(n/8)-byte accept bitmap."""
    if n is None:
        if len(tuples) % TUPLE_BYTES:
            raise ValueError("tuple buffer is not a multiple of 160 bytes")
        n = len(tuples) // TUPLE_BYTES
    if len(tuples) < n * TUPLE_BYTES:
        raise ValueError("tuple buffer too short")
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    buf = (ctypes.c_char * len(tuples)).from_buffer_copy(tuples) if n else None
    _check(load().sbv_p256_verify_batch(buf, n, out))
    return out.raw[:(n + 7) // 8]


def verify_batch_ptr(host_ptr: int, n: int, out_ptr: int) -> None:
    """Raw-pointer form (e.g. numpy buffers) of sbv_p256_verify_batch."""
    _check(load().sbv_p256_verify_batch(host_ptr, n, out_ptr))


def verify_batch_dev(d_tuples_ptr: int, n: int, d_bitmap_ptr: int, stream: int = 0) -> None:
    """Asynchronous verification of device-resident tuples on `stream` (a hipStream_t value)."""
    _check(load().sbv_p256_verify_batch_dev(d_tuples_ptr, n, d_bitmap_ptr, stream))


# ---- the registered-key wrappers of the three schemes: one ctypes body each, named by the C function ----
_U32 = ctypes.c_uint32
_PTR = ctypes.c_void_p


def _call(name: str, argtypes, *args) -> int:
    fn = getattr(load(), name)
    fn.argtypes = argtypes
    return fn(*args)


def _count_or_raise(rc: int) -> int:
    if rc < 0:
        _check(rc)
    return rc


def _register_keys(name: str, key_bytes: int, keys) -> list:
    keys = list(keys)
    blob = b"".join(keys)
    if len(blob) != key_bytes * len(keys):
        raise ValueError(f"every key must be {key_bytes} bytes")
    out = (_U32 * max(1, len(keys)))()
    _check(_call(name, [ctypes.c_char_p, ctypes.c_size_t, _PTR], blob, len(keys), out))
    return list(out[:len(keys)])


def _widen_keys(name: str, slots) -> None:
    slots = list(slots)
    arr = (_U32 * max(1, len(slots)))(*slots)
    _check(_call(name, [_PTR, ctypes.c_size_t], arr, len(slots)))


def _wide_key_stats(name: str):
    out = (_U32 * 4)()
    _check(_call(name, [_PTR], out))
    return out[0], out[1], out[2], out[3]


def _wide_selfcheck(name: str, slot: int) -> bool:
    return _count_or_raise(_call(name, [_U32], slot)) == 1


def _verify_batch_keyed(name: str, recs: bytes, slots, n: Optional[int]) -> bytes:
    if n is None:
        n = len(recs) // 96
    arr = (_U32 * max(1, n))(*slots)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    buf = (ctypes.c_char * len(recs)).from_buffer_copy(recs) if n else None
    _check(_call(name, [_PTR, _PTR, ctypes.c_size_t, _PTR], buf, arr, n, out))
    return out.raw[:(n + 7) // 8]


def _verify_batch_keyed_dev(name: str, d_recs_ptr: int, d_slots_ptr: int, n: int, d_bitmap_ptr: int, stream: int) -> None:
    _check(_call(name, [_PTR, _PTR, ctypes.c_size_t, _PTR, _PTR], d_recs_ptr, d_slots_ptr, n, d_bitmap_ptr, stream))


def register_keys(keys) -> list:
    """keys: iterable of 64-byte Qx|Qy -> list of slots (equal keys share a slot)."""
    return _register_keys("sbv_p256_register_keys", 64, keys)


def key_count() -> int:
    return load().sbv_p256_key_count()


def clear_keys() -> None:
    _check(load().sbv_p256_clear_keys())


WIDE_BITS_AUTO = 1


def wide_keys(bits: int = WIDE_BITS_AUTO, max_keys: int = 64) -> None:
    """sbv_p256_wide_keys: width and cap of the wide combs sbv_p256_widen_keys builds (bits = 0: off); see include/sbv.h."""
    _check(_call("sbv_p256_wide_keys", [ctypes.c_int, _U32], bits, max_keys))


def widen_keys(slots) -> None:
    """sbv_p256_widen_keys: a wide comb for each of these registered slots (the consenters')."""
    _widen_keys("sbv_p256_widen_keys", slots)


def wide_selfcheck(slot: int) -> bool:
    """sbv_p256_wide_selfcheck: the device-built wide comb of `slot` equals the host builder's output byte for byte."""
    return _wide_selfcheck("sbv_p256_wide_selfcheck", slot)


def wide_key_stats():
    """(slots holding a wide comb, bits, max_keys, KiB per key)"""
    return _wide_key_stats("sbv_p256_wide_key_stats")


def verify_batch_keyed(rsh: bytes, slots, n: Optional[int] = None) -> bytes:
    """Registered-key form: rsh = n x 96 bytes (r|s|hash), slots = n key slots."""
    return _verify_batch_keyed("sbv_p256_verify_batch_keyed", rsh, slots, n)


def verify_batch_keyed_dev(d_rsh_ptr: int, d_slots_ptr: int, n: int, d_bitmap_ptr: int, stream: int = 0) -> None:
    _verify_batch_keyed_dev("sbv_p256_verify_batch_keyed_dev", d_rsh_ptr, d_slots_ptr, n, d_bitmap_ptr, stream)


def ed25519_make_tuples(sigs, pks, msgs) -> bytes:
    """(64-byte sig, 32-byte pk, message) triples -> n x 128-byte tuples (R | S | pk | k)."""
    n = len(sigs)
    offs = (ctypes.c_uint64 * (n + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        offs[i] = acc
        acc += len(m)
    offs[n] = acc
    out = ctypes.create_string_buffer(max(1, 128 * n))
    _check(load().sbv_ed25519_make_tuples(b"".join(sigs), b"".join(pks), b"".join(msgs), offs, n, out))
    return out.raw[:128 * n]


def ed25519_verify_msgs(sigs, pks, msgs) -> bytes:
    """(64-byte sig, 32-byte pk, message) triples -> accept bitmap; SHA-512 and the reduction mod L run on the device."""
    n = len(sigs)
    offs = (ctypes.c_uint64 * (n + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        offs[i] = acc
        acc += len(m)
    offs[n] = acc
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    _check(load().sbv_ed25519_verify_msgs(b"".join(sigs), b"".join(pks), b"".join(msgs), offs, n, out))
    return out.raw[:(n + 7) // 8]


def ed25519_verify_batch(tuples: bytes, n: Optional[int] = None) -> bytes:
    if n is None:
        n = len(tuples) // 128
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    buf = (ctypes.c_char * len(tuples)).from_buffer_copy(tuples) if n else None
    _check(load().sbv_ed25519_verify_batch(buf, n, out))
    return out.raw[:(n + 7) // 8]


def ed25519_verify_batch_dev(d_tuples_ptr: int, n: int, d_bitmap_ptr: int, stream: int = 0) -> None:
    _check(load().sbv_ed25519_verify_batch_dev(d_tuples_ptr, n, d_bitmap_ptr, stream))


def ed25519_register_keys(pks) -> list:
    """pks: iterable of 32-byte encoded Ed25519 keys -> list of slots (equal encodings share a slot; see include/sbv.h)."""
    return _register_keys("sbv_ed25519_register_keys", 32, pks)


def ed25519_key_count() -> int:
    return _count_or_raise(load().sbv_ed25519_key_count())


def ed25519_clear_keys() -> None:
    _check(load().sbv_ed25519_clear_keys())


def ed25519_wide_keys(max_keys: int = 64) -> None:
    """sbv_ed25519_wide_keys: cap on the registered Ed25519 slots with a 16-bit comb (0 = none)."""
    _check(_call("sbv_ed25519_wide_keys", [_U32], max_keys))


def ed25519_widen_keys(slots) -> None:
    """sbv_ed25519_widen_keys: a 16-bit comb of -A for each of these registered slots (the consenters')."""
    _widen_keys("sbv_ed25519_widen_keys", slots)


def ed25519_wide_key_stats():
    """(slots holding a 16-bit comb, 16, cap, KiB per comb)"""
    return _wide_key_stats("sbv_ed25519_wide_key_stats")


def ed25519_wide_selfcheck(slot: int) -> bool:
    """sbv_ed25519_wide_selfcheck: the device-built 16-bit comb of `slot` equals the host builder's output byte for byte."""
    return _wide_selfcheck("sbv_ed25519_wide_selfcheck", slot)


def ed25519_verify_batch_keyed(rsk: bytes, slots, n: Optional[int] = None) -> bytes:
    """Registered-key form: rsk = n x 96 bytes (R | S | k), slots = n key slots -> accept bitmap."""
    return _verify_batch_keyed("sbv_ed25519_verify_batch_keyed", rsk, slots, n)


def ed25519_verify_batch_keyed_dev(d_rsk_ptr: int, d_slots_ptr: int, n: int, d_bitmap_ptr: int, stream: int = 0) -> None:
    _verify_batch_keyed_dev("sbv_ed25519_verify_batch_keyed_dev", d_rsk_ptr, d_slots_ptr, n, d_bitmap_ptr, stream)


def ed25519_verify_msgs_keyed(sigs, msgs, slots) -> bytes:
    """(64-byte sig, message, slot) triples -> accept bitmap; k = SHA-512(R | A | M) mod L on the device, A from the registry."""
    n = len(sigs)
    offs = (ctypes.c_uint64 * (n + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        offs[i] = acc
        acc += len(m)
    offs[n] = acc
    arr = (ctypes.c_uint32 * max(1, n))(*slots)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    lib = load()
    lib.sbv_ed25519_verify_msgs_keyed.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
                                                  ctypes.c_size_t, ctypes.c_void_p]
    _check(lib.sbv_ed25519_verify_msgs_keyed(b"".join(sigs), b"".join(msgs), offs, arr, n, out))
    return out.raw[:(n + 7) // 8]


def secp256k1_verify_batch(tuples: bytes, n: Optional[int] = None) -> bytes:
    """ECDSA over secp256k1 on 160-byte tuples r | s | hash | Qx | Qy (include/sbv.h); returns the accept bitmap."""
    if n is None:
        n = len(tuples) // 160
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    buf = (ctypes.c_char * len(tuples)).from_buffer_copy(tuples) if n else None
    _check(load().sbv_secp256k1_verify_batch(buf, n, out))
    return out.raw[:(n + 7) // 8]


def secp256k1_verify_batch_dev(d_tuples_ptr: int, n: int, d_bitmap_ptr: int, stream: int = 0) -> None:
    _check(load().sbv_secp256k1_verify_batch_dev(d_tuples_ptr, n, d_bitmap_ptr, stream))


def secp256k1_register_keys(keys) -> list:
    """keys: iterable of 64-byte Qx | Qy -> list of slots of the secp256k1 registry (equal keys share a slot; see include/sbv.h)."""
    return _register_keys("sbv_secp256k1_register_keys", 64, keys)


def secp256k1_key_count() -> int:
    return _count_or_raise(load().sbv_secp256k1_key_count())


def secp256k1_clear_keys() -> None:
    _check(load().sbv_secp256k1_clear_keys())


def secp256k1_wide_keys(max_keys: int = 64) -> None:
    """sbv_secp256k1_wide_keys: cap on the registered secp256k1 slots with a 16-bit comb (0 = none)."""
    _check(_call("sbv_secp256k1_wide_keys", [_U32], max_keys))


def secp256k1_widen_keys(slots) -> None:
    """sbv_secp256k1_widen_keys: a 16-bit comb of Q for each of these registered slots (the consenters')."""
    _widen_keys("sbv_secp256k1_widen_keys", slots)


def secp256k1_wide_key_stats():
    """(slots holding a 16-bit comb, 16, cap, KiB per comb)"""
    return _wide_key_stats("sbv_secp256k1_wide_key_stats")


def secp256k1_wide_selfcheck(slot: int) -> bool:
    """sbv_secp256k1_wide_selfcheck: the device-built 16-bit comb of `slot` equals the host builder's output byte for byte."""
    return _wide_selfcheck("sbv_secp256k1_wide_selfcheck", slot)


def secp256k1_verify_batch_keyed(rsh: bytes, slots, n: Optional[int] = None) -> bytes:
    """Registered-key form: rsh = n x 96 bytes (r | s | hash), slots = n key slots -> accept bitmap."""
    return _verify_batch_keyed("sbv_secp256k1_verify_batch_keyed", rsh, slots, n)


def secp256k1_verify_batch_keyed_dev(d_rsh_ptr: int, d_slots_ptr: int, n: int, d_bitmap_ptr: int, stream: int = 0) -> None:
    _verify_batch_keyed_dev("sbv_secp256k1_verify_batch_keyed_dev", d_rsh_ptr, d_slots_ptr, n, d_bitmap_ptr, stream)


def secp256k1_verify_msgs_keyed(msgs, sigs_der, slots) -> bytes:
    """Device front end: SHA-256(msg) + strict DER parse on the GPU, then registered-key verification over secp256k1."""
    n = len(msgs)
    mo = (ctypes.c_uint64 * (n + 1))()
    so = (ctypes.c_uint64 * (n + 1))()
    a = b = 0
    for i in range(n):
        mo[i], so[i] = a, b
        a += len(msgs[i]); b += len(sigs_der[i])
    mo[n], so[n] = a, b
    arr = (ctypes.c_uint32 * max(1, n))(*slots)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    lib = load()
    lib.sbv_secp256k1_verify_msgs_keyed.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p,
                                                    ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_verify_msgs_keyed(b"".join(msgs), mo, b"".join(sigs_der), so, arr, n, out))
    return out.raw[:(n + 7) // 8]


def verify_msgs_keyed(msgs, sigs_der, slots) -> bytes:
    """Device front end: SHA-256(msg) + strict DER parse on the GPU, then registered-key verification."""
    n = len(msgs)
    mo = (ctypes.c_uint64 * (n + 1))()
    so = (ctypes.c_uint64 * (n + 1))()
    a = b = 0
    for i in range(n):
        mo[i], so[i] = a, b
        a += len(msgs[i]); b += len(sigs_der[i])
    mo[n], so[n] = a, b
    arr = (ctypes.c_uint32 * max(1, n))(*slots)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    _check(load().sbv_p256_verify_msgs_keyed(b"".join(msgs), mo, b"".join(sigs_der), so, arr, n, out))
    return out.raw[:(n + 7) // 8]


_MSGS_ARGS = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p]


def _msgs_tables(msgs, sigs_der, keys, offsets=None):
    """(n, message offsets, signature offsets, key bytes) of a raw-message call; keys: n x 64 bytes Qx | Qy, as a list or one string"""
    n = len(msgs)
    mo = (ctypes.c_uint64 * (n + 1))()
    so = (ctypes.c_uint64 * (n + 1))()
    a = b = 0
    for i in range(n):
        mo[i], so[i] = a, b
        a += len(msgs[i]); b += len(sigs_der[i])
    mo[n], so[n] = a, b
    if offsets is not None:
        for i in range(n + 1):
            mo[i], so[i] = offsets[0][i], offsets[1][i]
    kb = bytes(keys) if isinstance(keys, (bytes, bytearray)) else b"".join(keys)
    if len(kb) != 64 * n:
        raise ValueError("keys must be n x 64 bytes Qx | Qy")
    return n, mo, so, kb


def _verify_msgs(symbol, msgs, sigs_der, keys) -> bytes:
    n, mo, so, kb = _msgs_tables(msgs, sigs_der, keys)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    fn = getattr(load(), symbol)
    fn.argtypes = _MSGS_ARGS + [ctypes.c_size_t, ctypes.c_void_p]
    _check(fn(b"".join(msgs), mo, b"".join(sigs_der), so, kb, n, out))
    return out.raw[:(n + 7) // 8]


def verify_msgs(msgs, sigs_der, keys) -> bytes:
    """sbv_p256_verify_msgs: raw messages + DER signatures + the signers' 64-byte keys (no registry): SHA-256, the strict DER parse and
    the tuple layout on the GPU, then the generic P-256 step -> accept bitmap (n <= 2^21)."""
    return _verify_msgs("sbv_p256_verify_msgs", msgs, sigs_der, keys)


def secp256k1_verify_msgs(msgs, sigs_der, keys) -> bytes:
    """sbv_secp256k1_verify_msgs: the same front end in front of the generic secp256k1 step."""
    return _verify_msgs("sbv_secp256k1_verify_msgs", msgs, sigs_der, keys)


def _sec1_pack(keys, offsets=None):
    """(m, packed bytes, offset table or None) of SEC1 keys.  keys: a list of byte strings (packed back to back, with an offset table),
    or one bytes object of 33-byte compressed keys (the fixed stride, no table); offsets: a table of m + 1 entries to pass as it is."""
    if isinstance(keys, (bytes, bytearray)) and offsets is None:
        if len(keys) % 33:
            raise ValueError("a bytes object of SEC1 keys must be m x 33 bytes (compressed keys); pass a list for mixed lengths")
        return len(keys) // 33, bytes(keys), None
    if offsets is not None:
        m = len(offsets) - 1
        ko = (ctypes.c_uint64 * (m + 1))(*offsets)
        return m, (bytes(keys) if isinstance(keys, (bytes, bytearray)) else b"".join(keys)), ko
    m = len(keys)
    ko = (ctypes.c_uint64 * (m + 1))()
    a = 0
    for i in range(m):
        ko[i] = a
        a += len(keys[i])
    ko[m] = a
    return m, b"".join(keys), ko


def _decode_keys(symbol, keys, offsets, want_ok):
    m, kb, ko = _sec1_pack(keys, offsets)
    fn = getattr(load(), symbol)
    fn.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    keys64, ok = ctypes.create_string_buffer(max(1, 64 * m)), ctypes.create_string_buffer(max(1, m))
    _check(fn(kb, ko, m, keys64, ok if want_ok else None))
    return keys64.raw[:64 * m], (ok.raw[:m] if want_ok else None)


def p256_decode_keys(keys, offsets=None, want_ok: bool = True):
    """sbv_p256_decode_keys: SEC1 public keys (65 bytes 04 | X | Y, 33 bytes 02/03 | X) -> (keys64, ok): X | Y per key in one bytes object,
    the bytes every ECDSA entry and register_keys take, 64 zero bytes and ok 0 for a refused key.  keys: a list of byte strings, or one
    bytes object of m x 33 compressed keys (the fixed stride)."""
    return _decode_keys("sbv_p256_decode_keys", keys, offsets, want_ok)


def secp256k1_decode_keys(keys, offsets=None, want_ok: bool = True):
    """sbv_secp256k1_decode_keys: the same for secp256k1."""
    return _decode_keys("sbv_secp256k1_decode_keys", keys, offsets, want_ok)


_SEC1_STREAM_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def p256_decode_keys_stream(d_keys_ptr: int, d_key_offsets_ptr: int, key_bytes: int, m: int, d_keys64_ptr: int, d_ok_ptr: int = 0,
                            stream: int = 0) -> None:
    """sbv_p256_decode_keys_stream: device pointers, launched on `stream`, no synchronisation.  d_key_offsets_ptr 0: the 33-byte stride."""
    lib = load()
    lib.sbv_p256_decode_keys_stream.argtypes = _SEC1_STREAM_ARGS
    _check(lib.sbv_p256_decode_keys_stream(d_keys_ptr or None, d_key_offsets_ptr or None, key_bytes, m, d_keys64_ptr or None, d_ok_ptr or None,
                                           stream or None))


def secp256k1_decode_keys_stream(d_keys_ptr: int, d_key_offsets_ptr: int, key_bytes: int, m: int, d_keys64_ptr: int, d_ok_ptr: int = 0,
                                 stream: int = 0) -> None:
    """sbv_secp256k1_decode_keys_stream: the same for secp256k1."""
    lib = load()
    lib.sbv_secp256k1_decode_keys_stream.argtypes = _SEC1_STREAM_ARGS
    _check(lib.sbv_secp256k1_decode_keys_stream(d_keys_ptr or None, d_key_offsets_ptr or None, key_bytes, m, d_keys64_ptr or None,
                                                d_ok_ptr or None, stream or None))


def _verify_msgs_sec1(symbol, msgs, sigs_der, keys) -> bytes:
    n, mo, so, _ = _msgs_tables(msgs, sigs_der, bytes(64 * len(msgs)))
    m, kb, ko = _sec1_pack(keys)
    if m != n:
        raise ValueError("one SEC1 key per message")
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    fn = getattr(load(), symbol)
    fn.argtypes = _MSGS_ARGS + [ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_void_p]
    _check(fn(b"".join(msgs), mo, b"".join(sigs_der), so, kb, ko, n, out))
    return out.raw[:(n + 7) // 8]


def p256_verify_msgs_sec1(msgs, sigs_der, keys) -> bytes:
    """sbv_p256_verify_msgs_sec1: verify_msgs with the signers' keys as SEC1 octet strings (a list, or m x 33 bytes of compressed keys),
    decoded on the GPU in front of the front end, once per signature.  A refused key is a reject."""
    return _verify_msgs_sec1("sbv_p256_verify_msgs_sec1", msgs, sigs_der, keys)


def secp256k1_verify_msgs_sec1(msgs, sigs_der, keys) -> bytes:
    """sbv_secp256k1_verify_msgs_sec1: the same in front of the generic secp256k1 step."""
    return _verify_msgs_sec1("sbv_secp256k1_verify_msgs_sec1", msgs, sigs_der, keys)


def debug_sec1_op(curve: int, op: int, records):
    """sbv_debug_sec1_op (test only): one case per lane, 192-byte input records -> 128-byte output records (include/sbv.h)"""
    lib = load()
    n = len(records)
    lib.sbv_debug_sec1_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(1, 128 * n))
    _check(lib.sbv_debug_sec1_op(curve, op, b"".join(records), out, n))
    return [out.raw[128 * i:128 * i + 128] for i in range(n)]


def set_grouping(enabled: bool, min_batch: int = 0, min_count: int = 0, max_groups: int = 0) -> None:
    """In-step grouping of generic batches by public key (0 keeps a value; min_batch = GROUP_MIN_BATCH_DEFAULT restores the
    built-in thresholds); see include/sbv.h."""
    lib = load()
    _check(lib.sbv_p256_set_grouping(1 if enabled else 0, min_batch, min_count, max_groups))


SCHEME_P256, SCHEME_SECP256K1, SCHEME_ED25519 = 0, 1, 2
GROUP_MIN_BATCH_DEFAULT = (1 << 64) - 1     # (size_t)-1


def key_cache(enabled: bool, capacity: int = 0, scheme: int = SCHEME_P256) -> None:
    """sbv_key_cache: the persistent key-table cache of a scheme's grouped step (off also empties it); the default is the
    P-256 one (sbv_p256_key_cache)."""
    lib = load()
    lib.sbv_key_cache.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32]
    _check(lib.sbv_key_cache(scheme, 1 if enabled else 0, capacity))


def sign_batch(keys: bytes, digests: bytes, key_index=None):
    """sbv_p256_sign_batch: RFC 6979 ECDSA P-256 signatures (r | s, 64 bytes each) of n 32-byte digests under the 32-byte private
    scalars in `keys` (key_index[i], default i % n_keys).  Returns (sigs, ok) with ok[i] = 1 per produced signature."""
    lib = load()
    n, nk = len(digests) // 32, len(keys) // 32
    lib.sbv_p256_sign_batch.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                        ctypes.c_char_p, ctypes.c_char_p]
    sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(max(1, n))
    idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
    _check(lib.sbv_p256_sign_batch(keys, nk, idx, digests, n, sigs, ok))
    return sigs.raw, ok.raw[:n]


def sign_batch_dev(d_keys_ptr: int, n_keys: int, d_index_ptr: int, d_digests_ptr: int, n: int, d_sigs_ptr: int, d_ok_ptr: int,
                   stream: int = 0) -> None:
    lib = load()
    lib.sbv_p256_sign_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_p256_sign_batch_dev(d_keys_ptr, n_keys, d_index_ptr or None, d_digests_ptr, n, d_sigs_ptr, d_ok_ptr, stream or None))


K256_SIGN_LOW_S = 1      # SBV_K256_SIGN_LOW_S


def secp256k1_sign_batch(keys: bytes, digests: bytes, key_index=None, low_s: bool = False):
    """sbv_secp256k1_sign_batch: RFC 6979 ECDSA secp256k1 signatures (r | s, 64 bytes each) of n 32-byte digests under the 32-byte
    private scalars in `keys` (key_index[i], default i % n_keys); low_s replaces s > (n-1)/2 by n - s.  Returns (sigs, recid, ok):
    recid[i] = the recovery id 0..3, ok[i] = 1 per produced signature (a key outside [1, n-1] or an index out of range gives
    ok[i] = 0, 64 zero bytes and recid[i] = 0).  NOT constant-time: see include/sbv.h."""
    lib = load()
    n, nk = len(digests) // 32, len(keys) // 32
    lib.sbv_secp256k1_sign_batch.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    sigs, recid, ok = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n)), ctypes.create_string_buffer(max(1, n))
    idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
    _check(lib.sbv_secp256k1_sign_batch(keys, nk, idx, digests, n, K256_SIGN_LOW_S if low_s else 0, sigs, recid, ok))
    return sigs.raw[:64 * n], recid.raw[:n], ok.raw[:n]


def secp256k1_sign_batch_stream(d_keys_ptr: int, n_keys: int, d_index_ptr: int, d_digests_ptr: int, n: int, d_sigs_ptr: int,
                                d_recid_ptr: int, d_ok_ptr: int, low_s: bool = False, stream: int = 0) -> None:
    """device pointers; asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_secp256k1_sign_batch_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                    ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_sign_batch_stream(d_keys_ptr, n_keys, d_index_ptr or None, d_digests_ptr, n, K256_SIGN_LOW_S if low_s else 0,
                                               d_sigs_ptr, d_recid_ptr or None, d_ok_ptr, stream or None))


ECDSA_SIGN_LOW_S = 1     # SBV_ECDSA_SIGN_LOW_S
ECDSA_DER_MAX = 72       # SBV_ECDSA_DER_MAX


def _msg_offsets(msgs, offsets=None):
    """(blob, ctypes offset table, n) of a list of messages, or of a blob with a given offset list"""
    if offsets is not None:
        return (None if msgs is None else bytes(msgs)), (ctypes.c_uint64 * len(offsets))(*offsets), len(offsets) - 1
    offs = (ctypes.c_uint64 * (len(msgs) + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        offs[i] = acc
        acc += len(m)
    offs[len(msgs)] = acc
    return b"".join(msgs), offs, len(msgs)


def sha256_msgs(msgs, offsets=None):
    """sbv_sha256_msgs: SHA-256 of every message on the device (a list of messages, or a blob with `offsets`) -> a list of digests"""
    lib = load()
    blob, offs, n = _msg_offsets(msgs, offsets)
    lib.sbv_sha256_msgs.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_char_p]
    out = ctypes.create_string_buffer(max(1, 32 * n))
    _check(lib.sbv_sha256_msgs(blob, offs, n, out))
    return [out.raw[32 * i:32 * i + 32] for i in range(n)]


def sha256_msgs_stream(d_msgs_ptr: int, d_offsets_ptr: int, n: int, d_digests_ptr: int, stream: int = 0) -> None:
    """device pointers; asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_sha256_msgs_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_sha256_msgs_stream(d_msgs_ptr or None, d_offsets_ptr, n, d_digests_ptr, stream or None))


def _ecdsa_sign_msgs(symbol, keys: bytes, msgs, key_index, low_s, offsets, with_recid):
    lib = load()
    blob, offs, n = _msg_offsets(msgs, offsets)
    nk = len(keys) // 32
    C, U64P = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
    sigs, soff = ctypes.create_string_buffer(max(1, ECDSA_DER_MAX * n)), (ctypes.c_uint64 * (n + 1))()
    recid, ok = ctypes.create_string_buffer(max(1, n)), ctypes.create_string_buffer(max(1, n))
    idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
    head = [C, ctypes.c_uint32, ctypes.c_void_p, C, U64P, ctypes.c_size_t, ctypes.c_uint32, C, U64P]
    fn = getattr(lib, symbol)
    fn.argtypes = head + ([C, C] if with_recid else [C])
    flags = ECDSA_SIGN_LOW_S if low_s else 0
    if with_recid:
        _check(fn(keys, nk, idx, blob, offs, n, flags, sigs, soff, recid, ok))
    else:
        _check(fn(keys, nk, idx, blob, offs, n, flags, sigs, soff, ok))
    return sigs.raw[:soff[n]], list(soff), recid.raw[:n], ok.raw[:n]


def p256_sign_msgs(keys: bytes, msgs, key_index=None, low_s: bool = False, offsets=None):
    """sbv_p256_sign_msgs: SHA-256, RFC 6979 ECDSA P-256 and DER on the device, one call.  keys: 32-byte private scalars (key_index[i],
    default i % n_keys); msgs: a list of messages (or a blob with `offsets`); low_s replaces s > (n-1)/2 by n - s.  Returns
    (sigs, sig_offsets, ok): the DER signatures packed back to back with their n + 1 offsets — the pair verify_msgs takes — and
    ok[i] = 1 per produced signature (a refused item has an empty signature).  NOT constant-time: see include/sbv.h."""
    sigs, soff, _, ok = _ecdsa_sign_msgs("sbv_p256_sign_msgs", keys, msgs, key_index, low_s, offsets, False)
    return sigs, soff, ok


def secp256k1_sign_msgs(keys: bytes, msgs, key_index=None, low_s: bool = False, offsets=None):
    """sbv_secp256k1_sign_msgs: as p256_sign_msgs over secp256k1.  Returns (sigs, sig_offsets, recid, ok); recid[i] = the recovery id
    0..3 (0 for a refused item).  NOT constant-time: see include/sbv.h."""
    return _ecdsa_sign_msgs("sbv_secp256k1_sign_msgs", keys, msgs, key_index, low_s, offsets, True)


def ecdsa_sign_msgs_workspace(n: int) -> int:
    """sbv_ecdsa_sign_msgs_workspace: bytes of d_work for a _stream call of n messages"""
    lib = load()
    lib.sbv_ecdsa_sign_msgs_workspace.restype = ctypes.c_size_t
    lib.sbv_ecdsa_sign_msgs_workspace.argtypes = [ctypes.c_size_t]
    return lib.sbv_ecdsa_sign_msgs_workspace(n)


def p256_sign_msgs_stream(d_keys_ptr: int, n_keys: int, d_index_ptr: int, d_msgs_ptr: int, d_offsets_ptr: int, n: int, d_records_ptr: int,
                          d_len_ptr: int, d_ok_ptr: int, d_work_ptr: int, low_s: bool = False, stream: int = 0) -> None:
    """device pointers; asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    V = ctypes.c_void_p
    lib.sbv_p256_sign_msgs_stream.argtypes = [V, ctypes.c_uint32, V, V, V, ctypes.c_size_t, ctypes.c_uint32, V, V, V, V, V]
    _check(lib.sbv_p256_sign_msgs_stream(d_keys_ptr, n_keys, d_index_ptr or None, d_msgs_ptr or None, d_offsets_ptr, n,
                                         ECDSA_SIGN_LOW_S if low_s else 0, d_records_ptr, d_len_ptr, d_ok_ptr, d_work_ptr, stream or None))


def secp256k1_sign_msgs_stream(d_keys_ptr: int, n_keys: int, d_index_ptr: int, d_msgs_ptr: int, d_offsets_ptr: int, n: int,
                               d_records_ptr: int, d_len_ptr: int, d_recid_ptr: int, d_ok_ptr: int, d_work_ptr: int, low_s: bool = False,
                               stream: int = 0) -> None:
    """device pointers; asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    V = ctypes.c_void_p
    lib.sbv_secp256k1_sign_msgs_stream.argtypes = [V, ctypes.c_uint32, V, V, V, ctypes.c_size_t, ctypes.c_uint32, V, V, V, V, V, V]
    _check(lib.sbv_secp256k1_sign_msgs_stream(d_keys_ptr, n_keys, d_index_ptr or None, d_msgs_ptr or None, d_offsets_ptr, n,
                                              ECDSA_SIGN_LOW_S if low_s else 0, d_records_ptr, d_len_ptr, d_recid_ptr or None, d_ok_ptr,
                                              d_work_ptr, stream or None))


def debug_ecdsa_der_op(curve: int, rs_list, low_s: bool = False):
    """sbv_debug_ecdsa_der_op (test only): k_ecdsa_sig_finish on given 64-byte r | s -> a list of (72-byte record, length)"""
    lib = load()
    n = len(rs_list)
    lib.sbv_debug_ecdsa_der_op.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    rec, ln = ctypes.create_string_buffer(max(1, 72 * n)), ctypes.create_string_buffer(max(1, n))
    _check(lib.sbv_debug_ecdsa_der_op(curve, ECDSA_SIGN_LOW_S if low_s else 0, b"".join(rs_list), rec, ln, n))
    return [(rec.raw[72 * i:72 * i + 72], ln.raw[i]) for i in range(n)]


def secp256k1_pubkeys(keys: bytes):
    """sbv_secp256k1_pubkeys: 32-byte private scalars -> (pubs, ok): m x 64 bytes Qx | Qy in one bytes object and ok[i] = 1 per key in
    [1, n-1] (otherwise 64 zero bytes).  NOT constant-time: see include/sbv.h."""
    lib = load()
    m = len(keys) // 32
    lib.sbv_secp256k1_pubkeys.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    pubs, ok = ctypes.create_string_buffer(max(1, 64 * m)), ctypes.create_string_buffer(max(1, m))
    _check(lib.sbv_secp256k1_pubkeys(keys, m, pubs, ok))
    return pubs.raw[:64 * m], ok.raw[:m]


def secp256k1_pubkeys_stream(d_keys_ptr: int, m: int, d_pubs_ptr: int, d_ok_ptr: int, stream: int = 0) -> None:
    lib = load()
    lib.sbv_secp256k1_pubkeys_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_pubkeys_stream(d_keys_ptr, m, d_pubs_ptr, d_ok_ptr, stream or None))


def debug_secp256k1_sign_op(op: int, records):
    """sbv_debug_secp256k1_sign_op (test only): one case per lane, 192-byte input records -> 128-byte output records (include/sbv.h)"""
    lib = load()
    n = len(records)
    lib.sbv_debug_secp256k1_sign_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(1, 128 * n))
    _check(lib.sbv_debug_secp256k1_sign_op(op, b"".join(records), out, n))
    return [out.raw[128 * i:128 * i + 128] for i in range(n)]


K256_RECOVER_LOW_S = 1   # SBV_K256_RECOVER_LOW_S


def secp256k1_recover(sigs: bytes, recid: bytes, digests: bytes, low_s: bool = False):
    """sbv_secp256k1_recover: the signers' public keys of n signatures (r | s, 64 bytes each) with their recovery ids (n bytes, 0..3) and
    32-byte digests: exactly the arrays secp256k1_sign_batch returns.  Returns (pubs, ok): n x 64 bytes Qx | Qy in one bytes object and
    ok[i] = 1 per recovered key; a refused input (include/sbv.h has the rules) gives ok[i] = 0 and 64 zero bytes.  low_s also refuses
    s > (n-1)/2."""
    lib = load()
    n = len(recid)
    if len(sigs) != 64 * n or len(digests) != 32 * n:
        raise ValueError("secp256k1_recover: sigs, recid and digests disagree about n")
    lib.sbv_secp256k1_recover.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32,
                                          ctypes.c_char_p, ctypes.c_char_p]
    pubs, ok = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
    _check(lib.sbv_secp256k1_recover(bytes(sigs), bytes(recid), bytes(digests), n, K256_RECOVER_LOW_S if low_s else 0, pubs, ok))
    return pubs.raw[:64 * n], ok.raw[:n]


def secp256k1_recover_workspace(n: int) -> int:
    """sbv_secp256k1_recover_workspace: the bytes of device workspace secp256k1_recover_stream needs for n signatures"""
    lib = load()
    lib.sbv_secp256k1_recover_workspace.argtypes = [ctypes.c_size_t]
    lib.sbv_secp256k1_recover_workspace.restype = ctypes.c_size_t
    return int(lib.sbv_secp256k1_recover_workspace(n))


def secp256k1_recover_stream(d_sigs_ptr: int, d_recid_ptr: int, d_digests_ptr: int, n: int, d_pubs_ptr: int, d_ok_ptr: int,
                             d_work_ptr: int, work_bytes: int, low_s: bool = False, stream: int = 0, flags=None) -> None:
    """device pointers and the caller's workspace (16-byte aligned, secp256k1_recover_workspace(n) bytes); asynchronous on `stream`
    under the stream contract of the _dev entries (include/sbv.h).  `flags` overrides low_s with a raw flag word."""
    lib = load()
    lib.sbv_secp256k1_recover_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    f = (K256_RECOVER_LOW_S if low_s else 0) if flags is None else flags
    _check(lib.sbv_secp256k1_recover_stream(d_sigs_ptr or None, d_recid_ptr or None, d_digests_ptr or None, n, f, d_pubs_ptr or None,
                                            d_ok_ptr or None, d_work_ptr or None, work_bytes, stream or None))


def debug_secp256k1_recover_op(op: int, records):
    """sbv_debug_secp256k1_recover_op (test only): one case per lane, 192-byte input records -> 128-byte output records (include/sbv.h)"""
    lib = load()
    n = len(records)
    lib.sbv_debug_secp256k1_recover_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(1, 128 * n))
    _check(lib.sbv_debug_secp256k1_recover_op(op, b"".join(records), out, n))
    return [out.raw[128 * i:128 * i + 128] for i in range(n)]


def keccak256_msgs(msgs, offsets=None):
    """sbv_keccak256_msgs: Keccak-256 (Ethereum's keccak256, not SHA3-256) of a list of byte strings -> the list of 32-byte digests.
    With `offsets` (n + 1 integers), `msgs` is instead the messages back to back in one bytes object (None when all are empty) and the
    result is the n x 32 digest bytes in one object: the raw entry, bad offset tables included."""
    lib = load()
    lib.sbv_keccak256_msgs.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    if offsets is None:
        msgs = [bytes(m) for m in msgs]
        offs, blob = [0], b"".join(msgs)
        for m in msgs:
            offs.append(offs[-1] + len(m))
    else:
        offs, blob = list(offsets), msgs
    n = len(offs) - 1
    out = ctypes.create_string_buffer(max(1, 32 * n))
    _check(lib.sbv_keccak256_msgs(blob, (ctypes.c_uint64 * (n + 1))(*offs), n, out))
    return [out.raw[32 * i:32 * i + 32] for i in range(n)] if offsets is None else out.raw[:32 * n]


def keccak256_msgs_stream(d_msgs_ptr: int, d_offsets_ptr: int, n: int, d_digests_ptr: int, stream: int = 0) -> None:
    """device pointers (offsets: n + 1 u64, 8-byte aligned; messages at any alignment); asynchronous on `stream` under the stream
    contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_keccak256_msgs_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_keccak256_msgs_stream(d_msgs_ptr or None, d_offsets_ptr or None, n, d_digests_ptr or None, stream or None))


def secp256k1_addresses(pubs: bytes) -> bytes:
    """sbv_secp256k1_addresses: m x 64 bytes Qx | Qy -> m x 20 bytes, the Ethereum-style addresses Keccak-256(Qx | Qy)[12:]; a pure
    hash, the keys are not checked against the curve"""
    lib = load()
    m = len(pubs) // 64
    if len(pubs) != 64 * m:
        raise ValueError("secp256k1_addresses: pubs is not a whole number of 64-byte keys")
    lib.sbv_secp256k1_addresses.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    addrs = ctypes.create_string_buffer(max(1, 20 * m))
    _check(lib.sbv_secp256k1_addresses(bytes(pubs), m, addrs))
    return addrs.raw[:20 * m]


def secp256k1_addresses_stream(d_pubs_ptr: int, m: int, d_addrs_ptr: int, stream: int = 0) -> None:
    lib = load()
    lib.sbv_secp256k1_addresses_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_addresses_stream(d_pubs_ptr or None, m, d_addrs_ptr or None, stream or None))


def secp256k1_recover_addresses(sigs: bytes, recid: bytes, digests: bytes, low_s: bool = False):
    """sbv_secp256k1_recover_addresses: secp256k1_recover with the signer's 20-byte address in place of the key (what Ethereum's
    ecrecover returns).  Returns (addrs, ok): n x 20 bytes in one object and ok[i] = 1 per recovered signer; a refused input gives
    ok[i] = 0 and 20 zero bytes."""
    lib = load()
    n = len(recid)
    if len(sigs) != 64 * n or len(digests) != 32 * n:
        raise ValueError("secp256k1_recover_addresses: sigs, recid and digests disagree about n")
    lib.sbv_secp256k1_recover_addresses.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32,
                                                    ctypes.c_char_p, ctypes.c_char_p]
    addrs, ok = ctypes.create_string_buffer(max(1, 20 * n)), ctypes.create_string_buffer(max(1, n))
    _check(lib.sbv_secp256k1_recover_addresses(bytes(sigs), bytes(recid), bytes(digests), n, K256_RECOVER_LOW_S if low_s else 0, addrs, ok))
    return addrs.raw[:20 * n], ok.raw[:n]


def secp256k1_recover_addresses_stream(d_sigs_ptr: int, d_recid_ptr: int, d_digests_ptr: int, n: int, d_addrs_ptr: int, d_ok_ptr: int,
                                       d_work_ptr: int, work_bytes: int, low_s: bool = False, stream: int = 0, flags=None) -> None:
    """device pointers and the caller's workspace, exactly as secp256k1_recover_stream; addrs is n x 20 bytes"""
    lib = load()
    lib.sbv_secp256k1_recover_addresses_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_size_t, ctypes.c_void_p]
    f = (K256_RECOVER_LOW_S if low_s else 0) if flags is None else flags
    _check(lib.sbv_secp256k1_recover_addresses_stream(d_sigs_ptr or None, d_recid_ptr or None, d_digests_ptr or None, n, f,
                                                      d_addrs_ptr or None, d_ok_ptr or None, d_work_ptr or None, work_bytes, stream or None))


def debug_keccak_op(op: int, states):
    """sbv_debug_keccak_op (test only): one case per lane, 200-byte states -> 200-byte states (include/sbv.h)"""
    lib = load()
    n = len(states)
    lib.sbv_debug_keccak_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(1, 200 * n))
    _check(lib.sbv_debug_keccak_op(op, b"".join(states), out, n))
    return [out.raw[200 * i:200 * i + 200] for i in range(n)]


def secp256k1_schnorr_verify(pks: bytes, msgs: bytes, sigs: bytes) -> bytes:
    """sbv_secp256k1_schnorr_verify: BIP-340 verification of n signatures (R.x | s, 64 bytes each) of 32-byte messages under x-only
    32-byte keys.  Returns ok: one byte per item, 1 = valid (include/sbv.h has the rules)."""
    lib = load()
    n = len(sigs) // 64
    if len(sigs) != 64 * n or len(pks) != 32 * n or len(msgs) != 32 * n:
        raise ValueError("secp256k1_schnorr_verify: pks, msgs and sigs disagree about n")
    lib.sbv_secp256k1_schnorr_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    ok = ctypes.create_string_buffer(max(1, n))
    _check(lib.sbv_secp256k1_schnorr_verify(bytes(pks), bytes(msgs), bytes(sigs), n, ok))
    return ok.raw[:n]


def secp256k1_schnorr_verify_workspace(n: int) -> int:
    """sbv_secp256k1_schnorr_verify_workspace: the bytes of device workspace secp256k1_schnorr_verify_stream needs for n signatures"""
    lib = load()
    lib.sbv_secp256k1_schnorr_verify_workspace.argtypes = [ctypes.c_size_t]
    lib.sbv_secp256k1_schnorr_verify_workspace.restype = ctypes.c_size_t
    return int(lib.sbv_secp256k1_schnorr_verify_workspace(n))


def secp256k1_schnorr_verify_stream(d_pks_ptr: int, d_msgs_ptr: int, d_sigs_ptr: int, n: int, d_ok_ptr: int, d_work_ptr: int,
                                    work_bytes: int, stream: int = 0) -> None:
    """device pointers and the caller's workspace (16-byte aligned, secp256k1_schnorr_verify_workspace(n) bytes); asynchronous on
    `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_secp256k1_schnorr_verify_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_schnorr_verify_stream(d_pks_ptr or None, d_msgs_ptr or None, d_sigs_ptr or None, n, d_ok_ptr or None,
                                                   d_work_ptr or None, work_bytes, stream or None))


def secp256k1_schnorr_expand_keys(keys: bytes, want_pks: bool = True):
    """sbv_secp256k1_schnorr_expand_keys: 32-byte private scalars -> (expanded, pks, ok): the 64-byte records d | P.x (AS SECRET AS THE
    KEYS) in one bytes object, the x-only public keys in one bytes object (None without want_pks) and ok[i] = 1 per key in [1, n-1]
    (otherwise an all-zero record and key).  NOT constant-time: see include/sbv.h."""
    lib = load()
    m = len(keys) // 32
    lib.sbv_secp256k1_schnorr_expand_keys.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    exp, ok = ctypes.create_string_buffer(max(1, 64 * m)), ctypes.create_string_buffer(max(1, m))
    pks = ctypes.create_string_buffer(max(1, 32 * m)) if want_pks else None
    _check(lib.sbv_secp256k1_schnorr_expand_keys(bytes(keys), m, exp, pks, ok))
    return exp.raw[:64 * m], (pks.raw[:32 * m] if want_pks else None), ok.raw[:m]


def secp256k1_schnorr_expand_keys_stream(d_keys_ptr: int, m: int, d_expanded_ptr: int, d_pks_ptr: int, d_ok_ptr: int, stream: int = 0) -> None:
    """device pointers (d_pks_ptr may be 0); asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_secp256k1_schnorr_expand_keys_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                             ctypes.c_void_p]
    _check(lib.sbv_secp256k1_schnorr_expand_keys_stream(d_keys_ptr or None, m, d_expanded_ptr or None, d_pks_ptr or None, d_ok_ptr or None,
                                                        stream or None))


def secp256k1_schnorr_sign(expanded: bytes, msgs: bytes, aux=None, key_index=None):
    """sbv_secp256k1_schnorr_sign: BIP-340 signatures (R.x | s, 64 bytes each) of n 32-byte messages under the records of
    secp256k1_schnorr_expand_keys (key_index[i], default i % n_keys); aux: n x 32 bytes of auxiliary randomness, None = zero bytes.
    Returns (sigs, ok); a refused record or an index out of range gives ok[i] = 0 and 64 zero bytes.  Records must come from
    secp256k1_schnorr_expand_keys: a record whose P.x does not belong to its d yields signatures that can leak d.  NOT constant-time:
    see include/sbv.h."""
    lib = load()
    n, nk = len(msgs) // 32, len(expanded) // 64
    if aux is not None and len(aux) != 32 * n:
        raise ValueError("secp256k1_schnorr_sign: aux and msgs disagree about n")
    lib.sbv_secp256k1_schnorr_sign.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                               ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    sigs, ok = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
    idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
    _check(lib.sbv_secp256k1_schnorr_sign(bytes(expanded), nk, idx, bytes(msgs), None if aux is None else bytes(aux), n, sigs, ok))
    return sigs.raw[:64 * n], ok.raw[:n]


def secp256k1_schnorr_sign_stream(d_expanded_ptr: int, n_keys: int, d_index_ptr: int, d_msgs_ptr: int, d_aux_ptr: int, n: int,
                                  d_sigs_ptr: int, d_ok_ptr: int, stream: int = 0) -> None:
    """device pointers (d_index_ptr and d_aux_ptr may be 0); asynchronous on `stream` under the stream contract of the _dev entries"""
    lib = load()
    lib.sbv_secp256k1_schnorr_sign_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_schnorr_sign_stream(d_expanded_ptr or None, n_keys, d_index_ptr or None, d_msgs_ptr or None, d_aux_ptr or None, n,
                                                 d_sigs_ptr or None, d_ok_ptr or None, stream or None))


def debug_secp256k1_schnorr_op(op: int, records):
    """sbv_debug_secp256k1_schnorr_op (test only): one case per lane, 192-byte input records -> 128-byte output records (include/sbv.h)"""
    lib = load()
    n = len(records)
    lib.sbv_debug_secp256k1_schnorr_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(1, 128 * n))
    _check(lib.sbv_debug_secp256k1_schnorr_op(op, b"".join(records), out, n))
    return [out.raw[128 * i:128 * i + 128] for i in range(n)]


def secp256k1_schnorr_lift_keys(pks: bytes):
    """sbv_secp256k1_schnorr_lift_keys: x-only 32-byte keys -> (keys64, ok): x | y of lift_x per key in one bytes object, the bytes
    secp256k1_register_keys takes, and ok[i] = 1 per key on the curve (otherwise x | 32 zero bytes, which registers as an invalid slot)."""
    lib = load()
    m = len(pks) // 32
    if len(pks) != 32 * m:
        raise ValueError("secp256k1_schnorr_lift_keys: pks is not a multiple of 32 bytes")
    lib.sbv_secp256k1_schnorr_lift_keys.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    keys, ok = ctypes.create_string_buffer(max(1, 64 * m)), ctypes.create_string_buffer(max(1, m))
    _check(lib.sbv_secp256k1_schnorr_lift_keys(bytes(pks), m, keys, ok))
    return keys.raw[:64 * m], ok.raw[:m]


def secp256k1_schnorr_lift_keys_stream(d_pks_ptr: int, m: int, d_keys64_ptr: int, d_ok_ptr: int, stream: int = 0) -> None:
    """device pointers (d_ok_ptr may be 0); asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_secp256k1_schnorr_lift_keys_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_secp256k1_schnorr_lift_keys_stream(d_pks_ptr or None, m, d_keys64_ptr or None, d_ok_ptr or None, stream or None))


def secp256k1_schnorr_register_keys(pks: bytes):
    """lift + register: x-only 32-byte keys -> (slots, ok).  The slots are those of secp256k1_register_keys (one registry for ECDSA and
    Schnorr); a key off the curve gets a slot too, an invalid one (ok[i] = 0), against which every signature is rejected."""
    keys, ok = secp256k1_schnorr_lift_keys(pks)
    return secp256k1_register_keys([keys[64 * i:64 * i + 64] for i in range(len(ok))]), ok


def secp256k1_schnorr_verify_keyed(msgs: bytes, sigs: bytes, slots) -> bytes:
    """sbv_secp256k1_schnorr_verify_keyed: BIP-340 verification of n signatures (R.x | s) of 32-byte messages under registered keys
    (slots of secp256k1_register_keys / secp256k1_schnorr_register_keys).  Returns ok: one byte per item, 1 = valid; byte for byte
    secp256k1_schnorr_verify with pk = the slot's Qx."""
    lib = load()
    n = len(sigs) // 64
    if len(sigs) != 64 * n or len(msgs) != 32 * n or len(slots) != n:
        raise ValueError("secp256k1_schnorr_verify_keyed: msgs, sigs and slots disagree about n")
    lib.sbv_secp256k1_schnorr_verify_keyed.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    arr = (ctypes.c_uint32 * max(1, n))(*slots)
    ok = ctypes.create_string_buffer(max(1, n))
    _check(lib.sbv_secp256k1_schnorr_verify_keyed(bytes(msgs), bytes(sigs), arr, n, ok))
    return ok.raw[:n]


def secp256k1_schnorr_verify_keyed_stream(d_msgs_ptr: int, d_sigs_ptr: int, d_slots_ptr: int, n: int, d_ok_ptr: int, stream: int = 0) -> None:
    """device pointers; asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h); no workspace"""
    lib = load()
    lib.sbv_secp256k1_schnorr_verify_keyed_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                              ctypes.c_void_p]
    _check(lib.sbv_secp256k1_schnorr_verify_keyed_stream(d_msgs_ptr or None, d_sigs_ptr or None, d_slots_ptr or None, n, d_ok_ptr or None,
                                                         stream or None))


def debug_secp256k1_schnorr_keyed_op(op: int, records, slots):
    """sbv_debug_secp256k1_schnorr_keyed_op (test only): one case per lane, 192-byte input records u1 | u2 and a slot each -> 128-byte
    output records x | y | . | ok of u1 G + u2 Q_slot (include/sbv.h)"""
    lib = load()
    n = len(records)
    if len(slots) != n:
        raise ValueError("debug_secp256k1_schnorr_keyed_op: records and slots disagree about n")
    lib.sbv_debug_secp256k1_schnorr_keyed_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    arr = (ctypes.c_uint32 * max(1, n))(*slots)
    out = ctypes.create_string_buffer(max(1, 128 * n))
    _check(lib.sbv_debug_secp256k1_schnorr_keyed_op(op, b"".join(records), arr, out, n))
    return [out.raw[128 * i:128 * i + 128] for i in range(n)]


def ed25519_expand_keys(seeds):
    """sbv_ed25519_expand_keys: 32-byte seeds (a list, or their concatenation) -> (expanded, pks): the 96-byte expanded records
    (a mod L | prefix | A_enc, as secret as the seeds) in one bytes object, and the list of 32-byte public keys."""
    lib = load()
    blob = seeds if isinstance(seeds, (bytes, bytearray)) else b"".join(seeds)
    if len(blob) % 32:
        raise ValueError("seeds are 32 bytes each")
    m = len(blob) // 32
    lib.sbv_ed25519_expand_keys.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    exp, pks = ctypes.create_string_buffer(max(1, 96 * m)), ctypes.create_string_buffer(max(1, 32 * m))
    _check(lib.sbv_ed25519_expand_keys(bytes(blob), m, exp, pks))
    return exp.raw[:96 * m], [pks.raw[32 * i:32 * i + 32] for i in range(m)]


def ed25519_sign_msgs(expanded: bytes, msgs, key_index=None):
    """sbv_ed25519_sign_msgs: RFC 8032 signatures (R | S, 64 bytes each) of the messages under the expanded records
    (key_index[i], default i % n_keys).  Returns (sigs, ok): a list of signatures and ok[i] = 1 per produced one (an index out of
    range gives ok[i] = 0 and 64 zero bytes).  NOT constant-time: see include/sbv.h."""
    lib = load()
    n, nk = len(msgs), len(expanded) // 96
    offs = (ctypes.c_uint64 * (n + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        offs[i] = acc
        acc += len(m)
    offs[n] = acc
    lib.sbv_ed25519_sign_msgs.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    sigs, ok = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
    idx = None if key_index is None else (ctypes.c_uint32 * n)(*key_index)
    _check(lib.sbv_ed25519_sign_msgs(expanded, nk, idx, b"".join(msgs), offs, n, sigs, ok))
    return [sigs.raw[64 * i:64 * i + 64] for i in range(n)], ok.raw[:n]


def ed25519_sign(seeds, msgs, key_index=None):
    """expand the seeds, then sign: (sigs, ok) as ed25519_sign_msgs returns them"""
    expanded, _ = ed25519_expand_keys(seeds)
    return ed25519_sign_msgs(expanded, msgs, key_index)


def ed25519_expand_keys_stream(d_seeds_ptr: int, m: int, d_expanded_ptr: int, d_pks_ptr: int = 0, stream: int = 0) -> None:
    lib = load()
    lib.sbv_ed25519_expand_keys_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_ed25519_expand_keys_stream(d_seeds_ptr, m, d_expanded_ptr, d_pks_ptr or None, stream or None))


def ed25519_sign_msgs_stream(d_expanded_ptr: int, n_keys: int, d_index_ptr: int, d_msgs_ptr: int, d_offsets_ptr: int, n: int,
                             d_sigs_ptr: int, d_ok_ptr: int, stream: int = 0) -> None:
    """device pointers; asynchronous on `stream` under the stream contract of the _dev entries (include/sbv.h)"""
    lib = load()
    lib.sbv_ed25519_sign_msgs_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(lib.sbv_ed25519_sign_msgs_stream(d_expanded_ptr, n_keys, d_index_ptr or None, d_msgs_ptr or None, d_offsets_ptr, n, d_sigs_ptr,
                                            d_ok_ptr, stream or None))


def debug_ed25519_sign_op(op: int, blobs):
    """sbv_debug_ed25519_sign_op (test only): one case per lane; op 0 takes 96-byte inputs, ops 1 and 2 32-byte ones -> 32-byte outputs"""
    lib = load()
    n = len(blobs)
    lib.sbv_debug_ed25519_sign_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(1, 32 * n))
    _check(lib.sbv_debug_ed25519_sign_op(op, b"".join(blobs), out, n))
    return [out.raw[32 * i:32 * i + 32] for i in range(n)]


def key_cache_stats(scheme: int = SCHEME_P256):
    """(cached keys, groups of the last grouped batch that hit, that missed, capacity)"""
    out = (ctypes.c_uint32 * 4)()
    lib = load()
    lib.sbv_key_cache_stats.argtypes = [ctypes.c_int, ctypes.c_void_p]
    _check(lib.sbv_key_cache_stats(scheme, out))
    return out[0], out[1], out[2], out[3]


def parse_der(sig: bytes) -> Optional[bytes]:
    """Strict DER -> r|s (64 bytes), or None when Go's parseSignature would fail."""
    out = ctypes.create_string_buffer(64)
    rc = load().sbv_p256_parse_der(sig, len(sig), out)
    if rc == SBV_OK:
        return out.raw
    if rc == -6:
        return None
    _check(rc)
    return None


def sha256_batch(msgs) -> bytes:
    blob = b"".join(msgs)
    offs = (ctypes.c_uint64 * (len(msgs) + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        offs[i] = acc
        acc += len(m)
    offs[len(msgs)] = acc
    out = ctypes.create_string_buffer(32 * max(1, len(msgs)))
    _check(load().sbv_sha256_batch(blob, offs, len(msgs), out))
    return out.raw[:32 * len(msgs)]


def host_alloc(nbytes: int) -> int:
    """Page-locked host memory for the host-pointer entries (sbv_host_alloc); returns the address, 0 on failure."""
    lib = load()
    lib.sbv_host_alloc.restype = ctypes.c_void_p
    lib.sbv_host_alloc.argtypes = [ctypes.c_size_t]
    return lib.sbv_host_alloc(nbytes) or 0


def host_free(ptr: int) -> None:
    lib = load()
    lib.sbv_host_free.argtypes = [ctypes.c_void_p]
    lib.sbv_host_free(ptr)


class ShardInfo(ctypes.Structure):
    _fields_ = [("devices", ctypes.c_int), ("shards", ctypes.c_int), ("mode", ctypes.c_int), ("tuples_per_shard", ctypes.c_size_t),
                ("h2d_us", ctypes.c_double), ("kernels_us", ctypes.c_double), ("gather_us", ctypes.c_double), ("total_us", ctypes.c_double)]


def init_all() -> int:
    """Initialise every visible gfx950 device (sbv_init_all); returns how many."""
    n = load().sbv_init_all()
    if n < 0:
        _check(n)
    return n


def shard_plan(n: int, devices: int, group: int = 0, min_per_device: int = 0):
    """The pure split of sbv_p256_verify_batch_sharded: list of shard start indices + [n]."""
    lib = load()
    lib.sbv_shard_plan.restype = ctypes.c_size_t
    lib.sbv_shard_plan.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    first = (ctypes.c_size_t * 17)()
    k = lib.sbv_shard_plan(n, devices, group, min_per_device, first)
    return [first[i] for i in range(k + 1)]


def shard_min_for(tuples, n: int, group: int = 0) -> int:
    """sbv_shard_min_for: the per-device minimum the sharded entry plans this host batch with (few signers -> 2^16, else 2^17)."""
    lib = load()
    lib.sbv_shard_min_for.restype = ctypes.c_size_t
    lib.sbv_shard_min_for.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]
    if isinstance(tuples, int):
        return lib.sbv_shard_min_for(tuples, n, group)
    buf = (ctypes.c_char * len(tuples)).from_buffer_copy(tuples) if not isinstance(tuples, ctypes.Array) else tuples
    return lib.sbv_shard_min_for(ctypes.addressof(buf), n, group)


def verify_batch_sharded(host_ptr: int, n: int, out_ptr: int, group: int = 0, quorum: int = 0, quorum_out_ptr: int = 0) -> ShardInfo:
    """sbv_p256_verify_batch_sharded on raw pointers (numpy / ctypes buffers)."""
    lib = load()
    lib.sbv_p256_verify_batch_sharded.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.POINTER(ShardInfo)]
    info = ShardInfo()
    _check(lib.sbv_p256_verify_batch_sharded(host_ptr, n, group, quorum, out_ptr, quorum_out_ptr or None, ctypes.byref(info)))
    return info


def verify_batch_keyed_sharded(rsh_ptr: int, slots_ptr: int, n: int, out_ptr: int, group: int = 0, quorum: int = 0,
                               quorum_out_ptr: int = 0) -> ShardInfo:
    """sbv_p256_verify_batch_keyed_sharded on raw pointers: n x 96-byte records r | s | hash + n u32 key slots, split over every
    initialised device (each holds a replica of the key registry and of the consenters' wide combs); quorum bits by distinct slot."""
    lib = load()
    lib.sbv_p256_verify_batch_keyed_sharded.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ShardInfo)]
    info = ShardInfo()
    _check(lib.sbv_p256_verify_batch_keyed_sharded(rsh_ptr, slots_ptr, n, group, quorum, out_ptr, quorum_out_ptr or None, ctypes.byref(info)))
    return info


def verify_msgs_keyed_sharded(msgs, sigs_der, slots, group: int = 0, quorum: int = 0, offsets=None):
    """sbv_p256_verify_msgs_keyed_sharded: raw messages + DER signatures + key slots over every initialised device, SHA-256 and the
    DER parse on the devices, uploads in pieces.  Returns (accept bitmap, quorum bitmap or None, ShardInfo).
    offsets = (msg_offsets, sig_offsets): use these tables instead of the ones the byte strings imply (tests of malformed tables)."""
    lib = load()
    lib.sbv_p256_verify_msgs_keyed_sharded.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.POINTER(ShardInfo)]
    n = len(msgs)
    mo = (ctypes.c_uint64 * (n + 1))()
    so = (ctypes.c_uint64 * (n + 1))()
    a = b = 0
    for i in range(n):
        mo[i], so[i] = a, b
        a += len(msgs[i]); b += len(sigs_der[i])
    mo[n], so[n] = a, b
    if offsets is not None:
        for i in range(n + 1):
            mo[i], so[i] = offsets[0][i], offsets[1][i]
    arr = (ctypes.c_uint32 * max(1, n))(*slots)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    props = n // group if group else 0
    qout = ctypes.create_string_buffer(max(1, (props + 7) // 8)) if group and quorum else None
    info = ShardInfo()
    _check(lib.sbv_p256_verify_msgs_keyed_sharded(b"".join(msgs), mo, b"".join(sigs_der), so, arr, n, group, quorum, out, qout, ctypes.byref(info)))
    return out.raw[:(n + 7) // 8], (qout.raw[:(props + 7) // 8] if qout is not None else None), info


def verify_msgs_sharded(msgs, sigs_der, keys, group: int = 0, quorum: int = 0, offsets=None):
    """sbv_p256_verify_msgs_sharded: raw messages + DER signatures + the signers' keys over every initialised device (always the
    contiguous split), SHA-256 and the DER parse on the devices, uploads in pieces.  Returns (accept bitmap, quorum bitmap or None,
    ShardInfo).  offsets = (msg_offsets, sig_offsets): use these tables instead of the ones the byte strings imply."""
    lib = load()
    lib.sbv_p256_verify_msgs_sharded.argtypes = _MSGS_ARGS + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                                              ctypes.POINTER(ShardInfo)]
    n, mo, so, kb = _msgs_tables(msgs, sigs_der, keys, offsets)
    out = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    props = n // group if group else 0
    qout = ctypes.create_string_buffer(max(1, (props + 7) // 8)) if group and quorum else None
    info = ShardInfo()
    _check(lib.sbv_p256_verify_msgs_sharded(b"".join(msgs), mo, b"".join(sigs_der), so, kb, n, group, quorum, out, qout, ctypes.byref(info)))
    return out.raw[:(n + 7) // 8], (qout.raw[:(props + 7) // 8] if qout is not None else None), info


def shard_mode(by_key: bool, parts: int = 0) -> None:
    """sbv_shard_mode: how the sharded entry partitions a batch that spans devices (contiguous ranges / by key hash); parts = 0
    means one part per device, more parts than devices run one after another on their device."""
    lib = load()
    lib.sbv_shard_mode.argtypes = [ctypes.c_int, ctypes.c_uint]
    _check(lib.sbv_shard_mode(1 if by_key else 0, parts))


def verify_batch_dev_part(d_tuples_ptr: int, n: int, part: int, parts: int, d_bitmap_words_ptr: int, stream: int = 0) -> int:
    """sbv_p256_verify_batch_dev_part: part `part` of `parts` (by key hash) of n device-resident tuples; the bitmap (ceil(n/32)
    words) receives that part's verdict bits.  Returns how many tuples the part held."""
    lib = load()
    lib.sbv_p256_verify_batch_dev_part.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    members = ctypes.c_size_t(0)
    _check(lib.sbv_p256_verify_batch_dev_part(d_tuples_ptr, n, part, parts, d_bitmap_words_ptr, stream, ctypes.byref(members)))
    return members.value


def verify_batch_on(device: int, host_ptr: int, n: int, out_ptr: int) -> None:
    lib = load()
    lib.sbv_p256_verify_batch_on.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _check(lib.sbv_p256_verify_batch_on(device, host_ptr, n, out_ptr))


def last_timing() -> Timing:
    t = Timing()
    _check(load().sbv_last_timing(ctypes.byref(t)))
    return t


def profile_enable(on) -> None:
    """True / 1: step triples + dominant-kernel pairs; 2: dominant-kernel pairs only; False / 0: off."""
    _check(load().sbv_profile_enable(2 if on == 2 else (1 if on else 0)))


def profile_read():
    """(prep_us_sum, verify_us_sum, launches) of the device-pointer calls since the last read."""
    p, v, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
    _check(load().sbv_profile_read(ctypes.byref(p), ctypes.byref(v), ctypes.byref(k)))
    return p.value, v.value, k.value


def profile_read_dominant():
    """(summed duration in us, number of launches) of the dominant stage-B kernel since profiling was enabled;
    call before profile_read()."""
    d = ctypes.c_double()
    k = ctypes.c_uint64()
    _check(load().sbv_profile_read_dominant(ctypes.byref(d), ctypes.byref(k)))
    return d.value, k.value


def last_group_stats():
    """(key groups, tuples through the per-batch key tables, tuples through the generic kernel, ungrouped tuples
    rejected for their public key alone) of the last grouped batch."""
    out = (ctypes.c_uint32 * 4)()
    _check(load().sbv_p256_last_group_stats(out))
    return out[0], out[1], out[2], out[3]


def last_table_classes():
    """(groups verified from a full table, groups filled in this batch, grouped tuples served by the rows-only pass) of the last grouped
    P-256 batch (sbv_p256_last_table_classes)."""
    out = (ctypes.c_uint32 * 3)()
    lib = load()
    lib.sbv_p256_last_table_classes.argtypes = [ctypes.c_void_p]
    _check(lib.sbv_p256_last_table_classes(out))
    return out[0], out[1], out[2]


def pool_stats():
    """sbv_p256_pool_stats: dict of the grouped step's pools on the default device (cached keys, groups per batch, shrunk, fallbacks for
    lack of memory, hot-key combs, contexts sharing the GPU)."""
    out = (ctypes.c_uint32 * 6)()
    lib = load()
    lib.sbv_p256_pool_stats.argtypes = [ctypes.c_void_p]
    _check(lib.sbv_p256_pool_stats(out))
    return {"cache_keys": out[0], "groups_per_batch": out[1], "shrunk": bool(out[2]), "nomem_fallbacks": out[3], "hot_pool": out[4], "gpu_share": out[5]}


def debug_hot_check(device: int = 0):
    """sbv_debug_hot_check: tuple of the 8 diagnostic words for context `device` (slow: a host build per promoted comb)."""
    out = (ctypes.c_uint32 * 8)()
    lib = load()
    lib.sbv_debug_hot_check.argtypes = [ctypes.c_int, ctypes.c_void_p]
    _check(lib.sbv_debug_hot_check(device, out))
    return tuple(out)


GROUP_ARRAYS = ("ht", "rep", "cnt", "slot_of", "group_rep", "counters", "slots", "grp_idx", "grp_of", "ung_idx", "ung_cand", "gcount", "gcursor",
                "tslot", "cold", "acc", "cache_keys", "cache_count")       # SBV_GROUP_ARRAY_* of include/sbv.h, in order
GROUP_HEADER = ("scheme", "n", "ht_mask", "max_groups", "min_count", "sample_mask", "min_samples", "seed", "sorted", "kc_cap", "kc_enabled", "serial",
                "groups", "cached")


def debug_group_header(device: int = 0):
    """sbv_debug_group_header: the 16 header words of the last grouped launch of context `device` (word 0 = 0xFFFFFFFF: none yet;
    word 11 = the serial number of grouped launches)."""
    out = (ctypes.c_uint32 * 16)()
    _check(_call("sbv_debug_group_header", [ctypes.c_int, _PTR], device, out))
    return tuple(out)


def group_readout_from(header, array):
    """The read-out dict of a grouped step from a pair of entries shaped like sbv_debug_group_header / sbv_debug_group_array
    (header() -> 16 words, array(which, count, address) -> 0): the header fields by name and one numpy array per GROUP_ARRAYS name, each
    cut to the length the counters give it.  None before the first grouped launch.  (The test emulator exports the same pair.)"""
    import numpy as np
    h = header()
    if h[0] == 0xFFFFFFFF:
        return None
    ro = {name: int(h[i]) for i, name in enumerate(GROUP_HEADER)}

    def get(name, count, dtype=np.uint32):
        out = np.zeros(max(int(count), 1), dtype=dtype)
        rc = array(GROUP_ARRAYS.index(name), int(count), out.ctypes.data)
        if rc != SBV_OK:
            raise SbvError(rc, f"group read-out of {name}[{count}]")
        return out[:int(count)]

    n, groups, srt = ro["n"], ro["groups"], ro["sorted"]
    c = ro["counters"] = get("counters", 12)
    ro["ht"] = get("ht", ro["ht_mask"] + 1)
    for name in ("rep", "cnt", "slot_of", "slots"):
        ro[name] = get(name, n)
    ro["acc"] = get("acc", n, np.uint8)
    ro["group_rep"], ro["tslot"], ro["cold"] = get("group_rep", groups), get("tslot", groups), get("cold", groups, np.uint8)
    ro["grp_idx"] = get("grp_idx", min(int(c[1]), n))
    ro["ung_idx"] = get("ung_idx", min(int(c[2]), n))
    ro["grp_of"] = get("grp_of", min(int(c[1]), n) if srt else 0)
    ro["ung_cand"] = get("ung_cand", min(int(c[4]), n) if srt else 0)
    ro["gcount"], ro["gcursor"] = get("gcount", groups if srt else 0), get("gcursor", groups if srt else 0)
    ro["cache_count"] = get("cache_count", 4)
    ro["cache_keys"] = get("cache_keys", min(int(ro["cache_count"][0]), ro["kc_cap"]) * 16).reshape(-1, 16)
    return ro


def debug_group_readout(device: int = 0):
    """sbv_debug_group_header + sbv_debug_group_array: what the LAST grouped launch of any scheme left in context `device` — the grouping
    table, representatives, counts, lists, sort cursors, table slots, verdict bytes and the scheme's cached keys — as a dict of header
    fields and numpy arrays (group_readout_from).  Tests and tools only: it waits for the device and copies every array."""
    load()
    return group_readout_from(lambda: debug_group_header(device),
                              lambda which, count, addr: _call("sbv_debug_group_array", [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, _PTR], device, which, count, addr))


def hot_keys(max_keys: int = 1024, min_hits: int = 0) -> None:
    """sbv_p256_hot_keys: wide combs for hot cache slots of the generic path (0 keys = off)."""
    lib = load()
    lib.sbv_p256_hot_keys.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    _check(lib.sbv_p256_hot_keys(max_keys, min_hits))


def hot_key_stats():
    """(promoted keys, pool capacity, tuples of the last grouped batch served by the wide pass, min_hits)"""
    out = (ctypes.c_uint32 * 4)()
    lib = load()
    lib.sbv_p256_hot_key_stats.argtypes = [ctypes.c_void_p]
    _check(lib.sbv_p256_hot_key_stats(out))
    return out[0], out[1], out[2], out[3]


def hot_selfcheck(index: int) -> bool:
    lib = load()
    lib.sbv_p256_hot_selfcheck.argtypes = [ctypes.c_uint32]
    rc = lib.sbv_p256_hot_selfcheck(index)
    if rc < 0:
        _check(rc)
    return rc == 1


def ed_hot_keys(max_keys: int = 1024, min_hits: int = 0) -> None:
    """sbv_ed25519_hot_keys: 16-bit combs of -A for hot cache slots of the Ed25519 variant (0 keys = off)."""
    lib = load()
    lib.sbv_ed25519_hot_keys.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    _check(lib.sbv_ed25519_hot_keys(max_keys, min_hits))


def ed_hot_key_stats():
    """(promoted keys, pool capacity, tuples of the last grouped Ed25519 batch served by the wide pass, min_hits)"""
    out = (ctypes.c_uint32 * 4)()
    lib = load()
    lib.sbv_ed25519_hot_key_stats.argtypes = [ctypes.c_void_p]
    _check(lib.sbv_ed25519_hot_key_stats(out))
    return out[0], out[1], out[2], out[3]


def ed_hot_selfcheck(index: int) -> bool:
    lib = load()
    lib.sbv_ed25519_hot_selfcheck.argtypes = [ctypes.c_uint32]
    rc = lib.sbv_ed25519_hot_selfcheck(index)
    if rc < 0:
        _check(rc)
    return rc == 1


def k256_hot_keys(max_keys: int = 1024, min_hits: int = 0) -> None:
    """sbv_secp256k1_hot_keys: 16-bit combs of Q for hot cache slots of the secp256k1 variant (off by default; 0 keys = off)."""
    lib = load()
    lib.sbv_secp256k1_hot_keys.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    _check(lib.sbv_secp256k1_hot_keys(max_keys, min_hits))


def k256_hot_key_stats():
    """(promoted keys, pool capacity, tuples of the last grouped secp256k1 batch served by the wide pass, min_hits)"""
    out = (ctypes.c_uint32 * 4)()
    lib = load()
    lib.sbv_secp256k1_hot_key_stats.argtypes = [ctypes.c_void_p]
    _check(lib.sbv_secp256k1_hot_key_stats(out))
    return out[0], out[1], out[2], out[3]


def k256_hot_selfcheck(index: int) -> bool:
    lib = load()
    lib.sbv_secp256k1_hot_selfcheck.argtypes = [ctypes.c_uint32]
    rc = lib.sbv_secp256k1_hot_selfcheck(index)
    if rc < 0:
        _check(rc)
    return rc == 1


def bitmap_to_list(bm: bytes, n: int):
    return [bool((bm[i >> 3] >> (i & 7)) & 1) for i in range(n)]
