"""CPU tier: the Go adapter (go/gpuverifier) cannot be compiled here (no Go toolchain in the image), so what CAN be checked
mechanically is: every cgo call site against include/sbv.h (tools/check_cgo.py: the function exists, arity, pointer kinds and
element types), that the checker really catches a wrong call, the method set of api.Verifier / api.Signer /
api.RequestInspector (pkg/api/dependencies.go:46-83 of the reference) signature for signature, and that every file is at
least lexically sound (balanced brackets outside strings and comments, one package clause)."""
import json
import os
import re
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_cgo  # noqa: E402

GO = os.path.join(ROOT, "go", "gpuverifier")
HEADER = os.path.join(ROOT, "include", "sbv.h")


def test_every_cgo_call_matches_the_header():
    seen, problems, protos = check_cgo.check(GO, HEADER)
    assert not problems, problems
    assert seen >= 10                                           # init / shutdown / last_error + the eight work entries
    called = {name for fn in os.listdir(GO) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(GO, fn)).read())}
    # the routes VERDICT r2 (#3) asked the adapter to reach
    for need in ("sbv_p256_register_keys", "sbv_p256_verify_msgs_keyed", "sbv_p256_verify_batch_keyed", "sbv_p256_verify_batch_sharded",
                 "sbv_ed25519_verify_msgs", "sbv_secp256k1_verify_batch", "sbv_p256_sign_batch", "sbv_p256_parse_der", "sbv_init_all"):
        assert need in called, need
        assert need in protos, need


def test_the_checker_catches_wrong_calls(tmp_path):
    d = tmp_path / "gpuverifier"
    shutil.copytree(GO, d)
    p = d / "backend_cgo.go"
    src = p.read_text()
    bad = src.replace("C.sbv_secp256k1_verify_batch(u8(buf), C.size_t(n), u8(bitmap))", "C.sbv_secp256k1_verify_batch(u8(buf), u8(bitmap))")
    bad = bad.replace("(*C.uint32_t)(unsafe.Pointer(&slots[0])), C.size_t(n), u8(bitmap)", "(*C.uint64_t)(unsafe.Pointer(&slots[0])), C.size_t(n), u8(bitmap)")
    bad = bad.replace("C.sbv_shutdown()", "C.sbv_shut_down()")
    bad = bad.replace("C.size_t(len(it.Sig))", "len(it.Sig)")
    assert bad != src
    p.write_text(bad)
    _, problems, _ = check_cgo.check(str(d), HEADER)
    text = "\n".join(problems)
    assert "2 arguments, the header declares 3" in text
    assert "is not a uint32_t* expression" in text
    assert "sbv_shut_down: not declared" in text
    assert "should be C.size_t" in text
    assert len(problems) == 4, problems


API = {   # pkg/api/dependencies.go:46-83, Go signatures with the reference's own type names
    "Verifier": ["VerifyProposal(p bft.Proposal) ([]bft.RequestInfo, error)", "VerifyRequest(raw []byte) (bft.RequestInfo, error)",
                 "VerifyConsenterSig(s bft.Signature, prop bft.Proposal) ([]byte, error)", "VerifySignature(s bft.Signature) error",
                 "VerificationSequence() uint64", "RequestsFromProposal(p bft.Proposal) []bft.RequestInfo", "AuxiliaryData(msg []byte) []byte",
                 "RequestID(raw []byte) bft.RequestInfo"],
    "Signer": ["Sign(msg []byte) []byte", "SignProposal(p bft.Proposal, auxiliaryInput []byte) *bft.Signature"],
}


def _shape(sig):
    """method signature -> (name, parameter types, result types), names dropped"""
    m = re.match(r"(\w+)\((.*?)\)\s*(.*)$", sig.strip())
    name, params, res = m.group(1), m.group(2), m.group(3).strip()
    ptypes = [p.strip().split()[-1] for p in params.split(",") if p.strip()]
    rtypes = [r.strip().split()[-1] for r in res.strip("()").split(",") if r.strip()]
    return name, ptypes, rtypes


def test_api_method_sets_match_the_reference_interfaces():
    for recv, fn in (("Verifier", "verifier.go"), ("Signer", "signer.go")):
        src = open(os.path.join(GO, fn)).read()
        have = {}
        for m in re.finditer(r"^func \(\w+ \*" + recv + r"\) (\w+\(.*?\).*?) \{$", src, flags=re.M):
            n, p, r = _shape(m.group(1))
            have[n] = (p, r)
        for want in API[recv]:
            n, p, r = _shape(want)
            assert n in have, (recv, n)
            assert have[n] == (p, r), (recv, n, have[n], (p, r))
    # the reference's interfaces, method by method (tests/golden/reference_api_interfaces.json, taken from pkg/api/dependencies.go)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_api_interfaces.json")))["interfaces"]
    for iface, methods in (("Verifier", API["Verifier"][:7]), ("Signer", API["Signer"]), ("RequestInspector", API["Verifier"][7:])):
        rmethods = {n: ([t.replace("types.", "bft.") for t in m["params"]], [t.replace("types.", "bft.") for t in m["results"]])
                    for n, m in ref[iface].items()}
        assert set(rmethods) == {_shape(m)[0] for m in methods}, (iface, sorted(rmethods))
        for m in methods:
            n, p, r = _shape(m)
            assert rmethods[n] == (p, r), (iface, n, rmethods[n], (p, r))


def _strip(src):
    """drop comments, string / rune / raw-string literals"""
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if src.startswith("//", i):
            i = src.find("\n", i) if "\n" in src[i:] else n
        elif src.startswith("/*", i):
            i = src.find("*/", i) + 2
        elif c == "`":
            i = src.find("`", i + 1) + 1
        elif c in "\"'":
            j = i + 1
            while src[j] != c:
                j += 2 if src[j] == "\\" else 1
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


def test_go_files_are_lexically_sound():
    pairs = {")": "(", "]": "[", "}": "{"}
    for fn in sorted(os.listdir(GO)):
        if not fn.endswith(".go"):
            continue
        code = _strip(open(os.path.join(GO, fn)).read())
        assert len(re.findall(r"^package gpuverifier$", code, flags=re.M)) == 1, fn
        stack = []
        for ch in code:
            if ch in "([{":
                stack.append(ch)
            elif ch in ")]}":
                assert stack and stack.pop() == pairs[ch], fn
        assert not stack, fn
        # every imported package is used, every used stdlib selector is imported (the two mistakes a compiler would stop at first)
        imports = re.findall(r'^\s*(?:(\w+)\s+)?"([\w./-]+)"$', open(os.path.join(GO, fn)).read(), flags=re.M)
        imports = [(a, p_) for a, p_ in imports if p_ != "C"]
        for alias, path in imports:
            name = alias or path.split("/")[-1]
            assert re.search(r"\b" + re.escape(name) + r"\.", code), (fn, "unused import", path)
        for name in ("sha256", "ecdsa", "ed25519", "binary", "errors", "runtime", "sync", "atomic", "time", "asn1", "big", "unsafe", "bytes", "fmt", "rand", "elliptic", "assert"):
            if re.search(r"(?<![\w.])" + name + r"\.\w", code):
                assert any((alias or path.split("/")[-1]) == name for alias, path in imports), (fn, "missing import", name)
