// msgs_generic_emul.cc — CPU TEST TIER ONLY: the lane of the generic verifiers' message front end (consensus_amd/csrc/sha256_dev.h:
// msg_frontend_tuple_lane) and a host model of its kernel (msg_frontend_kernels.hip: k_msg_frontend_tuples), lane by lane.
//
// Compiles the lane code the gfx950 kernel is built from with g++.  Every lane runs on heap copies of EXACTLY its inputs — the message
// in mlen bytes, the signature in dlen bytes (no buffer at all for an empty one), the key in 64 bytes — and writes into exactly 160
// bytes, so that a sanitizer build sees any byte read outside msg[0 .. len), der[0 .. dlen) and key[0 .. 64).  The kernel model takes
// what the kernel takes (packed bytes, both offset tables, the bases and the uploaded sizes), applies the lane's slice check and reads
// the tables and the key array through exact copies as well.  Not part of libsbv.so, never shipped, not a fallback.
//
// With -DSBV_EMUL_MAIN the file is a program of its own (so that a sanitizer build needs nothing loaded into an interpreter):
//     msgs_generic_emul CASES
// CASES holds one case per line, four hex fields separated by blanks ("-" is the empty string): message, signature bytes, key, the
// expected 160-byte tuple.  Every case runs through the lane alone; then all of them run through the kernel model in one batch, packed
// back to back, once with honest tables and once per bent table (an offset below the base, above the upload, decreasing), where the
// bent lane must answer the tuple of an empty message and an empty signature and every other lane its own.  Exit status 0 = every byte
// matched.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../consensus_amd/csrc/sha256_dev.h"

using namespace sbv;

namespace {

// a heap copy of exactly n bytes; null for n == 0
uint8_t* exact(const uint8_t* p, size_t n) {
    if (n == 0) return nullptr;
    uint8_t* q = (uint8_t*)malloc(n);
    memcpy(q, p, n);
    return q;
}

void lane(const uint8_t* msg, size_t mlen, const uint8_t* der, size_t dlen, const uint8_t* key64, uint8_t* out160) {
    uint8_t *m = exact(msg, mlen), *d = exact(der, dlen), *k = exact(key64, 64);
    u32* t = (u32*)malloc(160);
    msg_frontend_tuple_lane(m, mlen, d, dlen, reinterpret_cast<const u32*>(k), t);
    memcpy(out160, t, 160);
    free(t); free(k); free(d); free(m);
}

void kernel(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n,
            uint8_t* tuples, uint64_t mbase, uint64_t sbase, uint64_t mbytes, uint64_t sbytes) {
    uint8_t *um = exact(msgs, mbytes), *us = exact(sigs, sbytes), *uk = exact(keys, n * 64);          // the uploads
    uint64_t* mo = (uint64_t*)exact((const uint8_t*)moff, (n + 1) * 8);
    uint64_t* so = (uint64_t*)exact((const uint8_t*)soff, (n + 1) * 8);
    for (size_t i = 0; i < n; ++i) {
        uint64_t m0 = mo[i] - mbase, m1 = mo[i + 1] - mbase, s0 = so[i] - sbase, s1 = so[i + 1] - sbase;
        if (!(m0 <= m1 && m1 <= mbytes && s0 <= s1 && s1 <= sbytes)) { m0 = m1 = 0; s0 = s1 = 0; }
        lane(m1 > m0 ? um + m0 : nullptr, (size_t)(m1 - m0), s1 > s0 ? us + s0 : nullptr, (size_t)(s1 - s0), uk + 64 * i, tuples + 160 * i);
    }
    free(so); free(mo); free(uk); free(us); free(um);
}

}  // namespace

extern "C" {
void sbvmg_lane(const uint8_t* msg, size_t mlen, const uint8_t* der, size_t dlen, const uint8_t* key64, uint8_t* out160) {
    lane(msg, mlen, der, dlen, key64, out160);
}
void sbvmg_kernel(const uint8_t* msgs, const uint64_t* moff, const uint8_t* sigs, const uint64_t* soff, const uint8_t* keys, size_t n,
                  uint8_t* tuples, uint64_t mbase, uint64_t sbase, uint64_t mbytes, uint64_t sbytes) {
    kernel(msgs, moff, sigs, soff, keys, n, tuples, mbase, sbase, mbytes, sbytes);
}
}

#ifdef SBV_EMUL_MAIN
namespace {
std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}
const char* kEmptyHash = "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855";
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<std::vector<uint8_t>> msgs, sigs, keys, want;
    {
        std::string line;
        int ch;
        auto flush = [&]() {
            if (line.empty()) return true;
            std::vector<std::string> fld;
            size_t at = 0;
            while (at < line.size()) {
                size_t e = line.find(' ', at);
                if (e == std::string::npos) e = line.size();
                fld.push_back(line.substr(at, e - at));
                at = e + 1;
            }
            line.clear();
            if (fld.size() != 4) return false;
            msgs.push_back(unhex(fld[0])); sigs.push_back(unhex(fld[1])); keys.push_back(unhex(fld[2])); want.push_back(unhex(fld[3]));
            return keys.back().size() == 64 && want.back().size() == 160;
        };
        while ((ch = fgetc(f)) != EOF) {
            if (ch == '\n') { if (!flush()) { fprintf(stderr, "bad line %zu\n", msgs.size() + 1); return 2; } }
            else line.push_back((char)ch);
        }
        if (!flush()) { fprintf(stderr, "bad last line\n"); return 2; }
        fclose(f);
    }
    const size_t n = msgs.size();
    size_t bad = 0;
    // every case through the lane alone
    for (size_t i = 0; i < n; ++i) {
        uint8_t* out = (uint8_t*)malloc(160);
        lane(msgs[i].data(), msgs[i].size(), sigs[i].data(), sigs[i].size(), keys[i].data(), out);
        if (memcmp(out, want[i].data(), 160)) { fprintf(stderr, "lane: case %zu differs\n", i); ++bad; }
        free(out);
    }
    // the kernel model: one batch, honest tables, then bent ones; the bases are not 0, as for a piece of a larger batch
    const uint64_t mbase = 1000, sbase = 77;
    std::vector<uint8_t> mblob, sblob, kblob;
    std::vector<uint64_t> mo(n + 1), so(n + 1);
    for (size_t i = 0; i < n; ++i) {
        mo[i] = mbase + mblob.size(); so[i] = sbase + sblob.size();
        mblob.insert(mblob.end(), msgs[i].begin(), msgs[i].end());
        sblob.insert(sblob.end(), sigs[i].begin(), sigs[i].end());
        kblob.insert(kblob.end(), keys[i].begin(), keys[i].end());
    }
    mo[n] = mbase + mblob.size(); so[n] = sbase + sblob.size();
    const std::vector<uint8_t> empty_hash = unhex(kEmptyHash);
    struct Bend { const char* name; int table; size_t at; uint64_t value; };
    const size_t mid = n / 2;
    std::vector<Bend> bends = {{"honest", -1, 0, 0}};
    if (n >= 4) {
        bends.push_back({"message offset below the base", 0, mid, mbase - 1});
        bends.push_back({"message offset above the upload", 0, mid + 1, mbase + mblob.size() + 1});
        bends.push_back({"message offset decreasing", 0, mid + 1, mo[mid] - (mo[mid] > mbase ? 1 : 0)});
        bends.push_back({"signature offset below the base", 1, mid, sbase - 1});
        bends.push_back({"signature offset above the upload", 1, mid + 1, sbase + sblob.size() + 1});
        bends.push_back({"signature offset decreasing", 1, mid + 1, so[mid] - 1});
    }
    for (const Bend& b : bends) {
        std::vector<uint64_t> m2 = mo, s2 = so;
        if (b.table == 0) m2[b.at] = b.value;
        if (b.table == 1) s2[b.at] = b.value;
        uint8_t* out = (uint8_t*)malloc(160 * n + 1);
        kernel(mblob.data(), m2.data(), sblob.data(), s2.data(), kblob.data(), n, out, mbase, sbase, mblob.size(), sblob.size());
        for (size_t i = 0; i < n; ++i) {
            // lanes i = at - 1 and i = at read the bent entry
            const bool touched = b.table >= 0 && (i + 1 == b.at || i == b.at);
            const uint64_t* t = b.table == 0 ? m2.data() : s2.data();
            const uint64_t base = b.table == 0 ? mbase : sbase, size = b.table == 0 ? mblob.size() : sblob.size();
            bool emptied = false;
            if (touched) { const uint64_t a = t[i] - base, e = t[i + 1] - base; emptied = !(a <= e && e <= size); }
            if (touched && !emptied && (t[i] != (b.table == 0 ? mo : so)[i] || t[i + 1] != (b.table == 0 ? mo : so)[i + 1])) continue;   // a shifted but valid slice: not this test's subject
            std::vector<uint8_t> expect = want[i];
            if (emptied) {
                memset(expect.data(), 0, 64);
                memcpy(expect.data() + 64, empty_hash.data(), 32);
            }
            if (memcmp(out + 160 * i, expect.data(), 160)) { fprintf(stderr, "kernel model, %s: lane %zu differs\n", b.name, i); ++bad; }
        }
        free(out);
    }
    printf("%zu cases, %zu table forms, %zu mismatches\n", n, bends.size(), bad);
    return bad ? 1 : 0;
}
#endif
