// trim_emul.cc — CPU tier of the 32-bit canonical store and the shortened comb ends (tests/test_emul_trim.py).
//
// g++ build of the unit ops of tools/devunit_trim.hip (host backend, SBV_F29_CHECK on: every contract the code relies on is
// asserted and a breach aborts) plus the table builders that store through the 32-bit canonical form:
//   sbvt_key_table      a key's 33-window comb and its compact rows from the chain / rows / fill lane functions of p256_keytab29.h
//   sbvt_generic_qtab   the eight entries of the one-lane kernel's per-signature table (p256_comb29.h: verify29_generic_q)
//   sbvt_canon32_abort  f29_canon32 on limbs of the caller's choice (the contract assertion, run in a child process)
// Built twice by the test, the second time with -DSBV_F29_STORE_REF, which sends every table store through f29_canon: the two
// builds must produce the same bytes.
#include "../../tools/devunit_trim.hip"

#include <vector>

extern "C" {
// qx, qy: plain coordinates (8 words each), ANY pair — the arithmetic does not ask whether they are on the curve.
// table: 33 x 128 entries, crows: 33 x 16 entries, both zeroed first (the slots the builders leave alone stay zero).
void sbvt_key_table(const uint32_t* qx, const uint32_t* qy, uint32_t* table, uint32_t* crows) {
    apt* tab = reinterpret_cast<apt*>(table);
    apt* ctab = reinterpret_cast<apt*>(crows);
    memset(tab, 0, SBVT_COMB_ENTRIES * sizeof(apt));
    memset(ctab, 0, (size_t)SBV_NTAB_ENTRIES * sizeof(apt));
    fe29 x, y;
    f29_from_plain(x, ldw(qx));
    f29_from_plain(y, ldw(qy));
    keychain_quad_host q;
    for (int i = 0; i < 4; ++i) keychain29_start(q.s[i], x, y);
    std::vector<u32> bases((size_t)SBV_GTAB_WINDOWS * SBV_KT29_POINTS_PER_WINDOW * SBV_KT29_REC_WORDS, 0u);
    for (int j = 0; j < SBV_GTAB_WINDOWS; ++j)
        for (int d = 0; d < 8; ++d) {
            if (d == 0 || d == 4) kchain_store(&bases[((size_t)j * SBV_KT29_POINTS_PER_WINDOW + d) * SBV_KT29_REC_WORDS], q.s[0]);
            if (j == SBV_GTAB_WINDOWS - 1) break;
            keychain29_dbl(q);
        }
    std::vector<u32> tmp(SBV_KT29_ROWS_TMP_WORDS, 0u);
    for (int j = 0; j < SBV_GTAB_WINDOWS; ++j) {
        const bool top = j == SBV_GTAB_WINDOWS - 1;
        const u32* b2 = &bases[(size_t)j * SBV_KT29_POINTS_PER_WINDOW * SBV_KT29_REC_WORDS];
        apt* row = tab + (size_t)j * SBV_GTAB_PER_WINDOW;
        for (int which = 0; which < (top ? 1 : 2); ++which) keytab29_rows_lane(b2, which, top, tmp.data(), row, ctab + (size_t)j * SBV_NTAB_PER_WINDOW);
        if (!top)
            for (int a = 1; a <= 8; ++a) keytab29_fill_sym_lane(a, tmp.data(), row);
    }
}
// out: 8 x 16 words
void sbvt_generic_qtab(const uint32_t* u2, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
    std::vector<u32> qtab(SBV_QTAB29_WORDS, 0u);
    xyzz S;
    bool ok = true;
    verify29_generic_q(S, ok, ldw(u2), ldw(qx), ldw(qy), qtab.data());
    memcpy(out, qtab.data(), 8 * 16 * sizeof(u32));
}
void sbvt_canon32_abort(const int32_t* limbs) {
    fe29 a, z;
    for (int i = 0; i < 9; ++i) a.v[i] = limbs[i];
    f29_canon32(z, a);
}
}
