// devunit.hip — TEST ONLY: the device arithmetic, one primitive per kernel, one case per lane.
//
// Every field / scalar / point primitive the product's kernels execute, instantiated from the product's own headers
// (consensus_amd/csrc/*.h) by hipcc -O3 for gfx950 — the compiler and the code paths (clang's add-with-carry builtins, the
// opaque reduction constants, SBV_UNROLL, DPP quad broadcasts, __shfl_xor) that tests/emul, a g++ host build, never sees.
// tests/test_gpu_devunit.py feeds it the cases of tests/arith_cases.py and compares every output with Python big integers;
// tests/test_devunit_cpu.py does the same through backend 0 (the same run_op in a host loop, clang host code), so that the
// generators, the packing and the references are debugged without a GPU.  Backend 0 is a second system under test, never
// the reference.  Not linked into libsbv.so; nothing in the product calls it.
//
// Records are 32-bit words; signed limbs travel as their bit patterns.  sbvd_op_words() gives the record sizes, so the
// Python side packs blindly.  Cross-lane ops (quad chains through DPP, the __shfl_xor sum) exist on the device only.
//
// The same file also compiles as plain C++ (g++ -x c++ with the SBV_*_CHECK macros: tests/test_devunit_cpu.py builds that as
// tests/emul/libsbv_devunit_check.so): there every primitive asserts its operand contract and aborts on a breach, which is
// how the case generators are proved to stay inside the contracts.  That build has no device backend.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <string.h>

#include "../consensus_amd/csrc/p256_core.h"
#include "../consensus_amd/csrc/p256_pt29.h"
#include "../consensus_amd/csrc/p256_sc29.h"
#include "../consensus_amd/csrc/p256_keytab29.h"
#include "../consensus_amd/csrc/p256_sign.h"
#include "../consensus_amd/csrc/ed25519_core.h"
#include "../consensus_amd/csrc/ed25519_group.h"
#include "../consensus_amd/csrc/sha512_dev.h"
#include "../consensus_amd/csrc/k256_core.h"
#include "../consensus_amd/csrc/k256_group.h"

using namespace sbv;

// name, words in, words out.  Layouts: f = fe29 / kfe (9 limbs), w = 8 words, e = fe25 (10 limbs), xyzz = X Y ZZ ZZZ inf (37),
// jac = X Y Z (27), jacf / kjpt = X Y Z inf (28), ept / pniels = 40 limbs, flags and counts one word each.  The P-256 signer's
// helpers (sha256_msg, hmac_v, hmac_v_tag, sign29_finish: p256_sign.h and below) state their records next to their code.
#define SBVD_OPS(X) \
    X(f29_mul, 18, 9) X(f29_sqr, 9, 9) X(f29_mulx, 18, 9) X(f29_sqrx, 9, 9) X(f29_mul_sub_mul, 36, 9) X(f29_sqr_sub_val, 18, 9) \
    X(f29_canon, 9, 9) X(f29_norm, 9, 9) X(f29_norm_red, 9, 9) X(f29_is_zero, 9, 1) X(f29_maybe_zero, 9, 1) X(f29_pack, 9, 8) \
    X(f29_unpack, 8, 9) X(f29_from_fe, 8, 9) X(f29_to_fe, 9, 8) X(f29_from_plain, 8, 9) X(f29_inv, 9, 9) X(f29_inv_ct, 9, 9) \
    X(f29_mulchain, 19, 9) \
    X(s29_mul, 18, 9) X(s29_canon, 9, 9) X(s29_inv, 9, 9) X(s29_inv_ct, 9, 9) X(sc_mul, 16, 8) X(sc_inv, 8, 8) X(sc_inv_gcd, 8, 8) \
    X(fe_inv_gcd, 8, 8) X(modinv30, 9, 8) X(modinv30_ct, 9, 8) \
    X(sha256_msg, 257, 8) X(hmac_v, 16, 8) X(hmac_v_tag, 34, 8) X(sign29_finish, 32, 17) \
    X(pt29_dbl, 37, 37) X(pt29_madd, 56, 37) X(pt29_add, 74, 37) X(pt29_mdbl, 18, 37) X(pt29_mdbl_a, 27, 37) X(pt29_dbl_jac, 27, 27) \
    X(pt29_dbl_jacx, 28, 28) X(pt29_madd_jacx, 47, 28) X(apt29_add_with_inverse, 45, 18) X(pt29_rx_matches, 45, 1) \
    X(fe25_mul, 20, 10) X(fe25_sqr, 10, 10) X(fe25_carry, 10, 10) X(fe25_add, 20, 10) X(fe25_sub, 20, 10) X(fe25_neg, 10, 10) \
    X(fe25_freeze, 10, 8) X(fe25_from_words, 8, 10) X(fe25_inv, 10, 10) X(fe25_inv_gcd, 10, 10) X(fe25_pow22523, 10, 10) \
    X(fe25_is_negative, 10, 1) X(ed_dbl, 40, 40) X(ed_add_pniels, 82, 40) X(ed_add_aniels, 72, 40) X(ed_decompress, 8, 41) \
    X(ed_encoding_matches, 48, 1) X(mod_l_512, 16, 8) X(sha512_ram, 273, 16) \
    X(kfe_mul, 18, 9) X(kfe_sqr, 9, 9) X(kfe_add, 18, 9) X(kfe_sub, 18, 9) X(kfe_lin, 20, 9) X(kfe_lin3, 29, 9) X(kfe_cneg, 10, 9) \
    X(kfe_inv, 9, 9) X(kfe_is_zero, 9, 1) X(kfe_maybe_zero, 9, 1) X(kfe_equal, 18, 1) X(kfe_to_words, 9, 8) X(kfe_from_words, 8, 9) \
    X(ksc_mul, 16, 8) X(ksc_inv, 8, 8) X(ksc_reduce512, 16, 8) X(ksc_split_lambda, 8, 18) X(kpt_dbl, 28, 28) X(kpt_madd, 48, 28) \
    X(k256_on_curve, 18, 1)
// device only: every lane of a quad (of a 2^k-lane group for x_shfl_sum) gets the same record apart from its own point
#define SBVD_XOPS(X) X(x_keychain29, 19, 36) X(x_edchain, 41, 40) X(x_k256chain, 19, 27) X(x_shfl_sum, 38, 37)

#define SBVD_ENUM(name, in_w, out_w) OP_##name,
enum { SBVD_OPS(SBVD_ENUM) SBVD_XOPS(SBVD_ENUM) OP_COUNT };
enum { OP_PLAIN_COUNT = OP_x_keychain29 };      // the first cross-lane op
#define SBVD_INFO(name, in_w, out_w) {#name, in_w, out_w},
struct op_info { const char* name; int in_w, out_w; };
static const op_info g_ops[] = {SBVD_OPS(SBVD_INFO) SBVD_XOPS(SBVD_INFO)};

#define SBVD_MAX_CASES ((size_t)1 << 20)
#define SBVD_MAX_CHAIN 256          // doublings of a quad chain (the product's chains run 8 per window, 256 per key)
#define SBVD_SHA_MAX_MSG 1024

// ---- record access -------------------------------------------------------------------------------------------------------
SBV_HD fe29 ld29(const u32* p) { fe29 r; for (int i = 0; i < 9; ++i) r.v[i] = (i32)p[i]; return r; }
SBV_HD void st29(u32* p, const fe29& a) { for (int i = 0; i < 9; ++i) p[i] = (u32)a.v[i]; }
SBV_HD kfe ldk(const u32* p) { kfe r; for (int i = 0; i < 9; ++i) r.v[i] = (i32)p[i]; return r; }
SBV_HD void stk(u32* p, const kfe& a) { for (int i = 0; i < 9; ++i) p[i] = (u32)a.v[i]; }
SBV_HD fe25 ld25(const u32* p) { fe25 r; for (int i = 0; i < 10; ++i) r.v[i] = (i32)p[i]; return r; }
SBV_HD void st25(u32* p, const fe25& a) { for (int i = 0; i < 10; ++i) p[i] = (u32)a.v[i]; }
SBV_HD u256 ldw(const u32* p) { u256 r; for (int i = 0; i < 8; ++i) r.v[i] = p[i]; return r; }
SBV_HD void stw(u32* p, const u256& a) { for (int i = 0; i < 8; ++i) p[i] = a.v[i]; }
SBV_HD xyzz ldxyzz(const u32* p) { xyzz R; R.X = ld29(p); R.Y = ld29(p + 9); R.ZZ = ld29(p + 18); R.ZZZ = ld29(p + 27); R.inf = p[36] != 0; return R; }
SBV_HD void stxyzz(u32* p, const xyzz& R) { st29(p, R.X); st29(p + 9, R.Y); st29(p + 18, R.ZZ); st29(p + 27, R.ZZZ); p[36] = R.inf ? 1u : 0u; }
SBV_HD ept ldept(const u32* p) { ept R; R.X = ld25(p); R.Y = ld25(p + 10); R.Z = ld25(p + 20); R.T = ld25(p + 30); return R; }
SBV_HD void stept(u32* p, const ept& R) { st25(p, R.X); st25(p + 10, R.Y); st25(p + 20, R.Z); st25(p + 30, R.T); }
SBV_HD kjpt ldkj(const u32* p) { kjpt R; R.X = ldk(p); R.Y = ldk(p + 9); R.Z = ldk(p + 18); R.inf = p[27] != 0; return R; }
SBV_HD void stkj(u32* p, const kjpt& R) { stk(p, R.X); stk(p + 9, R.Y); stk(p + 18, R.Z); p[27] = R.inf ? 1u : 0u; }
SBV_HD modinfo30 modinfo_of(u32 which) {
    return which == 0 ? modinfo30_p256() : which == 1 ? modinfo30_p256_order() : which == 2 ? modinfo30_25519()
         : which == 3 ? modinfo30_k256_p() : modinfo30_k256_n();
}

// ---- one case of one op ----------------------------------------------------------------------------------------------------
template <int OP>
SBV_HD void run_op(const u32* in, u32* out) {
    if constexpr (OP == OP_f29_mul) { fe29 z; f29_mul(z, ld29(in), ld29(in + 9)); st29(out, z); }
    else if constexpr (OP == OP_f29_sqr) { fe29 z; f29_sqr(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_mulx) { fe29 z; f29_mulx(z, ld29(in), ld29(in + 9)); st29(out, z); }
    else if constexpr (OP == OP_f29_sqrx) { fe29 z; f29_sqrx(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_mul_sub_mul) {              // a b - c d as the mixed addition forms Y3: one reduction, f29_red_q
        fe29 nc, z;
        f29_neg(nc, ld29(in + 18));
        f29_cols t; f29_cols_zero(t); f29_cols_mul(t, ld29(in), ld29(in + 9)); f29_cols_mul(t, nc, ld29(in + 27));
        f29_reduce_x(z, t); f29_red_q(z); st29(out, z);
    }
    else if constexpr (OP == OP_f29_sqr_sub_val) {              // a^2 - v R as the mixed addition forms X3
        fe29 z;
        f29_cols t; f29_cols_zero(t); f29_cols_sqr(t, ld29(in)); f29_cols_sub_val(t, ld29(in + 9));
        f29_reduce_x(z, t); f29_red_q(z); st29(out, z);
    }
    else if constexpr (OP == OP_f29_canon) { fe29 z; f29_canon(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_norm) { fe29 z; f29_norm(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_norm_red) { fe29 z; f29_norm_red(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_is_zero) { out[0] = f29_is_zero(ld29(in)) ? 1u : 0u; }
    else if constexpr (OP == OP_f29_maybe_zero) { out[0] = f29_maybe_zero(ld29(in)) ? 1u : 0u; }
    else if constexpr (OP == OP_f29_pack) { u256 w; f29_pack(w.v, ld29(in)); stw(out, w); }
    else if constexpr (OP == OP_f29_unpack) { fe29 z; const u256 w = ldw(in); f29_unpack(z, w.v); st29(out, z); }
    else if constexpr (OP == OP_f29_from_fe) { fe29 z; f29_from_fe(z, ldw(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_to_fe) { fe w; f29_to_fe(w, ld29(in)); stw(out, w); }
    else if constexpr (OP == OP_f29_from_plain) { fe29 z; f29_from_plain(z, ldw(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_inv) { fe29 z; f29_inv(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_inv_ct) { fe29 z; f29_inv_ct(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_f29_mulchain) {                 // x = a; n <= 8 times x = x b / R: values stay loose from product to product
        fe29 x = ld29(in);
        const fe29 b = ld29(in + 9);
        const u32 n = in[18];
        SBV_NOUNROLL
        for (u32 k = 0; k < 8; ++k) if (k < n) f29_mul(x, x, b);
        st29(out, x);
    }
    else if constexpr (OP == OP_s29_mul) { fe29 z; s29_mul(z, ld29(in), ld29(in + 9)); st29(out, z); }
    else if constexpr (OP == OP_s29_canon) { fe29 z; s29_canon(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_s29_inv) { fe29 z; s29_inv(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_s29_inv_ct) { fe29 z; s29_inv_ct(z, ld29(in)); st29(out, z); }
    else if constexpr (OP == OP_sc_mul) { sc z; sc_mul(z, ldw(in), ldw(in + 8)); stw(out, z); }
    else if constexpr (OP == OP_sc_inv) { sc z; sc_inv(z, ldw(in)); stw(out, z); }
    else if constexpr (OP == OP_sc_inv_gcd) { sc z; sc_inv_gcd(z, ldw(in)); stw(out, z); }
    else if constexpr (OP == OP_fe_inv_gcd) { fe z; fe_inv_gcd(z, ldw(in)); stw(out, z); }
    else if constexpr (OP == OP_modinv30) { u256 z; modinv30(z, ldw(in + 1), modinfo_of(in[0])); stw(out, z); }
    else if constexpr (OP == OP_modinv30_ct) { u256 z; modinv30_ct(z, ldw(in + 1), modinfo_of(in[0])); stw(out, z); }
    else if constexpr (OP == OP_sha256_msg) {                   // in: length | message (SBVD_SHA_MAX_MSG bytes, little-endian words); out: the digest's big-endian words
        const size_t mlen = in[0] <= SBVD_SHA_MAX_MSG ? in[0] : SBVD_SHA_MAX_MSG;
        sha256_msg(reinterpret_cast<const uint8_t*>(in + 1), mlen, out);
    }
    else if constexpr (OP == OP_hmac_v) {                       // in: K | V (big-endian words); out: HMAC(K, V)
        hmac_key hk;
        hmac_set_key(hk, in);
        hmac_v(hk, in + 8, out);
    }
    else if constexpr (OP == OP_hmac_v_tag) {                   // in: K | V | tag | x | h | tail_only; out: HMAC(K, V || tag [|| x || h])
        hmac_key hk;
        hmac_set_key(hk, in);
        hmac_v_tag(hk, in + 8, in[16], in + 17, in + 25, in[33] != 0, out);
    }
    else if constexpr (OP == OP_sign29_finish) {                // in: x | d | k | e (plain integers); out: r | s | ok, all zero when not ok
        u256 r, s;
        const bool ok = sign29_finish(ldw(in), ldw(in + 8), ldw(in + 16), ldw(in + 24), r, s);
        for (int i = 0; i < 8; ++i) { out[i] = ok ? r.v[i] : 0u; out[8 + i] = ok ? s.v[i] : 0u; }
        out[16] = ok ? 1u : 0u;
    }
    else if constexpr (OP == OP_pt29_dbl) { xyzz R = ldxyzz(in); pt29_dbl(R); stxyzz(out, R); }
    else if constexpr (OP == OP_pt29_madd) { xyzz R = ldxyzz(in); apt29 q; q.x = ld29(in + 37); q.y = ld29(in + 46); pt29_madd(R, q, in[55] != 0); stxyzz(out, R); }
    else if constexpr (OP == OP_pt29_add) { xyzz R = ldxyzz(in); const xyzz Q = ldxyzz(in + 37); pt29_add(R, Q); stxyzz(out, R); }
    else if constexpr (OP == OP_pt29_mdbl) { xyzz R; pt29_mdbl(R, ld29(in), ld29(in + 9)); stxyzz(out, R); }
    else if constexpr (OP == OP_pt29_mdbl_a) { xyzz R; pt29_mdbl_a(R, ld29(in), ld29(in + 9), ld29(in + 18)); stxyzz(out, R); }
    else if constexpr (OP == OP_pt29_dbl_jac) { jpt29 R; R.X = ld29(in); R.Y = ld29(in + 9); R.Z = ld29(in + 18); pt29_dbl_jac(R); st29(out, R.X); st29(out + 9, R.Y); st29(out + 18, R.Z); }
    else if constexpr (OP == OP_pt29_dbl_jacx) {
        jpt29f R; R.X = ld29(in); R.Y = ld29(in + 9); R.Z = ld29(in + 18); R.inf = in[27] != 0;
        pt29_dbl_jacx(R);
        st29(out, R.X); st29(out + 9, R.Y); st29(out + 18, R.Z); out[27] = R.inf ? 1u : 0u;
    }
    else if constexpr (OP == OP_pt29_madd_jacx) {
        jpt29f R; R.X = ld29(in); R.Y = ld29(in + 9); R.Z = ld29(in + 18); R.inf = in[27] != 0;
        apt29 q; q.x = ld29(in + 28); q.y = ld29(in + 37);
        pt29_madd_jacx(R, q, in[46] != 0);
        st29(out, R.X); st29(out + 9, R.Y); st29(out + 18, R.Z); out[27] = R.inf ? 1u : 0u;
    }
    else if constexpr (OP == OP_apt29_add_with_inverse) {
        apt29 a, b, r; a.x = ld29(in); a.y = ld29(in + 9); b.x = ld29(in + 18); b.y = ld29(in + 27);
        apt29_add_with_inverse(r, a, b, ld29(in + 36));
        st29(out, r.x); st29(out + 9, r.y);
    }
    else if constexpr (OP == OP_pt29_rx_matches) { const xyzz R = ldxyzz(in); out[0] = pt29_rx_matches(R, ldw(in + 37)) ? 1u : 0u; }
    else if constexpr (OP == OP_fe25_mul) { fe25 z; fe25_mul(z, ld25(in), ld25(in + 10)); st25(out, z); }
    else if constexpr (OP == OP_fe25_sqr) { fe25 z; fe25_sqr(z, ld25(in)); st25(out, z); }
    else if constexpr (OP == OP_fe25_carry) { fe25 z; fe25_carry(z, ld25(in)); st25(out, z); }
    else if constexpr (OP == OP_fe25_add) { fe25 z; fe25_add(z, ld25(in), ld25(in + 10)); st25(out, z); }
    else if constexpr (OP == OP_fe25_sub) { fe25 z; fe25_sub(z, ld25(in), ld25(in + 10)); st25(out, z); }
    else if constexpr (OP == OP_fe25_neg) { fe25 z; fe25_neg(z, ld25(in)); st25(out, z); }
    else if constexpr (OP == OP_fe25_freeze) { u256 w; fe25_freeze(w, ld25(in)); stw(out, w); }
    else if constexpr (OP == OP_fe25_from_words) { fe25 z; const u256 w = ldw(in); fe25_from_words(z, w.v); st25(out, z); }
    else if constexpr (OP == OP_fe25_inv) { fe25 z; fe25_inv(z, ld25(in)); st25(out, z); }
    else if constexpr (OP == OP_fe25_inv_gcd) { fe25 z; fe25_inv_gcd(z, ld25(in)); st25(out, z); }
    else if constexpr (OP == OP_fe25_pow22523) { fe25 z; fe25_pow22523(z, ld25(in)); st25(out, z); }
    else if constexpr (OP == OP_fe25_is_negative) { out[0] = fe25_is_negative(ld25(in)) ? 1u : 0u; }
    else if constexpr (OP == OP_ed_dbl) { ept r; ed_dbl(r, ldept(in)); stept(out, r); }
    else if constexpr (OP == OP_ed_add_pniels) {
        ept R = ldept(in);
        pniels q; q.YpX = ld25(in + 40); q.YmX = ld25(in + 50); q.Z = ld25(in + 60); q.T2d = ld25(in + 70);
        ed_add_pniels(R, q, in[80] != 0, in[81] != 0);
        stept(out, R);
    }
    else if constexpr (OP == OP_ed_add_aniels) {
        ept R = ldept(in);
        aniels_r q; q.ypx = ld25(in + 40); q.ymx = ld25(in + 50); q.xy2d = ld25(in + 60);
        ed_add_aniels(R, q, in[70] != 0, in[71] != 0);
        stept(out, R);
    }
    else if constexpr (OP == OP_ed_decompress) { ept A; const u256 w = ldw(in); out[0] = ed_decompress(A, w.v) ? 1u : 0u; stept(out + 1, A); }
    else if constexpr (OP == OP_ed_encoding_matches) { const u256 w = ldw(in + 40); out[0] = ed_encoding_matches(ldept(in), w.v) ? 1u : 0u; }
    else if constexpr (OP == OP_mod_l_512) { u32 x[16], r[8]; for (int i = 0; i < 16; ++i) x[i] = in[i]; mod_l_512(x, r); for (int i = 0; i < 8; ++i) out[i] = r[i]; }
    else if constexpr (OP == OP_sha512_ram) {                   // in: length | R | A (64 bytes) | message (SBVD_SHA_MAX_MSG bytes, little-endian words)
        const size_t mlen = in[0] <= SBVD_SHA_MAX_MSG ? in[0] : SBVD_SHA_MAX_MSG;
        const uint8_t* b = reinterpret_cast<const uint8_t*>(in + 1);
        u64 st[8];
        sha512_ram(b, b + 32, b + 64, mlen, st);
        for (int i = 0; i < 8; ++i) { out[2 * i] = (u32)st[i]; out[2 * i + 1] = (u32)(st[i] >> 32); }
    }
    else if constexpr (OP == OP_kfe_mul) { kfe z; kfe_mul(z, ldk(in), ldk(in + 9)); stk(out, z); }
    else if constexpr (OP == OP_kfe_sqr) { kfe z; kfe_sqr(z, ldk(in)); stk(out, z); }
    else if constexpr (OP == OP_kfe_add) { kfe z; kfe_add(z, ldk(in), ldk(in + 9)); stk(out, z); }
    else if constexpr (OP == OP_kfe_sub) { kfe z; kfe_sub(z, ldk(in), ldk(in + 9)); stk(out, z); }
    else if constexpr (OP == OP_kfe_lin) { kfe z; kfe_lin(z, ldk(in), (int)in[18], ldk(in + 9), (int)in[19]); stk(out, z); }
    else if constexpr (OP == OP_kfe_lin3) { kfe z; kfe_lin3(z, ldk(in), ldk(in + 9), (int)in[27], ldk(in + 18), (int)in[28]); stk(out, z); }
    else if constexpr (OP == OP_kfe_cneg) { kfe z; kfe_cneg(z, ldk(in), in[9] != 0); stk(out, z); }
    else if constexpr (OP == OP_kfe_inv) { kfe z; kfe_inv(z, ldk(in)); stk(out, z); }
    else if constexpr (OP == OP_kfe_is_zero) { out[0] = kfe_is_zero(ldk(in)) ? 1u : 0u; }
    else if constexpr (OP == OP_kfe_maybe_zero) { out[0] = kfe_maybe_zero(ldk(in)) ? 1u : 0u; }
    else if constexpr (OP == OP_kfe_equal) { out[0] = kfe_equal(ldk(in), ldk(in + 9)) ? 1u : 0u; }
    else if constexpr (OP == OP_kfe_to_words) { u256 w; kfe_to_words(w, ldk(in)); stw(out, w); }
    else if constexpr (OP == OP_kfe_from_words) { kfe z; kfe_from_words(z, ldw(in)); stk(out, z); }
    else if constexpr (OP == OP_ksc_mul) { u256 z; ksc_mul(z, ldw(in), ldw(in + 8)); stw(out, z); }
    else if constexpr (OP == OP_ksc_inv) { u256 z; ksc_inv(z, ldw(in)); stw(out, z); }
    else if constexpr (OP == OP_ksc_reduce512) { u32 x[16]; for (int i = 0; i < 16; ++i) x[i] = in[i]; u256 z; ksc_reduce512(z, x); stw(out, z); }
    else if constexpr (OP == OP_ksc_split_lambda) {
        u256 k1, k2; bool n1, n2;
        ksc_split_lambda(k1, n1, k2, n2, ldw(in));
        stw(out, k1); stw(out + 8, k2); out[16] = n1 ? 1u : 0u; out[17] = n2 ? 1u : 0u;
    }
    else if constexpr (OP == OP_kpt_dbl) { kjpt r; kpt_dbl(r, ldkj(in)); stkj(out, r); }
    else if constexpr (OP == OP_kpt_madd) { kjpt r; kpt_madd(r, ldkj(in), ldk(in + 28), ldk(in + 37), in[46] != 0, in[47] != 0); stkj(out, r); }
    else if constexpr (OP == OP_k256_on_curve) { out[0] = k256_on_curve(ldk(in), ldk(in + 9)) ? 1u : 0u; }
}

#if defined(__HIPCC__)
// ---- cross-lane ops: the product's exchange policies, one record per lane ----------------------------------------------------
template <int OP>
__device__ __forceinline__ void run_xop(const u32* in, u32* out, u32 lane) {
    if constexpr (OP == OP_x_keychain29) {                      // in: x | y (affine, tight) | doublings; out: X Y Z T of this lane
        keychain_quad_dev q;
        q.r = (int)(lane & 3u);
        keychain29_start(q.s[0], ld29(in), ld29(in + 9));
        const u32 n = in[18] <= SBVD_MAX_CHAIN ? in[18] : SBVD_MAX_CHAIN;       // the same in all four lanes of a quad
        SBV_NOUNROLL
        for (u32 d = 0; d < SBVD_MAX_CHAIN; ++d) {
            if (d >= n) break;
            keychain29_dbl(q);
        }
        st29(out, q.s[0].X); st29(out + 9, q.s[0].Y); st29(out + 18, q.s[0].Z); st29(out + 27, q.s[0].T);
    }
    else if constexpr (OP == OP_x_edchain) {                    // in: X Y Z T (tight) | doublings
        edchain_quad_dev q;
        q.r = (int)(lane & 3u);
        q.s[0] = ldept(in);
        const u32 n = in[40] <= SBVD_MAX_CHAIN ? in[40] : SBVD_MAX_CHAIN;
        SBV_NOUNROLL
        for (u32 d = 0; d < SBVD_MAX_CHAIN; ++d) {
            if (d >= n) break;
            edchain_dbl(q);
        }
        stept(out, q.s[0]);
    }
    else if constexpr (OP == OP_x_k256chain) {                  // in: x | y (affine, reduced) | doublings
        k256_quad_dev q;
        q.r = (int)(lane & 3u);
        q.s[0].X = ldk(in); q.s[0].Y = ldk(in + 9); q.s[0].Z = kfe_one();
        const u32 n = in[18] <= SBVD_MAX_CHAIN ? in[18] : SBVD_MAX_CHAIN;
        SBV_NOUNROLL
        for (u32 d = 0; d < SBVD_MAX_CHAIN; ++d) {
            if (d >= n) break;
            k256_chain_dbl(q);
        }
        stk(out, q.s[0].X); stk(out + 9, q.s[0].Y); stk(out + 18, q.s[0].Z);
    }
    else if constexpr (OP == OP_x_shfl_sum) {                   // in: xyzz | group size 2^k <= 16 (the same in every lane of the launch)
        xyzz R = ldxyzz(in);
        const int lanes = (int)in[37];
        // the butterfly of k_p256_verify_keyed_coop / k_p256_verify_prepared_small (p256_kernels.hip)
        SBV_NOUNROLL
        for (int off = 8; off >= 1; off >>= 1) {
            if (off >= lanes) continue;
            xyzz P;
            SBV_UNROLL
            for (int l = 0; l < 9; ++l) {
                P.X.v[l] = __shfl_xor(R.X.v[l], off, 64);
                P.Y.v[l] = __shfl_xor(R.Y.v[l], off, 64);
                P.ZZ.v[l] = __shfl_xor(R.ZZ.v[l], off, 64);
                P.ZZZ.v[l] = __shfl_xor(R.ZZZ.v[l], off, 64);
            }
            P.inf = __shfl_xor(R.inf ? 1 : 0, off, 64) != 0;
            pt29_add(R, P);
        }
        stxyzz(out, R);
    }
}

// case i -> lane i, 64-lane workgroups like the product's table kernels
template <int OP>
__global__ __launch_bounds__(64) void k_devunit(const u32* __restrict__ in, u32* __restrict__ out, u32 n, int in_w, int out_w) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    run_op<OP>(in + (size_t)i * in_w, out + (size_t)i * out_w);
}
// cross-lane: n is a multiple of 64, every lane of every wavefront is active
template <int OP>
__global__ __launch_bounds__(64) void k_devunit_x(const u32* __restrict__ in, u32* __restrict__ out, u32 n, int in_w, int out_w) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    run_xop<OP>(in + (size_t)i * in_w, out + (size_t)i * out_w, i);
}
#endif

#define SBVD_ERR_BAD_OP (-1000)
#define SBVD_ERR_BAD_ARG (-1001)
#define SBVD_ERR_NOT_AVAILABLE (-1002)          // a cross-lane op on the host backend

#if defined(__HIPCC__)
static int hip_fail(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }

static int run_device(int op, const u32* in, u32* out, size_t n) {
    const op_info& oi = g_ops[op];
    const size_t in_b = n * (size_t)oi.in_w * 4, out_b = n * (size_t)oi.out_w * 4;
    u32 *din = nullptr, *dout = nullptr;
    int rc = hip_fail(hipMalloc(&din, in_b));
    if (rc) return rc;
    rc = hip_fail(hipMalloc(&dout, out_b));
    if (rc) { (void)hipFree(din); return rc; }
    rc = hip_fail(hipMemcpy(din, in, in_b, hipMemcpyHostToDevice));
    if (!rc) rc = hip_fail(hipMemset(dout, 0xA5, out_b));
    if (!rc) {
        const dim3 grid((unsigned)((n + 63) / 64)), block(64);
        switch (op) {
#define SBVD_LAUNCH(name, in_w, out_w) case OP_##name: hipLaunchKernelGGL(k_devunit<OP_##name>, grid, block, 0, 0, din, dout, (u32)n, in_w, out_w); break;
            SBVD_OPS(SBVD_LAUNCH)
#define SBVD_LAUNCH_X(name, in_w, out_w) case OP_##name: hipLaunchKernelGGL(k_devunit_x<OP_##name>, grid, block, 0, 0, din, dout, (u32)n, in_w, out_w); break;
            SBVD_XOPS(SBVD_LAUNCH_X)
        }
        rc = hip_fail(hipGetLastError());
        if (!rc) rc = hip_fail(hipDeviceSynchronize());
    }
    if (!rc) rc = hip_fail(hipMemcpy(out, dout, out_b, hipMemcpyDeviceToHost));
    (void)hipFree(din);
    (void)hipFree(dout);
    return rc;
}

#else
static int run_device(int, const u32*, u32*, size_t) { return SBVD_ERR_NOT_AVAILABLE; }
#endif

static int run_host(int op, const u32* in, u32* out, size_t n) {
    switch (op) {
#define SBVD_HOST(name, in_w, out_w) case OP_##name: for (size_t i = 0; i < n; ++i) run_op<OP_##name>(in + i * in_w, out + i * out_w); return 0;
        SBVD_OPS(SBVD_HOST)
    }
    return SBVD_ERR_NOT_AVAILABLE;
}

extern "C" {
int sbvd_op_count() { return OP_COUNT; }
const char* sbvd_op_name(int op) { return op >= 0 && op < OP_COUNT ? g_ops[op].name : nullptr; }
int sbvd_op_is_cross_lane(int op) { return op >= OP_PLAIN_COUNT && op < OP_COUNT ? 1 : 0; }
int sbvd_op_words(int op, uint32_t* in_words, uint32_t* out_words) {
    if (op < 0 || op >= OP_COUNT) return SBVD_ERR_BAD_OP;
    *in_words = (uint32_t)g_ops[op].in_w;
    *out_words = (uint32_t)g_ops[op].out_w;
    return 0;
}
// backend 1: one launch of the op's kernel on the current device; backend 0: the same run_op in a host loop.
// 0 = ok, -(hipError_t) for a HIP error, SBVD_ERR_* otherwise.
int sbvd_run(int backend, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (op < 0 || op >= OP_COUNT) return SBVD_ERR_BAD_OP;
    if ((backend != 0 && backend != 1) || n == 0 || n > SBVD_MAX_CASES || !in || !out) return SBVD_ERR_BAD_ARG;
    const bool cross = sbvd_op_is_cross_lane(op) != 0;
    if (cross && (backend == 0 || (n & 63) != 0)) return backend == 0 ? SBVD_ERR_NOT_AVAILABLE : SBVD_ERR_BAD_ARG;
    return backend == 1 ? run_device(op, in, out, n) : run_host(op, in, out, n);
}
}
