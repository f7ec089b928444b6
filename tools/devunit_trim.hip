// devunit_trim.hip — TEST ONLY: the 32-bit canonical store and the two shortened ends of a comb walk, one case per lane.
//
// A second unit library beside tools/devunit.hip (whose op inventory is pinned to tests/arith_cases.py): the same interface
// (sbvd_op_count / sbvd_op_name / sbvd_op_words / sbvd_run, backend 1 = one launch on the current device, backend 0 = the same
// code in a host loop), so tests/arith_cases.py loads and drives it unchanged.  tests/trim_cases.py holds the generators and the
// big-integer references, tests/test_gpu_trim.py runs them on the device, tests/test_emul_trim.py on a g++ build with the
// SBV_F29_CHECK assertions on (tests/emul/trim_emul.cc includes this file).  Not linked into libsbv.so.
//
// Every op that has a longer twin in the product returns BOTH results, so that a test compares the short form with the long one
// on the same lane as well as with Python big integers:
//   canon32   in: limbs (9)                                   out: f29_canon32 (9) | f29_canon (9)
//   mmadd     in: x1 (9) | y1 (9) | q (18) | neg (1)          out: pt29_mmadd (37) | pt29_madd on (x1, y1, 1, 1) (37)
//   madd_x    in: xyzz (37) | q (18) | neg (1)                out: pt29_madd_x (37) | pt29_madd (37)
//   walk_g    in: u (8) | x_only (1)                          out: gphase29_point from infinity over comb 0 (37)
//   walk_q    in: u2 (8) | x_only (1) | j0 (1) | xyzz (37)    out: qphase29_point, windows [j0, 33), over comb 1, added to xyzz (37)
// Combs: two 8-bit combs (33 windows x 128 canonical entries of the R = 2^261 domain, the layout of a key's table), uploaded
// once by sbvt_set_comb(): comb 0 is walked as a comb of G (gcomb), comb 1 as a key's table.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdlib.h>
#include <string.h>

#include "../consensus_amd/csrc/p256_core.h"
#include "../consensus_amd/csrc/p256_pt29.h"
#include "../consensus_amd/csrc/p256_comb29.h"
#include "../consensus_amd/csrc/p256_keytab29.h"

using namespace sbv;

#define SBVT_OPS(X) X(canon32, 9, 18) X(mmadd, 37, 74) X(madd_x, 56, 74) X(walk_g, 9, 37) X(walk_q, 47, 37)
#define SBVT_ENUM(name, in_w, out_w) OP_##name,
enum { SBVT_OPS(SBVT_ENUM) OP_COUNT };
#define SBVT_INFO(name, in_w, out_w) {#name, in_w, out_w},
struct op_info { const char* name; int in_w, out_w; };
static const op_info g_ops[] = {SBVT_OPS(SBVT_INFO)};

#define SBVT_MAX_CASES ((size_t)1 << 20)
#define SBVT_COMB_ENTRIES ((size_t)SBV_GTAB_WINDOWS * SBV_GTAB_PER_WINDOW)
struct combs { const apt* tab[2]; };

SBV_HD fe29 ld29(const u32* p) { fe29 r; for (int i = 0; i < 9; ++i) r.v[i] = (i32)p[i]; return r; }
SBV_HD void st29(u32* p, const fe29& a) { for (int i = 0; i < 9; ++i) p[i] = (u32)a.v[i]; }
SBV_HD u256 ldw(const u32* p) { u256 r; for (int i = 0; i < 8; ++i) r.v[i] = p[i]; return r; }
SBV_HD xyzz ldxyzz(const u32* p) { xyzz R; R.X = ld29(p); R.Y = ld29(p + 9); R.ZZ = ld29(p + 18); R.ZZZ = ld29(p + 27); R.inf = p[36] != 0; return R; }
SBV_HD void stxyzz(u32* p, const xyzz& R) { st29(p, R.X); st29(p + 9, R.Y); st29(p + 18, R.ZZ); st29(p + 27, R.ZZZ); p[36] = R.inf ? 1u : 0u; }
SBV_HD apt29 ldapt(const u32* p) { apt29 q; q.x = ld29(p); q.y = ld29(p + 9); return q; }

template <int OP>
SBV_HD void run_op(const u32* in, u32* out, const combs& cb) {
    if constexpr (OP == OP_canon32) {
        fe29 z;
        f29_canon32(z, ld29(in)); st29(out, z);
        f29_canon(z, ld29(in)); st29(out + 9, z);
    }
    else if constexpr (OP == OP_mmadd) {
        const apt29 q = ldapt(in + 18);
        xyzz R;
        pt29_set_inf(R);
        pt29_mmadd(R, ld29(in), ld29(in + 9), q, in[36] != 0);
        stxyzz(out, R);
        R.X = ld29(in); R.Y = ld29(in + 9); R.ZZ = f29_one(); R.ZZZ = f29_one(); R.inf = false;
        pt29_madd(R, q, in[36] != 0);
        stxyzz(out + 37, R);
    }
    else if constexpr (OP == OP_madd_x) {
        const apt29 q = ldapt(in + 37);
        xyzz R = ldxyzz(in);
        pt29_madd_x(R, q, in[55] != 0);
        stxyzz(out, R);
        R = ldxyzz(in);
        pt29_madd(R, q, in[55] != 0);
        stxyzz(out + 37, R);
    }
    else if constexpr (OP == OP_walk_g) {
        const gcomb gc = {cb.tab[0], 8, SBV_GTAB_WINDOWS};
        xyzz R;
        gphase29_point(R, ldw(in), gc, false, false, 0, -1, false, in[8] != 0);
        stxyzz(out, R);
    }
    else if constexpr (OP == OP_walk_q) {
        xyzz R = ldxyzz(in + 10);
        const int j0 = in[9] < (u32)SBV_GTAB_WINDOWS ? (int)in[9] : 0;
        qphase29_point(R, ldw(in), cb.tab[1], j0, SBV_GTAB_WINDOWS, in[8] != 0);
        stxyzz(out, R);
    }
}

static apt* g_host_comb[2] = {nullptr, nullptr};

#define SBVD_ERR_BAD_OP (-1000)
#define SBVD_ERR_BAD_ARG (-1001)
#define SBVD_ERR_NOT_AVAILABLE (-1002)

#if defined(__HIPCC__)
static apt* g_dev_comb[2] = {nullptr, nullptr};
// case i -> lane i, 64-lane workgroups
template <int OP>
__global__ __launch_bounds__(64) void k_devunit_trim(const u32* __restrict__ in, u32* __restrict__ out, u32 n, int in_w, int out_w, combs cb) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    run_op<OP>(in + (size_t)i * in_w, out + (size_t)i * out_w, cb);
}
static int hip_fail(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }
static int run_device(int op, const u32* in, u32* out, size_t n) {
    const op_info& oi = g_ops[op];
    if ((op == OP_walk_g && !g_dev_comb[0]) || (op == OP_walk_q && !g_dev_comb[1])) return SBVD_ERR_BAD_ARG;
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
        const combs cb = {{g_dev_comb[0], g_dev_comb[1]}};
        switch (op) {
#define SBVT_LAUNCH(name, in_w, out_w) case OP_##name: hipLaunchKernelGGL(k_devunit_trim<OP_##name>, grid, block, 0, 0, din, dout, (u32)n, in_w, out_w, cb); break;
            SBVT_OPS(SBVT_LAUNCH)
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
    if ((op == OP_walk_g && !g_host_comb[0]) || (op == OP_walk_q && !g_host_comb[1])) return SBVD_ERR_BAD_ARG;
    const combs cb = {{g_host_comb[0], g_host_comb[1]}};
    switch (op) {
#define SBVT_HOST(name, in_w, out_w) case OP_##name: for (size_t i = 0; i < n; ++i) run_op<OP_##name>(in + i * in_w, out + i * out_w, cb); return 0;
        SBVT_OPS(SBVT_HOST)
    }
    return SBVD_ERR_BAD_OP;
}

extern "C" {
int sbvd_op_count() { return OP_COUNT; }
const char* sbvd_op_name(int op) { return op >= 0 && op < OP_COUNT ? g_ops[op].name : nullptr; }
int sbvd_op_is_cross_lane(int) { return 0; }
int sbvd_op_words(int op, uint32_t* in_words, uint32_t* out_words) {
    if (op < 0 || op >= OP_COUNT) return SBVD_ERR_BAD_OP;
    *in_words = (uint32_t)g_ops[op].in_w;
    *out_words = (uint32_t)g_ops[op].out_w;
    return 0;
}
// comb `which` (0: walked as a comb of G, 1: as a key's table) = 33 x 128 entries of 16 words.  device != 0: a copy on the current
// device as well (backend 1).  0 = ok, -(hipError_t) for a HIP error.
int sbvt_set_comb(int which, const uint32_t* entries, int device) {
    if ((which != 0 && which != 1) || !entries) return SBVD_ERR_BAD_ARG;
    const size_t bytes = SBVT_COMB_ENTRIES * sizeof(apt);
    if (!g_host_comb[which]) g_host_comb[which] = static_cast<apt*>(aligned_alloc(64, bytes));
    if (!g_host_comb[which]) return SBVD_ERR_BAD_ARG;
    memcpy(g_host_comb[which], entries, bytes);
    if (!device) return 0;
#if defined(__HIPCC__)
    int rc = 0;
    if (!g_dev_comb[which]) rc = hip_fail(hipMalloc(&g_dev_comb[which], bytes));
    if (!rc) rc = hip_fail(hipMemcpy(g_dev_comb[which], entries, bytes, hipMemcpyHostToDevice));
    return rc;
#else
    return SBVD_ERR_NOT_AVAILABLE;
#endif
}
int sbvd_run(int backend, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (op < 0 || op >= OP_COUNT) return SBVD_ERR_BAD_OP;
    if ((backend != 0 && backend != 1) || n == 0 || n > SBVT_MAX_CASES || !in || !out) return SBVD_ERR_BAD_ARG;
    return backend == 1 ? run_device(op, in, out, n) : run_host(op, in, out, n);
}
}
