// gn_gemm.h -- what the projection translation units share: the argument structs and the launchers (gn_gemm.hip: slab
// kernel and entry points; gn_gemm_panel.hip; gn_gemm_colpipe.hip), the plane arithmetics (those three, the weight
// preparation of gn_gemm_split.hip, and the MFMA loops of gn_wgrad.hip and gn_eqff_fused.hip), and the pieces the three
// projection kernels have in common: the XCD cut of a tile list, the accumulator rescale, the three-term f16 product order
// and the epilogue value chain.
#pragma once
#include "gn_common.h"

namespace gn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmArgs {
    const float* A; const float* W; const float* bias; float* C;
    const float* res; const float* gate; float* pre_out;
    const float* a_pre; const float* a_gate;
    int lda, ldc, ldp, ldg, M, N, K;
    int act_lo, act_hi;
    int pro_mode, pro_lo, pro_hi;
    int row_cnt, row_gstride, row_goff;
    int gate_mode;                  // 0: value * gate; 1: value * SiLU'(gate)
    // K-segmented A operand: columns [s * a_seg, (s+1) * a_seg) of the logical A come from A / A2 / A3 (same row
    // addressing; A with leading dimension lda, A2 and A3 with lda2, below): sums up to three products that share their
    // output rows.  The last segment may be narrower than a_seg (K < 2 a_seg or < 3 a_seg).  a_seg = 0: plain A.
    const float* A2; const float* A3; int a_seg;
    int nt_store;                   // first output column written with non-temporal stores (outputs far larger than the L2s; INT_MAX: none)
    int act_kind;                   // GN_ACT_*: the activation of the epilogue columns, of gate_mode 1 and of the prologues
    int lda2;                       // leading dimension of A2 / A3 (the launcher resolves the descriptor's 0 to lda)
};

constexpr int GN_MAX_GROUP = 4;
struct GroupArgs {
    GemmArgs g[GN_MAX_GROUP];       // entries >= n repeat the last problem (never selected)
    int tile_end[GN_MAX_GROUP];     // running tile count: problem i owns the global tile ids [tile_end[i-1], tile_end[i])
    int n;
    int spread;                     // 1: every problem's tiles are cut into 8 XCD ranges; 0: one cut of the whole list
};

constexpr int BK = 32, PITCH = 36;

// ---- 3 x bf16 split (gn_gemm_split.hip) ----------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int SPLIT_PB = 40;    // bf16 per LDS row of an A plane (32 + 8 pad: 80-byte pitch, the 16-lane ds_read_b128
                                // groups hit 16 distinct 4-bank slots)

// x = hi + mid + lo EXACTLY, each a bf16 (8 significand bits): hi = x truncated to its top 16 bits, r1 = x - hi is
// exact (<= 16 significant bits), mid = r1 truncated, lo = r1 - mid has <= 8 significant bits left, so its own
// truncation is exact too.  (Truncation instead of round-to-nearest: two bit operations instead of a convert and a
// shift per plane, and no rounding term.)  Results below the fp32 normal range flush like any fp32 subtraction.
__device__ __forceinline__ unsigned pack_hi16(float a, float b) {      // (bf16(a), bf16(b)) by truncation
    return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ float trunc_bf16(float x) { return __uint_as_float(__float_as_uint(x) & 0xffff0000u); }
__device__ __forceinline__ void split4_trunc(float4 v, bf16x4& hi, bf16x4& mid, bf16x4& lo) {
    const float r0 = v.x - trunc_bf16(v.x), r1 = v.y - trunc_bf16(v.y);
    const float r2 = v.z - trunc_bf16(v.z), r3 = v.w - trunc_bf16(v.w);
    const float s0 = r0 - trunc_bf16(r0), s1 = r1 - trunc_bf16(r1);
    const float s2 = r2 - trunc_bf16(r2), s3 = r3 - trunc_bf16(r3);
    uint2 h, m, l;
    h.x = pack_hi16(v.x, v.y); h.y = pack_hi16(v.z, v.w);
    m.x = pack_hi16(r0, r1);   m.y = pack_hi16(r2, r3);
    l.x = pack_hi16(s0, s1);   l.y = pack_hi16(s2, s3);
    hi = __builtin_bit_cast(bf16x4, h);
    mid = __builtin_bit_cast(bf16x4, m);
    lo = __builtin_bit_cast(bf16x4, l);
}

// ---- 2 x fp16 split with block exponents (MODE 2) --------------------------------------------------------------
// x' = x * 2^-e with |x'| < 2^15 (e: a per-block power of two, see gemm_body), x' = hi + lo with hi = fp16(x') and
// lo = fp16(x' - hi): 22 significand bits in two planes, so an fp32 product needs THREE fp16 MFMAs (hi*hi, hi*lo, lo*hi;
// lo*lo is below 2^-22 of the product) instead of the six of the bf16 split.  fp16 has five exponent bits: elements more
// than 2^17 below their block's maximum keep fewer bits (absolute error <= 2^-39 of the block maximum) -- harmless in a
// dot product, which is dominated by the block's large elements.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// vector forms so that the compiler picks the packed instructions of gfx950: v_pk_mul_f32, v_cvt_pk_f16_f32 (round to
// nearest even), v_pk_add_f32 -- 3 VALU per element instead of 6 with scalar ldexp / convert / subtract
__device__ __forceinline__ void split4_f16(float4 v, float scale /* 2^-e */, f16x4& hi, f16x4& lo) {
    const f32x2 a0 = f32x2{v.x, v.y} * scale, a1 = f32x2{v.z, v.w} * scale;
    const f16x2 h0 = __builtin_convertvector(a0, f16x2), h1 = __builtin_convertvector(a1, f16x2);
    const f16x2 l0 = __builtin_convertvector(a0 - __builtin_convertvector(h0, f32x2), f16x2);
    const f16x2 l1 = __builtin_convertvector(a1 - __builtin_convertvector(h1, f32x2), f16x2);
    hi = f16x4{h0.x, h0.y, h1.x, h1.y};
    lo = f16x4{l0.x, l0.y, l1.x, l1.y};
}

// wave-wide maximum of an unsigned value without touching LDS: row_shr 1/2/4/8 (zero-filled), then row_bcast 15 and 31;
// the result is read from lane 63 and is wave-uniform (an SGPR)
__device__ __forceinline__ unsigned wave_umax_sgpr(unsigned v) {
    auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ int phys_row(const GemmArgs& p, int r) {
    // identity row map (row_cnt = 1: every product except the per-degree W_vk ones): no integer division -- the
    // epilogue calls this once per stored row, and a runtime division is ~40 VALU instructions
    if (p.row_cnt == 1) return r * p.row_gstride + p.row_goff;
    return (r / p.row_cnt) * p.row_gstride + p.row_goff + (r % p.row_cnt);
}

// ---- pieces shared by the slab, the panel and the column-loop kernel -------------------------------------------------
// XCD-aware order (block b runs on XCD b % 8, speed only): a list of T tiles is cut into 8 contiguous ranges and XCD x
// walks range x, [lo, lo + cnt) -- tiles that share their A rows are pulled through ONE L2 instead of all eight.
struct XcdCut { int lo, cnt; };
__device__ __forceinline__ XcdCut xcd_cut(int T, int xcd) {
    const int q = T >> 3, r = T & 7;
    return {xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, q + (xcd < r ? 1 : 0)};
}

__device__ __forceinline__ float exp_scale(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }   // 2^-e, e in [-120, 114]

// the three-term product of two split operands, smallest terms first: lo*hi, hi*lo, hi*hi (lo*lo is below 2^-22 of the
// product); term t multiplies plane F16_TA[t] of A with plane F16_TB[t] of the weight
constexpr int F16_TA[3] = {1, 0, 0};
constexpr int F16_TB[3] = {0, 1, 0};

// The block exponents (four signed bytes: one per 8-row block of a 32-row MFMA tile, accumulator registers 4q..4q+3)
// grew from e_old to e_new: bring the rows of `n` accumulator tiles along.  Exponents only grow: f <= 1, exact.
__device__ __forceinline__ void rescale_rows(f32x16* acc, int n, unsigned e_old, unsigned e_new) {
    asm volatile("" ::: "memory");                  // the caller's test is a real branch: never if-convert the multiplies
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float f = ldexpf(1.0f, (int)(signed char)(e_old >> (8 * q)) - (int)(signed char)(e_new >> (8 * q)));
#pragma unroll
        for (int t = 0; t < n; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][4 * q + r] *= f;
    }
}

// The epilogue's value chain for one float4 of one output row at element offset `off`:
//   x + bias -> pre_out -> activation (act: the column group lies in [act_lo, act_hi)) -> * gate or * act'(gate)
//   -> + res -> C, non-temporally from column nt_store on (gn: the float4's first column).
// rv / gv: the residual and gate values of that float4, loaded by the caller AHEAD of its stores, in an order that was
// measured at each site.  (The slab kernel's residual / gate branch states the chain in place, see there.)  A site without a
// gated / residual or non-temporal form (NT) passes nullptr / false and the compiler drops that link.  (float4s by reference,
// the column test at the store: by value and with the test ahead of the call the column-loop kernel spilled, 10 % longer.)
template <bool NT>
__device__ __forceinline__ void epi_store(const float4& x, const float4& bias4, size_t off, float* C, float* pre_out, bool act,
                                          int kind, const float* gate, int gate_mode, const float4& gv, const float* res,
                                          const float4& rv, int gn, int nt_store) {
    float4 v = x + bias4;
    if (pre_out) st4(pre_out + off, v);
    if (act) v = act4(v, kind);
    if (gate) v = v * (gate_mode ? dact4(gv, kind) : gv);
    if (res) v = rv + v;
    if (NT && gn >= nt_store) st4_nt(C + off, v); else st4(C + off, v);
}

// ---- column-loop kernel (gn_gemm_colpipe.hip) -----------------------------------------------------------------------
// Work decomposition: a UNIT is (row panel of 64, column pass of 128) of a problem, units are numbered panel-major.
// Workgroup w of G takes the units [w T / G, (w + 1) T / G) (T = all units of the group): every workgroup gets the same MFMA
// work to within one unit, and consecutive units of a workgroup are consecutive column passes of the same row panel.
struct ClArgs {
    GemmArgs g[GN_MAX_GROUP];
    long wend[GN_MAX_GROUP];        // running unit count: problem i owns the units [wend[i-1], wend[i])
    int n;
};
constexpr int CL_KC = 256;          // panel depth (one K chunk)
// workgroup barrier for LDS hand-over that does NOT drain the vector-memory counter (a __syncthreads() waits for every
// outstanding global store and load of the wave)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- host: the launchers -------------------------------------------------------------------------------------------------
// The kernel argument of a launch from its n <= GN_MAX_GROUP problems -- entries >= n repeat the last problem (never
// selected), end[i] = the running count of BM x BN output tiles (units).  Returns the count of all tiles.
template <class Args, class End>
inline long fill_group(Args& a, End (&end)[GN_MAX_GROUP], const GemmArgs* g, int n, int BM, int BN) {
    long run = 0;
    for (int i = 0; i < GN_MAX_GROUP; ++i) {
        a.g[i] = g[i < n ? i : n - 1];
        if (i < n) run += (long)((g[i].M + BM - 1) / BM) * ((g[i].N + BN - 1) / BN);
        end[i] = (End)run;
    }
    a.n = n;
    return run;
}
}  // namespace gn

// The two f16x2 kernels beside the slab kernel: their launchers take a validated group of n <= GN_MAX_GROUP problems with
// rows (GemmArgs as gn_gemm.hip makes them, nt_store included; W = the planes (+ header) written by gn_split_f16x2).
// the K-resident panel kernel for small f16x2 groups (gn_gemm_panel.hip): 1 = launched, 0 = does not apply, < 0 = -hipError_t
int gn_gemm_panel_launch(const gn::GemmArgs* g, int n, hipStream_t st);
// the column-loop kernel for large K = 256 f16x2 groups (gn_gemm_colpipe.hip): same return convention
int gn_gemm_colpipe_launch(const gn::GemmArgs* g, int n, hipStream_t st);
