// gn_gemm.hip -- fp32 dense projections on the CDNA4 matrix cores: the slab kernel, the routing and the entry points.
//
//   C[r, n] = epi( sum_k pro(A)[r, k] * W[n, k] + bias[n] )        W is nn.Linear's [out, in]
//
// Replaces every Dense/MLP on the path (reference layers.py:457-581; call sites
// gotennet.py:400-407, 432-441, 611, 728, 738) and, with transposed weights, their
// input-gradients in the force backward.  Exact fp32: v_mfma_f32_32x32x2_f32 is
// bitwise an fmaf chain, 157.3 TFLOP/s peak on MI355X (no TF32/xf32 on gfx950).
//
// Tiling: a 256-thread workgroup (4 waves as 2x2) owns a (64 TM) x (64 TN) output
// tile; each wave a (32 TM) x (32 TN) patch of 32x32 MFMA tiles.  TM = TN = 2 for
// the edge-sized products, TM = TN = 1 when the problem has too few 128x128 tiles to
// fill 256 CUs (atom-sized products: a wave's chain of 64-cycle MFMAs is the latency).
// (The plane arithmetics use 1 x 4 waves instead, and f16x2 1 x 8 waves -- 512 threads, a 128 x 256 tile -- for the K-heavy edge-sized
// products at most 256 columns wide, SLAB_TILES and tile_plan below; small f16x2 groups leave this file for the
// K-resident panel kernel of gn_gemm_panel.hip, wide K = 256 ones for the column-loop kernel of gn_gemm_colpipe.hip.)
// K in slabs of 32.  A and W slabs are staged through LDS as [rows][36] floats: the
// 36-float pitch keeps ds_read_b128 conflict-free for its 16-lane service groups
// (r*36 mod 64 hits 16 distinct 4-bank slots) and keeps 16-byte alignment.  Within a
// slab the K order is permuted so lanes 0-31 own k in [0,16) and lanes 32-63 own
// k in [16,32): each lane fetches its MFMA operands as contiguous float4s.  The next
// slab is prefetched into registers while the current one is multiplied.
//
// Prologue on A (applied while staging; columns [pro_lo, pro_hi) only):
//   1: A <- SiLU(A)                 (activations are stored pre-activation, consumers apply SiLU)
//   2: A <- A * SiLU'(P)            (backward through an activation; P = stored pre-activation)
//   and, for every column, A <- A * G when a_gate != NULL.
#include <climits>
#include <type_traits>
#include "gn_gemm.h"
#include "gn_tune.h"

namespace gn {

// ---- small pieces of the staging --------------------------------------------------------------------------------------
__device__ __forceinline__ float4 keep4(bool ok, const float4& v) {       // v, or zeros (four selects: never a branch around a load)
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}
__device__ __forceinline__ float amax4(const float4& v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// f16x2 block exponent of the R float4s every lane of a wave holds: the exponent bits of the wave-wide maximum -> e with
// |x| < 2^(e + 15), at least -120 (a signed byte; blocks below 2^-105 keep fewer bits).  An Inf in the block (a NaN never
// wins v_max) would give e = 114 and flush the block's finite rows: the block is scanned again for its FINITE maximum and only
// the rows that hold the Inf turn non-finite.  (The panel and column-loop kernels keep their own text: profiles/gemm_refactor_ab.txt)
template <int R>
__device__ __forceinline__ int block_exponent(const float4 (&v)[R]) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) m = fmaxf(m, amax4(v[i]));
    int need = (int)((wave_umax_sgpr(__float_as_uint(m)) >> 23) & 0xffu) - 126 - 15;          // |x| < 2^(need + 15)
    if (__builtin_expect(need > 112, 0)) {
        asm volatile("" ::: "memory");
        float mf = 0.f;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float c[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) mf = fmaxf(mf, fabsf(c[t]) <= 3.0e38f ? fabsf(c[t]) : 0.f);
        }
        need = (int)((wave_umax_sgpr(__float_as_uint(mf)) >> 23) & 0xffu) - 126 - 15;
    }
    return need < -120 ? -120 : need;
}
// x * scale as two fp16 planes, `apl` elements apart
__device__ __forceinline__ void store_f16x2(_Float16* d, int apl, const float4& v, float scale) {
    f16x4 h, l;
    split4_f16(v, scale, h, l);
    *reinterpret_cast<f16x4*>(d) = h;
    *reinterpret_cast<f16x4*>(d + apl) = l;
}

// SPLIT = true: the 3 x bf16-split arithmetic (gn_gemm_split.hip has the numerics): A is split into hi/mid/lo bf16
// planes while it is staged into LDS ([3][BM][40] bf16 per slab, double-buffered); the weight arrives pre-split in
// FRAGMENT-MAJOR order (gn_split_bf16x3: [n-tile of 32][k-step of 16][plane][lane][8 bf16], so one wave-wide 16-byte
// load is one contiguous KiB = exactly one MFMA B operand) and goes L2 -> registers, never through LDS: the weights
// are a few MB, L2-resident, and every wave needs a different column block.  Six v_mfma_f32_32x32x16_bf16 per
// 32x32x16 product block, fp32 accumulate; everything else (grouping, persistent tile walk, prologues, epilogue) is
// shared with the exact-fp32 instantiation.
// Wave grid: the 4 waves of a workgroup form WM x WN; each wave owns TM x TN MFMA tiles of 32 x 32, so the workgroup
// tile is (32 TM WM) x (32 TN WN).  Exact fp32: 2 x 2 waves.  SPLIT, 128 x 128 tile: 1 x 4 waves of 4 x 1 tiles -- every
// wave then needs ONE 32-column block of the weight per k-step (3 KiB from L2 through the 64 B/clk L1 path instead of
// 6 KiB with 2 x 2 tiles per wave) and re-reads the whole A slab from LDS, which has the bandwidth to spare.
// MODE: 0 exact fp32 MFMA, 1 three bf16 planes (six MFMA terms), 2 two scaled fp16 planes (three MFMA terms, gn_gemm.h)
template <int TM, int TN, int WM, int WN, bool PRO, int MODE, bool ASILU>
__device__ __forceinline__ void gemm_body(const GroupArgs ga) {
    constexpr int NW = WM * WN, NT = 64 * NW;       // waves and threads of the workgroup
    static_assert(NW == 4 || (NW == 8 && MODE == 2 && WM == 1), "four waves per workgroup, or 1 x 8 in the f16x2 arithmetic");
    constexpr bool SPLIT = MODE != 0;
    constexpr bool F16 = MODE == 2;
    constexpr int NP = F16 ? 2 : 3;                 // operand planes
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int SRS = 8 * NW;                     // rows one staging pass of the workgroup covers (8 float4 columns per row)
    constexpr int RA = BM / SRS, RB = BN / SRS;     // staged float4 rows per thread
    constexpr int EG = NW / 4;                      // F16: dwords of block exponents per slab buffer
    constexpr int STAGE = (BM + BN) * PITCH;        // floats per K-slab buffer (A rows then W rows)
    constexpr int CP = BN + 4;                      // epilogue tile pitch
    constexpr int APL = BM * SPLIT_PB;              // SPLIT: bf16 elements per A plane of a slab
    constexpr int STAGE_S = NP * APL;               // SPLIT: 16-bit elements per slab buffer
    constexpr int MAIN_FLOATS = SPLIT ? (2 * STAGE_S) / 2 : 2 * STAGE;
    constexpr int LDS_FLOATS = (MAIN_FLOATS > BM * CP) ? MAIN_FLOATS : BM * CP;
    // F16: + the block exponents of the two slab buffers, [2][4] signed bytes: wave q stages rows 8q..8q+7 of every
    // 32-row M-tile, and those rows -- accumulator registers 4q..4q+3 of every MFMA tile -- share ONE exponent per slab.
    // One dword per slab buffer, so "did anything change" is a single scalar compare per slab.
    // Eight waves (1 x 8, BM = 128): a staging pass covers 64 rows, so wave w stages rows 8 (w & 3) .. + 7 of the M-tiles
    // (w >> 2) and (w >> 2) + 2 -- 16 rows, and a 32-row block of the four-wave form is split between waves q and q + 4.  Giving both
    // halves ONE exponent would take a second workgroup barrier per slab (each wave's maximum is known only when its rows have
    // landed, right before the split), so the row grouping CHANGES here: every wave keeps its own exponent, [2][8] bytes, and
    // byte q of dword (i & 1) belongs to the accumulator registers 4q..4q+3 of M-tile i.  Blocks of 16 rows instead of 32: never a
    // larger exponent than the four-wave form's, the same per-row bound, but not the same bits.
    __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS + (F16 ? 2 * EG : 0)];
    signed char* const exps = reinterpret_cast<signed char*>(smem + LDS_FLOATS);
    int e_run = -120;                               // F16, staging side: running exponent of this wave's rows
    unsigned e_acc[EG];                             // F16, MFMA side: the block exponents (bytes) the accumulators are held in; M-tile i: e_acc[i % EG]
#pragma unroll
    for (int g = 0; g < EG; ++g) e_acc[g] = 0x88888888u;
    int ewt = 0;                                    // F16: the weight tensor's exponent (header of the packed planes)

    // ---- the tile walk: the XCD ranges, select, set_tile.  One launch walks the tiles of up to GN_MAX_GROUP independent
    // problems (a "group": the atom-sized products of a layer are too small to fill 256 CUs one at a time).  Inside a
    // problem tiles are row-tile major, so consecutive ids share their A rows.
    // XCD-aware order (block b runs on XCD b % 8, speed only): EVERY problem's tile list is cut into 8 contiguous
    // ranges, XCD x walks range x of problem 0, then range x of problem 1, ... -- an A row tile is pulled through ONE
    // L2 instead of all eight, and a problem with longer tiles (larger K) is spread over all XCDs.
    // grid = 8 * ceil(tiles / 8) capped; the excess exits.  Walk index j in [0, tiles_here).
    int cum[GN_MAX_GROUP], shift[GN_MAX_GROUP];      // cum: walk indices below cum[g] belong to problems <= g;
    const int xcd = blockIdx.x & 7;                  // shift: walk index j -> problem-local tile id j + shift[g]
    if (ga.spread) {
        int run = 0, prev_end = 0;
#pragma unroll
        for (int gi = 0; gi < GN_MAX_GROUP; ++gi) {
            const int tg = gi < ga.n ? ga.tile_end[gi] - prev_end : 0;
            prev_end = gi < ga.n ? ga.tile_end[gi] : prev_end;
            const XcdCut c = xcd_cut(tg, xcd);
            shift[gi] = c.lo - run;
            run += c.cnt;
            cum[gi] = run;
        }
    } else {
        // problems with equal tile lengths: ONE cut of the concatenated tile list (each XCD then touches one or two
        // weight matrices only: measured 46 vs 67 us on the x / v pair)
        int tiles_all = ga.tile_end[0];
#pragma unroll
        for (int gi = 1; gi < GN_MAX_GROUP; ++gi)
            if (gi < ga.n) tiles_all = ga.tile_end[gi];
        const XcdCut c = xcd_cut(tiles_all, xcd);
        const int lo = c.lo, hi = c.lo + c.cnt;
        int prev_end = 0;
#pragma unroll
        for (int gi = 0; gi < GN_MAX_GROUP; ++gi) {
            const int ge = gi < ga.n ? ga.tile_end[gi] : prev_end;
            const int a1 = ge < hi ? ge : hi;        // this XCD's part of problem gi ends at global id a1
            shift[gi] = lo - prev_end;               // walk index j is global id lo + j, problem-local id lo + j - prev_end
            cum[gi] = (a1 > lo ? a1 : lo) - lo;
            prev_end = ge;
        }
    }
    const int tile_stop = cum[GN_MAX_GROUP - 1];
    // the problem a walk index belongs to (indices only grow, so the scan never goes back)
    GemmArgs p = ga.g[0];
    int g_begin = -shift[0], g_end = cum[0], tiles_n = (p.N + BN - 1) / BN;
    auto select = [&](int t) {
#pragma unroll
        for (int gi = 1; gi < GN_MAX_GROUP; ++gi)
            if (t >= cum[gi - 1] && g_end <= cum[gi - 1]) {
                p = ga.g[gi];
                g_begin = -shift[gi];
                g_end = cum[gi];
            }
        tiles_n = (p.N + BN - 1) / BN;
    };
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int c4 = tid & 7;                         // staging map: thread -> (row sr + SRS i, float4 column c4)
    const int sr = tid >> 3;
    const int stride = gridDim.x >> 3;

    // ---- staging: global -> registers (fetchA / fetch) -> LDS (stash_f16 / stash_bf16 / stashA / stash) ------------------
    // fetch-side context of a tile (set one tile AHEAD at the end of the K loop: the first slab of the next
    // tile is already in flight while the current tile's epilogue runs)
    int prow[RA];
    const float* brow[RB];
    bool aok[RA], bok[RB];
    bool a_full = false;                            // every row of the tile is inside M and K is a multiple of the slab depth: no masks
    auto set_tile = [&](int t_idx) {
        const int m0f = ((t_idx - g_begin) / tiles_n) * BM, n0f = ((t_idx - g_begin) % tiles_n) * BN;
        a_full = m0f + BM <= p.M && (p.K % BK) == 0;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int gm = m0f + sr + SRS * i;
            aok[i] = gm < p.M;
            prow[i] = phys_row(p, aok[i] ? gm : 0);
        }
        if constexpr (!SPLIT) {
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int gn = n0f + sr + SRS * i;
                bok[i] = gn < p.N;
                brow[i] = p.W + (size_t)(bok[i] ? gn : 0) * p.K + 4 * c4;
            }
        }
    };

    f32x16 acc[TM][TN];

    // ONE register set of prefetched slabs (two and three sets measured no gain on MI355X and cost a wave of occupancy)
    float4 pa[RA], pb[RB];
    // AHEAD (planes, no prologue): branch-free A fetch into TWO register sets (slab s lives in set s & 1), so that the
    // compiler can count its loads exactly (exec-masked loads force conservative s_waitcnt: the HBM latency of the A
    // slab was exposed once per slab) and a slab stays in flight for two slab times.  The prologue instantiations and
    // exact fp32 keep the conditional loads of `fetch`.
    constexpr bool AHEAD = SPLIT && !PRO;
    float4 qa2[2][RA];
    bool kok2[2] = {true, true};
    auto fetchA = [&](int k0, float4 (&qa)[RA], bool& kflag) {
        const int kraw = k0 + 4 * c4;
        const bool kok = kraw < p.K;
        const int kc = kok ? kraw : 0;               // clamped: any valid column, zeroed by select in stashA
        const int k0c = kok ? k0 : 0;
        const float* Ab = p.A;
        int ka = kc, ld = p.lda;
        if (p.a_seg) {
            const bool s2 = k0c >= 2 * p.a_seg, s1 = k0c >= p.a_seg;
            Ab = s2 ? p.A3 : (s1 ? p.A2 : p.A);
            ka = kc - (s2 ? 2 * p.a_seg : (s1 ? p.a_seg : 0));
            // the segment's leading dimension goes with its base pointer (mask arithmetic: a select between two descriptor
            // fields is turned into an indexed load from a private copy, which then lives in scratch).  With ld a per-slab value
            // the row offsets prow * ld are no longer hoisted out of the K loop: one v_mad_i64_i32 per row and slab in place of
            // a 64-bit add, eight registers less (profiles/dt_kcat_ab.txt)
            ld = p.lda + ((p.lda2 - p.lda) & -(int)s1);
        }
#pragma unroll
        for (int i = 0; i < RA; ++i) qa[i] = ld4(Ab + (size_t)prow[i] * ld + ka);   // prow of a row past M is row 0: valid memory
        kflag = kok;
    };
    // F16: scale this wave's 8-row block of every M-tile by 2^-e (e = running maximum of the block's binary exponent
    // over the slabs staged so far, so that |x'| < 2^15), split x' = hi + lo into two fp16 planes, publish e
    auto stash_f16 = [&](int sb, const float4 (&v)[RA]) {
        _Float16* d0 = reinterpret_cast<_Float16*>(smem) + sb * STAGE_S + sr * SPLIT_PB + 4 * c4;
        const int need = block_exponent(v);
        e_run = need > e_run ? need : e_run;
        const float scale = exp_scale(e_run);
#pragma unroll
        for (int i = 0; i < RA; ++i) store_f16x2(d0 + SRS * i * SPLIT_PB, APL, v[i], scale);
        if (lane == 0) exps[sb * NW + wave] = (signed char)e_run;
    };
    // ... and the three bf16 planes of the staged rows
    auto stash_bf16 = [&](int sb, const float4 (&v)[RA]) {
        __bf16* d0 = reinterpret_cast<__bf16*>(smem) + sb * STAGE_S + sr * SPLIT_PB + 4 * c4;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            bf16x4 h, m, l;
            split4_trunc(v[i], h, m, l);
            __bf16* d = d0 + SRS * i * SPLIT_PB;
            *reinterpret_cast<bf16x4*>(d) = h;
            *reinterpret_cast<bf16x4*>(d + APL) = m;
            *reinterpret_cast<bf16x4*>(d + 2 * APL) = l;
        }
    };
    auto stashA = [&](int sb, const float4 (&qa)[RA], bool kflag) {
        if constexpr (F16) {
            if (a_full) {                            // interior tile (wave-uniform): 16 selects and their compares less per slab
                stash_f16(sb, qa);
                return;
            }
        }
        float4 v[RA];
#pragma unroll
        for (int i = 0; i < RA; ++i) v[i] = keep4(aok[i] && kflag, qa[i]);
        if constexpr (F16) stash_f16(sb, v);
        else stash_bf16(sb, v);
    };
    auto fetch = [&](int k0, float4 (&qa)[RA], float4 (&qb)[RB]) {
        if constexpr (AHEAD) {                           // (the cross-tile prefetch of a tile's first slab: set 0)
            fetchA(k0, qa2[0], kok2[0]);
            return;
        }
        const int kc = k0 + 4 * c4;
        const bool kok = kc < p.K;
        const bool pro = PRO && p.pro_mode && kc >= p.pro_lo && kc < p.pro_hi;
        // K-segmented A (a slab never straddles a segment: a_seg % BK == 0, checked by the launcher)
        const float* Ab = p.A;
        int ka = kc, ld = p.lda;
        if (p.a_seg) {
            if (k0 >= 2 * p.a_seg) { Ab = p.A3; ka = kc - 2 * p.a_seg; ld = p.lda2; }
            else if (k0 >= p.a_seg) { Ab = p.A2; ka = kc - p.a_seg; ld = p.lda2; }
        }
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            float4 v = zero4();
            if (aok[i] && kok) {
                v = ld4(Ab + (size_t)prow[i] * ld + ka);
                if constexpr (PRO) {
                    if (pro) v = (p.pro_mode == 1) ? act4(v, ASILU ? (int)GN_ACT_SILU : p.act_kind) : v * dact4(ld4(p.a_pre + (size_t)prow[i] * p.ldp + kc), ASILU ? (int)GN_ACT_SILU : p.act_kind);
                    if (p.a_gate) v = v * ld4(p.a_gate + (size_t)prow[i] * p.ldg + kc);
                }
            }
            qa[i] = v;
        }
        if constexpr (!SPLIT) {
#pragma unroll
            for (int i = 0; i < RB; ++i) qb[i] = (bok[i] && kok) ? ld4(brow[i] + k0) : zero4();
        }
    };
    // slab buffer `sb` (0 / 1) of the double buffer
    auto stash = [&](int sb, const float4 (&qa)[RA], const float4 (&qb)[RB]) {
        if constexpr (AHEAD) {
            stashA(sb, qa2[0], kok2[0]);
        } else if constexpr (F16) {
            stash_f16(sb, qa);
        } else if constexpr (SPLIT) {
            stash_bf16(sb, qa);
        } else {
            float* buf = smem + sb * STAGE;
#pragma unroll
            for (int i = 0; i < RA; ++i) st4(&buf[(sr + SRS * i) * PITCH + 4 * c4], qa[i]);
#pragma unroll
            for (int i = 0; i < RB; ++i) st4(&buf[(BM + sr + SRS * i) * PITCH + 4 * c4], qb[i]);
        }
    };
    // ---- planes: the weights.  B operands of k-step g (16 deep) for this wave's TN column blocks, NP planes each, L2 -> registers
    // (F16: the packed planes start with a 256-byte header whose first int is the weight tensor's exponent)
    const uint4* wfrag = reinterpret_cast<const uint4*>(p.W);
    int ks2 = 0;                                    // k-steps per column block in the fragment-major weight (even)
    size_t nt_off[TN];
    auto set_btile = [&](int n0b) {
        wfrag = reinterpret_cast<const uint4*>(p.W) + (F16 ? 16 : 0);
        if constexpr (F16) ewt = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(p.W));
        ks2 = 2 * ((p.K + BK - 1) / BK);
        const int nt_last = (p.N + 31) / 32 - 1;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int nt = n0b / 32 + wn * TN + j;
            nt = nt < nt_last ? nt : nt_last;        // column blocks past N: any valid block (results are never stored)
            nt_off[j] = (size_t)nt * ks2 * (NP * 64) + lane;
        }
    };
    auto load_b = [&](int g, uint4 (&q)[TN][NP]) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int s_ = 0; s_ < NP; ++s_) q[j][s_] = wfrag[nt_off[j] + (size_t)(g * NP + s_) * 64];
    };
    // F16: bring the accumulator rows of every 8-row block to the exponent slab buffer `sb` was staged with.  The
    // exponents only grow and settle after the first slabs: the common case is TM scalar compares that all fall through.
    auto rescale = [&](int sb) {
        if constexpr (EG == 1) {
            const unsigned en = (unsigned)__builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(exps + sb * 4));
            if (__builtin_expect(en != e_acc[0], 0)) {
                rescale_rows(&acc[0][0], TM * TN, e_acc[0], en);
                e_acc[0] = en;
            }
        } else {
            // eight waves: M-tile i was staged by the waves q + 4 (i & 1), dword i & 1 of the slab's exponents
            unsigned en[EG];
            bool same = true;
#pragma unroll
            for (int g = 0; g < EG; ++g) {
                en[g] = (unsigned)__builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(exps + sb * NW + 4 * g));
                same = same && en[g] == e_acc[g];
            }
            if (__builtin_expect(!same, 0)) {
#pragma unroll
                for (int i = 0; i < TM; ++i) rescale_rows(&acc[i][0], TN, e_acc[i % EG], en[i % EG]);
#pragma unroll
                for (int g = 0; g < EG; ++g) e_acc[g] = en[g];
            }
        }
    };

    // ---- planes: one 16-deep k-step of the wave's TM x TN MFMA tiles, either arithmetic -----------------------------------
    // Ap: this lane's fragment row in the A planes of the slab, bw: the weight fragments.  Consecutive MFMAs rotate over
    // the TM*TN accumulators so that none waits on the one before it.
    auto kstep = [&](const __bf16* Ap, int ks, const uint4 (&bw)[TN][NP]) {
        if constexpr (F16) {
            f16x8 a[TM][2];                          // the three terms of gn_gemm.h
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_)
                    a[i][s_] = *reinterpret_cast<const f16x8*>(Ap + s_ * APL + i * 32 * SPLIT_PB + ks * 16);
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                            a[i][F16_TA[t]], __builtin_bit_cast(f16x8, bw[j][F16_TB[t]]), acc[i][j], 0, 0, 0);
        } else {
            bf16x8 a[TM][3];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int s_ = 0; s_ < 3; ++s_)
                    a[i][s_] = *reinterpret_cast<const bf16x8*>(Ap + s_ * APL + i * 32 * SPLIT_PB + ks * 16);
            // smallest terms first (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi)
            constexpr int TA[6] = {2, 0, 1, 1, 0, 0};
            constexpr int TB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            a[i][TA[t]], __builtin_bit_cast(bf16x8, bw[j][TB[t]]), acc[i][j], 0, 0, 0);
        }
    };

    // ---- the main loops over the nk slabs of a tile: double-buffered LDS, one barrier per slab.  On entry slab 0 is
    // staged in buffer 0 and, in the plane arithmetics, the weights of k-step 0 are in bq[0] -----------------------------
    // Planes: one slab = two 16-deep k-steps.  While slab kt is multiplied: the weights of the NEXT k-step are in flight
    // (L2 -> registers), slab kt + 1 (already in registers) is split and written to the other LDS buffer, and after
    // the barrier slab kt + 2 goes in flight from HBM.  AHEAD: the last slab is peeled so that the steady-state body has no
    // conditional code: it is ONE scheduling region and the split arithmetic can sit in the MFMAs' shadow.  Load order per
    // slab kt (vmcnt retires in order): weights of k-step 2kt+1, THEN the A slab kt+2 (two slab times ahead), mid-slab the
    // weights of k-step 2kt+2: nothing that is needed soon ever queues behind an A load younger than one slab time.
    // sched_barrier(0) keeps the phases apart (without them the scheduler hoists across the whole region until the
    // 256-register budget spills: measured 15-30 % slower).
    // EARLY (eight waves, GN_F16_BIG8_PHASED): the two waves of a SIMD (w and w + 4) run the phases of a slab in OPPOSITE order.
    // All eight waves meet at one barrier per slab, so left alone they multiply at the same time and split at the same time:
    // the matrix pipe idles while both waves of a SIMD are in their split.  An early wave writes slab kt + 1 to LDS FIRST (the
    // other buffer: last read before the barrier that ended slab kt - 1) and multiplies slab kt after it, while its partner
    // multiplies first and splits last.  Its A slabs stay two slab times in flight as well: it requests slab kt + 3 right after the
    // split, into the registers the split freed (past K the loads are clamped to valid memory and never used).
    auto loop_planes_ahead = [&](int nk, uint4 (&bq)[2][TN][NP], auto EARLY) {
        constexpr bool early = decltype(EARLY)::value;
        const __bf16* const Abase = reinterpret_cast<const __bf16*>(smem) + (wm * 32 * TM + (lane & 31)) * SPLIT_PB + (lane >> 5) * 8;
        auto slab = [&](int kt, auto SET, auto LAST) {
            constexpr int set = decltype(SET)::value;            // register set of slab kt (= kt & 1)
            constexpr bool last = decltype(LAST)::value;
            const __bf16* Ap = Abase + set * STAGE_S;
            load_b(2 * kt + 1, bq[1]);
            if constexpr (!early) {
                if constexpr (!last) fetchA((kt + 2) * BK, qa2[set], kok2[set]);   // slab kt + 2 -> the set slab kt came from
            } else if constexpr (!last) {
                stashA(set ^ 1, qa2[set ^ 1], kok2[set ^ 1]);                      // slab kt + 1 -> the other LDS buffer
                __builtin_amdgcn_sched_barrier(0);
                fetchA((kt + 3) * BK, qa2[set ^ 1], kok2[set ^ 1]);                // slab kt + 3 -> the set that was just split
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (F16) rescale(set);
            kstep(Ap, 0, bq[0]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!last) load_b(2 * kt + 2, bq[0]);
            kstep(Ap, 1, bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!last && !early) stashA(set ^ 1, qa2[set ^ 1], kok2[set ^ 1]);  // slab kt + 1 -> the other LDS buffer
            __syncthreads();
        };
        using T0 = std::integral_constant<int, 0>; using T1 = std::integral_constant<int, 1>;
        using No = std::false_type; using Yes = std::true_type;
        fetchA(BK, qa2[1], kok2[1]);             // slab 1 (zero-filled past K); slab 0 is already staged
        if constexpr (early) fetchA(2 * BK, qa2[0], kok2[0]);
        int kt = 0;
        for (; kt + 2 < nk; kt += 2) {
            slab(kt, T0{}, No{});
            slab(kt + 1, T1{}, No{});
        }
        if (nk - kt == 2) {
            slab(kt, T0{}, No{});
            slab(kt + 1, T1{}, Yes{});
        } else {
            slab(kt, T0{}, Yes{});
        }
    };

    // ---- persistent over tiles: workgroup b walks the tiles base + b/8, base + b/8 + gridDim/8, ... of ITS XCD's range
    int idx = blockIdx.x >> 3;
    if (idx >= tile_stop) return;
    select(idx);
    set_tile(idx);
    fetch(0, pa, pb);
    for (;;) {
        const int nk = (p.K + BK - 1) / BK;
        const int m0 = ((idx - g_begin) / tiles_n) * BM;
        const int n0 = ((idx - g_begin) % tiles_n) * BN;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        if constexpr (F16) {
            e_run = -120;
#pragma unroll
            for (int g = 0; g < EG; ++g) e_acc[g] = 0x88888888u;   // -120 in every byte (the accumulators are zero)
        }
        stash(0, pa, pb);
        uint4 bq[2][TN][NP];
        if constexpr (SPLIT) {
            set_btile(n0);
            load_b(0, bq[0]);
        }
        __syncthreads();
        if constexpr (AHEAD && NW == 8 && GN_F16_BIG8_PHASED) {
            if (GN_F16_BIG8_PHASED == 2 ? (__builtin_amdgcn_readfirstlane(wave) & 1) : (__builtin_amdgcn_readfirstlane(wave) >= 4)) loop_planes_ahead(nk, bq, std::true_type{});
            else loop_planes_ahead(nk, bq, std::false_type{});
        } else if constexpr (AHEAD) loop_planes_ahead(nk, bq, std::false_type{});
        else if constexpr (SPLIT) {
            // Planes with a prologue, the conditional form, in place (as a lambda the [54368 x 256 x 1536] prologue launch
            // measured 2.5 % slower): weights, MFMAs and the split each in their own basic block.  (A branch-free single
            // block, with or without sched_group_barrier interleaving, measured 15-30 % SLOWER on MI355X: the scheduler
            // hoists until the 256-register budget spills.)
            const __bf16* const Abase = reinterpret_cast<const __bf16*>(smem) + (wm * 32 * TM + (lane & 31)) * SPLIT_PB + (lane >> 5) * 8;
            if (nk > 1) fetch(BK, pa, pb);
            for (int kt = 0; kt < nk; ++kt) {
                const __bf16* Ap = Abase + (kt & 1) * STAGE_S;
                load_b(2 * kt + 1, bq[1]);
                if constexpr (F16) rescale(kt & 1);
                kstep(Ap, 0, bq[0]);
                if (kt + 1 < nk) load_b(2 * kt + 2, bq[0]);
                kstep(Ap, 1, bq[1]);
                if (kt + 1 < nk) stash((kt + 1) & 1, pa, pb);
                __syncthreads();
                if (kt + 2 < nk) fetch((kt + 2) * BK, pa, pb);
            }
        }
        else {
            // Exact fp32, in place (as a third lambda it cost gemm_f32_mfma<2,2,2,2,false,false> a VGPR): the register set holds
            // slab kt + 1 when slab kt is multiplied and is refilled with slab kt + 2 right after it has been written to LDS
            const int khalf = (lane >> 5) * 16;
            const int frow = lane & 31;
            if (1 < nk) fetch(BK, pa, pb);
            for (int kt = 0; kt < nk; ++kt) {
                const float* As = smem + (kt & 1) * STAGE;
                const float* Bs = As + BM * PITCH;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    float a[TM][8], b[TN][8];
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const float* ap = &As[(wm * 32 * TM + i * 32 + frow) * PITCH + khalf + hh * 8];
                        const float4 a0 = ld4(ap), a1 = ld4(ap + 4);
                        a[i][0] = a0.x; a[i][1] = a0.y; a[i][2] = a0.z; a[i][3] = a0.w;
                        a[i][4] = a1.x; a[i][5] = a1.y; a[i][6] = a1.z; a[i][7] = a1.w;
                    }
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const float* bp = &Bs[(wn * 32 * TN + j * 32 + frow) * PITCH + khalf + hh * 8];
                        const float4 b0 = ld4(bp), b1 = ld4(bp + 4);
                        b[j][0] = b0.x; b[j][1] = b0.y; b[j][2] = b0.z; b[j][3] = b0.w;
                        b[j][4] = b1.x; b[j][5] = b1.y; b[j][6] = b1.z; b[j][7] = b1.w;
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q)
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int j = 0; j < TN; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[j][q], acc[i][j], 0, 0, 0);
                }
                if (kt + 1 < nk) stash((kt + 1) & 1, pa, pb);   // other buffer: last read in iteration kt-1
                __syncthreads();
                if (kt + 2 < nk) fetch((kt + 2) * BK, pa, pb);
            }
        }

        // next tile's first slab goes in flight now and lands during the epilogue (same problem only: the epilogue
        // below still needs this problem's arguments)
        const int next = idx + stride;
        const bool has_next = next < tile_stop;
        const bool same = has_next && next < g_end;
        if (same) {
            set_tile(next);
            fetch(0, pa, pb);
        }

        // ---- the epilogue (inline: as two lambdas, accumulators -> LDS and LDS -> rows, it cost 2 VGPRs in the big bf16x3
        // kernel and 4 in the small exact-fp32 ones; profiles/gemm_refactor_ab.txt)
        // (An epilogue straight from the accumulators -- a lane owns one column of each 32 x 32 tile, so a store instruction
        // would write two full 128-byte row segments with no LDS round trip -- measured 2x SLOWER per tile: 64 dword stores
        // per lane instead of 16 dwordx4; tools/gemm_trace.py.)
        {
        // epilogue through LDS: accumulators -> [BM][BN+4] tile -> coalesced float4 rows
        // (lane holds column (lane & 31), rows (r&3) + 8 (r>>2) + 4 (lane>>5) of each 32x32 tile)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    float v = acc[i][j][r];
                    if constexpr (F16) v = ldexpf(v, (int)(signed char)(e_acc[i % EG] >> (8 * (r >> 2))) + ewt);   // back from the block / weight exponents (only the RESULT may under- / overflow)
                    smem[row * CP + wn * 32 * TN + j * 32 + (lane & 31)] = v;
                }
        __syncthreads();
        {
            constexpr int C4 = BN / 4;                  // NT % C4 == 0: a thread keeps ONE column group
            const int cc = (tid % C4) * 4, gn = n0 + cc;
            if (gn < p.N) {
                const float4 bias4 = p.bias ? ld4(p.bias + gn) : zero4();
                const bool act = gn >= p.act_lo && gn < p.act_hi;          // act ranges are multiples of 4
                const int kind = ASILU ? (int)GN_ACT_SILU : p.act_kind;
                if (p.res || p.gate) {
                    // four rows per pass, all residual / gate loads of the pass issued BEFORE its first store: the
                    // stores may alias them as far as the compiler knows (res == C is allowed), and a load behind
                    // a store was one exposed round trip per row
                    constexpr int ITS = (BM * C4) / NT, UN = ITS < 4 ? ITS : 4;
                    for (int it0 = 0; it0 < ITS; it0 += UN) {
                        size_t off[UN];
                        bool ok[UN];
                        float4 rv[UN], gv[UN];
#pragma unroll
                        for (int u = 0; u < UN; ++u) {
                            const int gm = m0 + (it0 + u) * (NT / C4) + tid / C4;
                            ok[u] = gm < p.M;
                            off[u] = (size_t)phys_row(p, ok[u] ? gm : 0) * p.ldc + gn;
                            rv[u] = (ok[u] && p.res) ? ld4(p.res + off[u]) : zero4();
                            gv[u] = (ok[u] && p.gate) ? ld4(p.gate + off[u]) : zero4();
                        }
#pragma unroll
                        for (int u = 0; u < UN; ++u) {
                            if (!ok[u]) continue;
                            const int row = (it0 + u) * (NT / C4) + tid / C4;
                            // the chain of epi_store (gn_gemm.h) stated in place: through the function the exact-fp32
                            // prologue kernel without a compile-time activation took 100 VGPRs instead of 94
                            float4 v = ld4(&smem[row * CP + cc]) + bias4;
                            if (p.pre_out) st4(p.pre_out + off[u], v);
                            if (act) v = act4(v, ASILU ? (int)GN_ACT_SILU : p.act_kind);
                            if (p.gate) v = v * (p.gate_mode ? dact4(gv[u], ASILU ? (int)GN_ACT_SILU : p.act_kind) : gv[u]);
                            if (p.res) v = rv[u] + v;
                            st4(p.C + off[u], v);
                        }
                    }
                } else {
#pragma unroll 4
                    for (int it = 0; it < (BM * C4) / NT; ++it) {
                        const int row = it * (NT / C4) + tid / C4;
                        const int gm = m0 + row;
                        if (gm >= p.M) continue;
                        const float4 x = ld4(&smem[row * CP + cc]);
                        const size_t off = (size_t)phys_row(p, gm) * p.ldc + gn;
                        epi_store<true>(x, bias4, off, p.C, p.pre_out, act, kind, nullptr, 0, zero4(), nullptr, zero4(), gn, p.nt_store);
                    }
                }
            }
        }
        __syncthreads();                                // LDS is reused by the next tile's first slab
        }
        if (!has_next) break;
        if (!same) {                                    // first tile of the next problem
            select(next);
            set_tile(next);
            fetch(0, pa, pb);
        }
        idx = next;
    }
}

// ASILU: every problem of the launch uses SiLU (the reference's default): the activation is a compile-time constant.
// With the kind as a run-time switch the eleven other activations' code cost the 128x128 split kernel a 36-byte spill
// and the 64x64 fp32 kernel a wave of occupancy; models with another activation take the !ASILU instantiations.
template <int TM, int TN, int WM, int WN, bool PRO, bool ASILU>
__global__ __launch_bounds__(256) void gemm_f32_mfma(const GroupArgs ga) {
    gemm_body<TM, TN, WM, WN, PRO, 0, ASILU>(ga);
}

// 3 x bf16-split instantiation: two workgroups per CU (one wave of each per SIMD: while one is in its epilogue or at a
// barrier the other feeds the matrix pipe), so the register budget is capped at 256 per lane.
template <int TM, int TN, int WM, int WN, bool PRO, bool ASILU>
__global__ __launch_bounds__(256, GN_SPLIT_MINW) void gemm_bf16x3_mfma(const GroupArgs ga) {
    gemm_body<TM, TN, WM, WN, PRO, 1, ASILU>(ga);
}

// 2 x fp16-split instantiation (three MFMA terms per product, block exponents): same grid and tile shapes, and the 1 x 8-wave
// form (512 threads: ONE workgroup per CU holds the two waves per SIMD that two four-wave workgroups hold)
template <int TM, int TN, int WM, int WN, bool PRO, bool ASILU>
__global__ __launch_bounds__(64 * WM * WN, GN_SPLIT_MINW) void gemm_f16x2_mfma(const GroupArgs ga) {
    gemm_body<TM, TN, WM, WN, PRO, 2, ASILU>(ga);
}

}  // namespace gn

// =========================================================== host ===========================================================
namespace {
using gn::GemmArgs;
using SlabKernel = void (*)(const gn::GroupArgs);

// ---- the slab tiles: the wave layout of every (arithmetic, tile) that is built; TM = 0: not built ----------------------
enum Tile { TILE_BIG, TILE_MID, TILE_WIDE, TILE_SMALL, TILE_BIG8, TILE_COUNT };
struct TileShape {
    int TM, TN, WM, WN;
    constexpr int BM() const { return 32 * TM * WM; }
    constexpr int BN() const { return 32 * TN * WN; }
};
constexpr TileShape SLAB_TILES[3][TILE_COUNT] = {
    //  big 128 x 128   mid 64 x 128    wide 32 x 128   small 64 x 64   big8 128 x 256 (eight waves, no prologue)
    {{2, 2, 2, 2}, {0, 0, 0, 0}, {0, 0, 0, 0}, {1, 1, 2, 2}, {0, 0, 0, 0}},       // exact fp32
    {{4, 1, 1, 4}, {0, 0, 0, 0}, {0, 0, 0, 0}, {1, 1, 2, 2}, {0, 0, 0, 0}},       // bf16x3
    {{4, 1, 1, 4}, {2, 1, 1, 4}, {1, 1, 1, 4}, {1, 1, 2, 2}, {4, 1, 1, 8}},       // f16x2
};

template <int MODE, int T, bool PRO, bool ASILU>
SlabKernel slab_kernel() {
    constexpr TileShape s = SLAB_TILES[MODE][T];
    if constexpr (s.TM == 0 || (T == TILE_BIG8 && PRO)) return nullptr;
    else if constexpr (MODE == 0) return gn::gemm_f32_mfma<s.TM, s.TN, s.WM, s.WN, PRO, ASILU>;
    else if constexpr (MODE == 1) return gn::gemm_bf16x3_mfma<s.TM, s.TN, s.WM, s.WN, PRO, ASILU>;
    else return gn::gemm_f16x2_mfma<s.TM, s.TN, s.WM, s.WN, PRO, ASILU>;
}
template <int MODE, int T>
SlabKernel slab_kernel(bool pro, bool silu) {
    return pro ? (silu ? slab_kernel<MODE, T, true, true>() : slab_kernel<MODE, T, true, false>())
               : (silu ? slab_kernel<MODE, T, false, true>() : slab_kernel<MODE, T, false, false>());
}
template <int MODE>
SlabKernel slab_kernel(Tile t, bool pro, bool silu) {
    switch (t) {
    case TILE_BIG: return slab_kernel<MODE, TILE_BIG>(pro, silu);
    case TILE_MID: return slab_kernel<MODE, TILE_MID>(pro, silu);
    case TILE_WIDE: return slab_kernel<MODE, TILE_WIDE>(pro, silu);
    case TILE_BIG8: return slab_kernel<MODE, TILE_BIG8>(pro, silu);
    default: return slab_kernel<MODE, TILE_SMALL>(pro, silu);
    }
}

// The slab tile of a group and the cap of its persistent grid (2 / 3 / 4 workgroups per CU walk the tile list: +2 %)
struct TilePlan { Tile tile; long cap; };
// form: GN_GEMM_FORM_* of gn_gemm_group_f16x2_form -- 0: the routing below; otherwise the caller names the 128-row tile
TilePlan tile_plan(const GemmArgs* g, int n, int split, bool pro, int form) {
    if (form == GN_GEMM_FORM_BIG) return {TILE_BIG, GN_GEMM_BIG_CAP};
    if (form == GN_GEMM_FORM_BIG8) return {TILE_BIG8, GN_F16_BIG8_CAP};
    long big = 0, rows_all = 0;
    bool wide = GN_F16_SMALL_WIDE && split == 2, gated = false;
    bool big8 = GN_F16_BIG8_MIN_K > 0 && split == 2 && !pro && g[0].K >= GN_F16_BIG8_MIN_K && g[0].N > 128;
    for (int i = 0; i < n; ++i) {
        big += (long)((g[i].M + 127) / 128) * ((g[i].N + 127) / 128);
        wide = wide && g[i].N >= 128;
        big8 = big8 && g[i].N <= 256;
        rows_all += g[i].M;
        gated = gated || (g[i].gate != nullptr && g[i].res != nullptr);
    }
    // f16x2, edge-sized K-heavy groups at most 256 columns wide (the input-gradient products dL/dt = [g_eproj | g_pre_t] W + gt
    // and their riders): 128 x 256 tiles of 1 x 8 waves -- an A slab is fetched, scaled and split ONCE per row panel
    // instead of once per 128 columns (GN_F16_BIG8_MIN_K, gn_tune.h; profiles/dt_wide_ab.txt)
    if (big8 && big >= (long)GN_GEMM_BIG_MIN) return {TILE_BIG8, GN_F16_BIG8_CAP};
    // 128x128 tiles from GN_GEMM_BIG_MIN = 900 tiles up (measured switch-over; a build-time constant of gn_tune.h, swept
    // with tools/variants.py): the [E x 256 x K] products (850 tiles = 1.66 rounds on 512 resident workgroups) run
    // 4-20 % faster as 3400 64x64 tiles, the [E x 1536 x 256] product (5100 tiles) and the four-problem X group (1008)
    // want the big tile
    if (big >= (long)GN_GEMM_BIG_MIN) return {TILE_BIG, GN_GEMM_BIG_CAP};
    // f16x2, small-tile groups with many rows: 64 x 128 tiles (waves 1 x 4 of 2 x 1 MFMA tiles) -- a weight fragment serves two
    // row tiles, half the L2 -> CU weight traffic of the 32 x 128 tile per output row (GN_F16_MID_ROWS, gn_tune.h; 0: never)
    // Measured (round 6, MI355X): the gated residual launch [54368 x 256 x 256]g + rider 75 -> 68.8 us in the step (stand-alone 69.3
    // -> 65.7, ungated 42.9 -> 37.5); the ungated launches of the step tie or lose 2 us (their riders have K = 512), so only
    // groups with a gated residual epilogue take it
    if (wide && gated && GN_F16_MID_ROWS > 0 && rows_all >= (long)GN_F16_MID_ROWS) return {TILE_MID, GN_F16_MID_CAP};
    // the f16x2 small tile is 32 x 128 (waves 1 x 4: a row is split once per 128 columns) unless a problem is narrower than a tile
    if (wide) return {TILE_WIDE, GN_F16_SMALL_CAP};
    return {TILE_SMALL, 1024};
}

// the slab kernel: every group
int slab_launch(const GemmArgs* g, int n, hipStream_t st, int split, int form = 0) {
    bool pro = false, silu = true;
    for (int i = 0; i < n; ++i) {
        pro = pro || g[i].pro_mode != 0 || g[i].a_gate != nullptr;
        silu = silu && g[i].act_kind == GN_ACT_SILU;
    }
    if (form != 0 && (split != 2 || (form == GN_GEMM_FORM_BIG8 && pro))) return GN_ERR_BAD_ARG;
    const TilePlan plan = tile_plan(g, n, split, pro, form);
    const TileShape shape = SLAB_TILES[split][plan.tile];
    gn::GroupArgs ga;
    const long tiles = gn::fill_group(ga, ga.tile_end, g, n, shape.BM(), shape.BN());
    if (tiles == 0) return GN_OK;
    // per-problem XCD ranges when the problems are unlike (different tile lengths K, or a small problem riding with
    // a large one: its tiles would otherwise all sit at the end of the last XCD's range)
    ga.spread = 0;
    for (int i = 0; i < n; ++i) {
        const long t0 = ga.tile_end[0], ti = ga.tile_end[i] - (i ? ga.tile_end[i - 1] : 0);
        ga.spread |= (g[i].K != g[0].K) || ti * 4 < t0 || t0 * 4 < ti;
    }
    long grid = 8L * ((tiles + 7) / 8);
    if (grid > plan.cap) grid = plan.cap;
    const SlabKernel k = split == 2 ? slab_kernel<2>(plan.tile, pro, silu)
                       : split == 1 ? slab_kernel<1>(plan.tile, pro, silu) : slab_kernel<0>(plan.tile, pro, silu);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * shape.WM * shape.WN), 0, st, ga);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

// ---- arguments ---------------------------------------------------------------------------------------------------------
bool act_kind_ok(int k) { return k >= 0 && k < GN_ACT_COUNT; }

// every check of one problem
bool desc_ok(const gn_gemm_desc& q) {
    if (q.M < 0 || q.N <= 0 || q.K <= 0 || (q.K & 3) || (q.lda & 3) || (q.N & 3) || (q.ldc & 3) || (q.act_lo & 3) ||
        (q.act_hi & 3) || q.row_cnt <= 0)
        return false;
    if (q.gate != nullptr && q.res == nullptr && q.gate_mode == 0) return false;
    if (q.pro_mode < 0 || q.pro_mode > 2 || (q.pro_mode == 2 && (!q.a_pre || (q.ldp & 3))) || (q.a_gate && (q.ldg & 3)) ||
        (q.pro_mode && ((q.pro_lo & 3) || (q.pro_hi & 3))))
        return false;
    if (q.a_seg < 0 || (q.a_seg && ((q.a_seg % gn::BK) || q.pro_mode || q.a_gate || q.K > 3 * q.a_seg ||
                                    !q.A2 || (q.K > 2 * q.a_seg && !q.A3) || q.lda2 < 0 || (q.lda2 & 3))))
        return false;
    // (a problem without rows of a group is skipped before its activation is looked at; gemm_single looks first)
    return q.M == 0 || act_kind_ok(q.act_kind);
}

// the kernels' view of one checked problem
GemmArgs make_args(const gn_gemm_desc& q) {
    GemmArgs p;
    p.A = q.A; p.W = q.W; p.bias = q.bias; p.C = q.C;
    p.res = q.res; p.gate = q.gate; p.pre_out = q.pre_out;
    p.a_pre = q.a_pre; p.a_gate = q.a_gate;
    p.lda = q.lda; p.ldc = q.ldc; p.ldp = q.ldp; p.ldg = q.ldg;
    p.M = q.M; p.N = q.N; p.K = q.K;
    p.act_lo = q.act_lo; p.act_hi = q.act_hi;
    p.pro_mode = q.pro_mode; p.pro_lo = q.pro_lo; p.pro_hi = q.pro_hi;
    p.row_cnt = q.row_cnt; p.row_gstride = q.row_gstride; p.row_goff = q.row_goff;
    p.gate_mode = q.gate_mode;
    p.A2 = q.A2; p.A3 = q.A3; p.a_seg = q.a_seg;
    p.act_kind = q.act_kind;
    p.lda2 = q.lda2 ? q.lda2 : q.lda;              // 0: A2 / A3 share A's leading dimension
    // outputs of 100 MB and more (the [E, (1+M)F] edge projection) are stored non-temporally from column nt_store on: later
    // kernels consume them from HBM anyway and they would only evict the node tables (K6 +5 %); GN_GEMM_NT_MB (gn_tune.h).
    // The first K columns stay on the normal path: for the edge projection [W_re | W_rs] that is the attention block, which
    // the segment softmax re-reads right away -- 23.3 -> 20.6 us for it at C2; GN_GEMM_NT_LO >= 0 fixes the column instead
    const int nt_lo = GN_GEMM_NT_LO >= 0 ? GN_GEMM_NT_LO : q.K;
    p.nt_store = (double)q.M * q.N * 4.0 >= (double)GN_GEMM_NT_MB * 1048576.0 ? (q.N > nt_lo ? nt_lo : 0) : INT_MAX;
    return p;
}

// The K-concatenated input-gradient of the X products, gX1 = gX + [gXp | gEQ | gEK_l] [W_vu^T | W_vq^T | W_vk_l^T]^T per degree
// block, and groups like it -- f16x2, no prologue, EVERY problem K-segmented, at least 768 deep and 129 .. 256 columns wide,
// GN_F16_XCAT_MIN_ROWS rows or more in the group: the eight-wave 128 x 256 tile, ahead of the panel kernel (32 x 128 tiles:
// the weight fragments of a 768-deep product are re-read from L2 for every 32 rows, an A row is converted for each of the
// two column tiles).  Below the row threshold the panel kernel keeps them (gn_tune.h; profiles/xside_ab.txt).
bool xcat_big8(const GemmArgs* g, int n) {
    if (GN_F16_XCAT_MIN_ROWS <= 0) return false;
    long rows = 0;
    for (int i = 0; i < n; ++i) {
        if (g[i].pro_mode != 0 || g[i].a_gate != nullptr || g[i].a_seg == 0 || g[i].K < 768 || g[i].N > 256 || g[i].N <= 128)
            return false;
        rows += g[i].M;
    }
    return rows >= (long)GN_F16_XCAT_MIN_ROWS;
}

// One launch for a validated group (GemmArgs from make_args: nt_store included); split: 0 exact fp32, 1 bf16x3, 2 f16x2).  The routing, in this order (each launcher states its conditions in full):
//   0. f16x2: the eight-wave slab tile for K-segmented groups with many rows (xcat_big8 above);
//   1. f16x2: the K-resident panel kernel -- no prologue, at most GN_GEMM_PANEL_MAX tiles of 32 x 128, one depth K in
//      {128, 256, 512} or depths that are all multiples of 256;
//   2. f16x2: the column-loop kernel -- SiLU, no prologue, no K segments, K = 256, a product >= GN_CP_MIN_N columns wide
//      and >= GN_CP_MIN_TILES tiles of 64 x 128;   3. the slab kernel of this file: everything else, every arithmetic.
int gemm_launch(const GemmArgs* g, int n, hipStream_t st, int split, int form) {
    if (form != 0) return slab_launch(g, n, st, split, form);
    if (split == 2) {
        if (xcat_big8(g, n)) return slab_launch(g, n, st, split, GN_GEMM_FORM_BIG8);
        int r = gn_gemm_panel_launch(g, n, st);
        if (r == 0) r = gn_gemm_colpipe_launch(g, n, st);
        if (r != 0) return r > 0 ? GN_OK : -r;
    }
    return slab_launch(g, n, st, split);
}

int gemm_group_impl(const gn_gemm_desc* d, int n, void* stream, int split, int form = 0) {
    if (n < 0 || n > gn::GN_MAX_GROUP || (n > 0 && !d)) return GN_ERR_BAD_ARG;
    GemmArgs g[gn::GN_MAX_GROUP];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        if (!desc_ok(d[i])) return GN_ERR_BAD_ARG;
        if (d[i].M != 0) g[m++] = make_args(d[i]);
    }
    if (m == 0) return GN_OK;
    return gemm_launch(g, m, (hipStream_t)stream, split, form);
}

// the single-problem entries: a group of one (no K segments).  They refuse a bad act_kind even at M == 0, the group entries
// skip a problem without rows before looking at it (desc_ok): inherited from the first ABI and kept on purpose
int gemm_single(const float* A, int lda, const void* W, const float* bias, float* C, int ldc, int Mrows, int Nout, int K,
                int act_lo, int act_hi, int row_cnt, int row_gstride, int row_goff, const float* res, const float* gate,
                int gate_mode, float* pre_out, int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
                const float* a_gate, int ldg, int act_kind, void* stream, int split) {
    if (!act_kind_ok(act_kind) || (split && !W)) return GN_ERR_BAD_ARG;
    gn_gemm_desc d{};
    d.A = A; d.lda = lda; d.W = static_cast<const float*>(W); d.bias = bias; d.C = C; d.ldc = ldc;
    d.M = Mrows; d.N = Nout; d.K = K; d.act_lo = act_lo; d.act_hi = act_hi;
    d.row_cnt = row_cnt; d.row_gstride = row_gstride; d.row_goff = row_goff;
    d.res = res; d.gate = gate; d.gate_mode = gate_mode; d.pre_out = pre_out;
    d.pro_mode = pro_mode; d.pro_lo = pro_lo; d.pro_hi = pro_hi; d.a_pre = a_pre; d.ldp = ldp; d.a_gate = a_gate; d.ldg = ldg;
    d.act_kind = act_kind;
    return gemm_group_impl(&d, 1, stream, split);
}
}  // namespace

extern "C" int gn_gemm_group(const gn_gemm_desc* d, int n, void* stream) { return gemm_group_impl(d, n, stream, 0); }
// the same group on the 3 x bf16-split path: every desc.W points to the planes written by gn_split_bf16x3
extern "C" int gn_gemm_group_split(const gn_gemm_desc* d, int n, void* stream) { return gemm_group_impl(d, n, stream, 1); }
// ... and on the 2 x fp16-split path: every desc.W points to the buffer written by gn_split_f16x2
extern "C" int gn_gemm_group_f16x2(const gn_gemm_desc* d, int n, void* stream) { return gemm_group_impl(d, n, stream, 2); }
// ... on the slab kernel's 128-row tile the caller names, whatever the routing would choose (A/B probes and tests)
extern "C" int gn_gemm_group_f16x2_form(const gn_gemm_desc* d, int n, int form, void* stream) {
    if (form != GN_GEMM_FORM_BIG && form != GN_GEMM_FORM_BIG8) return GN_ERR_BAD_ARG;
    return gemm_group_impl(d, n, stream, 2, form);
}

extern "C" int gn_gemm_ex(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int Mrows, int Nout,
        int K, int act_lo, int act_hi, int row_cnt, int row_gstride, int row_goff, const float* res, const float* gate,
        int gate_mode, float* pre_out, int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
        const float* a_gate, int ldg, int act_kind, void* stream) {
    return gemm_single(A, lda, W, bias, C, ldc, Mrows, Nout, K, act_lo, act_hi, row_cnt, row_gstride, row_goff, res, gate,
                       gate_mode, pre_out, pro_mode, pro_lo, pro_hi, a_pre, ldp, a_gate, ldg, act_kind, stream, 0);
}

extern "C" int gn_gemm_split(const float* A, int lda, const unsigned short* W3, const float* bias, float* C, int ldc, int Mrows, int Nout,
        int K, int act_lo, int act_hi, int row_cnt, int row_gstride, int row_goff, const float* res, const float* gate,
        int gate_mode, float* pre_out, int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
        const float* a_gate, int ldg, int act_kind, void* stream) {
    return gemm_single(A, lda, W3, bias, C, ldc, Mrows, Nout, K, act_lo, act_hi, row_cnt, row_gstride, row_goff, res, gate,
                       gate_mode, pre_out, pro_mode, pro_lo, pro_hi, a_pre, ldp, a_gate, ldg, act_kind, stream, 1);
}

extern "C" int gn_gemm_f16x2(const float* A, int lda, const unsigned short* W2, const float* bias, float* C, int ldc, int Mrows, int Nout,
        int K, int act_lo, int act_hi, int row_cnt, int row_gstride, int row_goff, const float* res, const float* gate,
        int gate_mode, float* pre_out, int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
        const float* a_gate, int ldg, int act_kind, void* stream) {
    return gemm_single(A, lda, W2, bias, C, ldc, Mrows, Nout, K, act_lo, act_hi, row_cnt, row_gstride, row_goff, res, gate,
                       gate_mode, pre_out, pro_mode, pro_lo, pro_hi, a_pre, ldp, a_gate, ldg, act_kind, stream, 2);
}

extern "C" int gn_gemm(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int Mrows, int Nout,
        int K, int act_lo, int act_hi, int row_cnt, int row_gstride, int row_goff, const float* res, const float* gate,
        void* stream) {
    return gn_gemm_ex(A, lda, W, bias, C, ldc, Mrows, Nout, K, act_lo, act_hi, row_cnt, row_gstride, row_goff,
                      res, gate, 0, nullptr, 0, 0, 0, nullptr, 0, nullptr, 0, GN_ACT_SILU, stream);
}
