// gn_gata.hip -- the GATA interaction kernels: attention scores + segment softmax,
// the fused message / segmented-reduction / residual kernel (K6, the HBM-bound
// gather-scatter stage this library is measured on) and the HTR edge weights (K7).
//
// All three use the per-target "slot" layout (gn_common.h GN_SLOT_GEOMETRY): CSR rows by
// target, one workgroup per target atom, F/4 lanes per incoming edge with 16-byte
// loads, register accumulation, fixed-order LDS reduction across slots (gn_highl.h
// reduce_rows, no atomics).
// Workgroup -> target mapping is XCD-aware (gn::xcd_item) so the source rows of one
// molecule are re-read through a single XCD's L2.
#include "gn_common.h"
#include "gn_tune.h"
#include "gn_highl.h"
#include "gn_dropout.h"

namespace gn {

// ------------------------------------------------------------------ attention weights
// reference gotennet.py:497-511 + PyG softmax.  One workgroup per target.  The raw scores, their exponentials and the
// normalised weights of a target live in LDS (deg * H floats) and a[] is written ONCE, coalesced, at the end: the
// round-2 form kept them in the target's global a[] rows, i.e. four dependent global round trips (store scores ->
// barrier -> load / store exp -> load / store weights) per workgroup of a kernel that moves 55 MB -- 29 us at C2, 1.9 TB/s.
// Targets whose scores do not fit (deg * H > ATTN_CAP: a 256-neighbour atom at 8 heads still fits) take the global
// form; the choice is workgroup-uniform and made ONCE (a per-access select cost 31 -> 38 us in round 2), the
// arithmetic and its order are the same in both, so the two forms agree bit for bit.
// ASILU: activation fixed to SiLU at compile time (the run-time switch over twelve kinds costs registers and branches).
constexpr int ATTN_CAP = 2048;
#define GN_ATTN_ARGS                                                                                                    \
    const float *__restrict__ q, const float *__restrict__ k, int ldqk, const float *__restrict__ ta, int ldt,          \
        const int *__restrict__ rowptr, const int *__restrict__ src, const int *__restrict__ outdeg, int N, int F, int H, \
        float inv_sqrt_f, float *__restrict__ a, int act_rt
#define GN_ATTN_PASS q, k, ldqk, ta, ldt, rowptr, src, outdeg, N, F, H, inv_sqrt_f, a, act_rt

// the final write of weight w, element n = e * H + h: a[n] = w, or (DROP: training mode, gn_attn_softmax_dropout) the
// weight twice -- undropped to drop.a_soft, times the dropout multiplier to a[]
template <bool DROP>
__device__ __forceinline__ void attn_put(float* a, const AttnDrop& drop, unsigned long long key, size_t n, float w) {
    if constexpr (DROP) {
        drop.a_soft[n] = w;
        a[n] = w * drop_mult((unsigned)key, (unsigned)(key >> 32), drop.layer, drop.thresh, drop.scale, drop.all, n);
    } else {
        a[n] = w;
    }
}

// DROP: the global form keeps its scores in the a_soft rows.  A compile-time flag: the instantiations without it are
// the ones inference launches.
template <bool IN_LDS, bool ASILU, bool DROP>
__device__ __forceinline__ void attn_softmax_body(
    const float* __restrict__ q, const float* __restrict__ k, int ldqk, const float* __restrict__ ta, int ldt,
    const int* __restrict__ src, const int* __restrict__ outdeg, int i, int e0, int e1, int F, int H, float inv_sqrt_f,
    float* __restrict__ a, float* sc, int act, const AttnDrop drop) {
    unsigned long long dkey = 0;
    if constexpr (DROP) dkey = (unsigned long long)drop.key[0];
    const int lps = F >> 2, ns = 256 / lps;
    const int slot = threadIdx.x / lps, lp = threadIdx.x % lps, c0 = lp * 4;
    const int lph = lps / H;                       // lanes per head (power of two, >= 1)
    auto S = [&](int e, int h) -> float& {          // this target's score of edge e, head h
        if constexpr (IN_LDS) return sc[(e - e0) * H + h];
        else if constexpr (DROP) return drop.a_soft[(size_t)e * H + h];
        else return a[(size_t)e * H + h];
    };
    const float4 qi = ld4(q + (size_t)i * ldqk + c0);
    // two edges per trip: both index -> row load chains in flight together (a slot sees ~5 edges of a 20-neighbour atom)
    for (int e = e0 + slot; e < e1; e += 2 * ns) {
        const int eb = e + ns < e1 ? e + ns : e;
        const int ja = src[e], jb = src[eb];
        const float4 ka = ld4(k + (size_t)ja * ldqk + c0), kb = ld4(k + (size_t)jb * ldqk + c0);
        const float4 ta_ = act4(ld4_nt(ta + (size_t)e * ldt + c0), act);     // stored pre-activation: t_attn = act(.)
        const float4 tb_ = act4(ld4_nt(ta + (size_t)eb * ldt + c0), act);
        float pa = qi.x * ka.x * ta_.x;
        pa += qi.y * ka.y * ta_.y;
        pa += qi.z * ka.z * ta_.z;
        pa += qi.w * ka.w * ta_.w;
        float pb = qi.x * kb.x * tb_.x;
        pb += qi.y * kb.y * tb_.y;
        pb += qi.z * kb.z * tb_.z;
        pb += qi.w * kb.w * tb_.w;
        pa = group_sum(pa, lph);
        pb = group_sum(pb, lph);
        if ((lp & (lph - 1)) == 0) {
            S(e, lp / lph) = pa;
            if (eb != e) S(eb, lp / lph) = pb;
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int h = wave; h < H; h += 4) {
        float mx = -INFINITY;
        for (int e = e0 + lane; e < e1; e += 64) mx = fmaxf(mx, S(e, h));
        mx = wave_max(mx);
        float sm = 0.f;
        for (int e = e0 + lane; e < e1; e += 64) {
            const float ex = fast_exp(S(e, h) - mx);
            S(e, h) = ex;
            sm += ex;
        }
        const float rsm = __builtin_amdgcn_rcpf(wave_sum(sm) + 1e-16f);
        for (int e = e0 + lane; e < e1; e += 64) {
            const float nrm = outdeg ? sqrtf((float)outdeg[src[e]]) * inv_sqrt_f : inv_sqrt_f;
            const float w = S(e, h) * rsm * nrm;
            if constexpr (IN_LDS) S(e, h) = w;
            else attn_put<DROP>(a, drop, dkey, (size_t)e * H + h, w);
        }
    }
    if constexpr (IN_LDS) {
        __syncthreads();
        const int n = (e1 - e0) * H;
        for (int idx = threadIdx.x; idx < n; idx += 256) attn_put<DROP>(a, drop, dkey, (size_t)e0 * H + idx, sc[idx]);
    }
}

// the target of a workgroup and where its scores live; inference and dropout kernels differ in the AttnDrop argument alone
// (one kernel with the flag as a template parameter would hand the inference instantiations an argument they never read)
template <bool ASILU, bool DROP>
__device__ __forceinline__ void attn_softmax_target(GN_ATTN_ARGS, const AttnDrop& drop) {
    __shared__ float sc[ATTN_CAP];
    const int act = ASILU ? (int)GN_ACT_SILU : act_rt;
    const int i = xcd_item(blockIdx.x, N);
    if (i < 0) return;
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    if ((e1 - e0) * H <= ATTN_CAP)
        attn_softmax_body<true, ASILU, DROP>(q, k, ldqk, ta, ldt, src, outdeg, i, e0, e1, F, H, inv_sqrt_f, a, sc, act, drop);
    else
        attn_softmax_body<false, ASILU, DROP>(q, k, ldqk, ta, ldt, src, outdeg, i, e0, e1, F, H, inv_sqrt_f, a, sc, act, drop);
}
template <bool ASILU>
__global__ __launch_bounds__(256) GN_WPE(GN_W_ATTN) void attn_softmax_kernel(GN_ATTN_ARGS) {
    attn_softmax_target<ASILU, false>(GN_ATTN_PASS, AttnDrop{});
}
template <bool ASILU>
__global__ __launch_bounds__(256) void attn_softmax_drop_kernel(GN_ATTN_ARGS, const AttnDrop drop) {
    attn_softmax_target<ASILU, true>(GN_ATTN_PASS, drop);
}

// ---- one WAVE per target (F <= 256, H | 64): what ships for the default shapes.
// Round-3 counters on the workgroup-per-target kernel above (C2: 29 us for 55 MB): VALU-bound -- 1080 VALU instructions
// per wave, four waves per target, 20 % of the wave time issuing, the rest stalled on issue or parked at two barriers and
// 24 ds_bpermute round trips of the per-head reductions.  Here a target is ONE wave: its edges are walked 64 / (F / 4)
// at a time with the loads of eight steps in flight, the raw scores go to the wave's LDS strip, and the per-head max /
// sum run over the strip with (edge, head) = strip index per lane: the head of a lane is lane % H for every pass
// (H | 64), so the reductions are log2(64 / H) xor-shuffles, there is no barrier anywhere, and a[] is written once,
// coalesced.  Targets whose scores exceed the strip use their a[] rows as the strip (same code, same order).
constexpr int ATTN_W_STRIP = 512;                   // floats per wave: 64 incoming edges at 8 heads
// DROP: as in attn_softmax_body -- the global strip is the target's a_soft rows.
template <bool IN_LDS, bool ASILU, int FC, bool DROP>
__device__ __forceinline__ void attn_softmax_wave_body(
    const float* __restrict__ q, const float* __restrict__ k, int ldqk, const float* __restrict__ ta, int ldt,
    const int* __restrict__ src, const int* __restrict__ outdeg, int i, int e0, int e1, int F_rt, int H, float inv_sqrt_f,
    float* __restrict__ a, float* sc, int act, const AttnDrop drop) {
    const int F = FC ? FC : F_rt;                   // FC = 256: one edge per step, every index of the walk is wave-uniform
    const int lane = threadIdx.x & 63;
    const int lps = F >> 2, ns = 64 / lps;          // lanes per edge, edges per step
    const int slot = FC == 256 ? 0 : lane / lps, lp = lane % lps, c0 = lp * 4;
    const int lph = lps / H;                        // lanes per head
    float* const S = IN_LDS ? sc : (DROP ? drop.a_soft : a) + (size_t)e0 * H;   // strip: S[(e - e0) * H + h]
    const int n = (e1 - e0) * H;
    const float4 qi = ld4(q + (size_t)i * ldqk + c0);
    constexpr int U = 8;                            // steps per trip: U (index -> row) chains and U streamed rows in flight
    for (int eb = e0; eb < e1; eb += U * ns) {      // (a 20-neighbour target is three trips = three memory round trips)
        float4 kj[U], te[U];
        int ee[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = eb + u * ns + slot;
            ee[u] = e < e1 ? e : e1 - 1;            // clamped: a valid row, its score is not stored
            kj[u] = ld4(k + (size_t)src[ee[u]] * ldqk + c0);
            te[u] = ld4_nt(ta + (size_t)ee[u] * ldt + c0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 t4 = act4(te[u], act);     // stored pre-activation: t_attn = act(.)
            float p = qi.x * kj[u].x * t4.x;
            p += qi.y * kj[u].y * t4.y;
            p += qi.z * kj[u].z * t4.z;
            p += qi.w * kj[u].w * t4.w;
            p = group_sum(p, lph);
            if ((lp & (lph - 1)) == 0 && eb + u * ns + slot < e1) S[(ee[u] - e0) * H + lp / lph] = p;
        }
    }
    if constexpr (!IN_LDS) __builtin_amdgcn_s_waitcnt(0);         // the strip is this target's a[] rows: stores done before the loads
    __builtin_amdgcn_wave_barrier();
    // per-head max and sum over the strip; lane's head = lane % H in every pass
    float mx = -INFINITY;
    for (int idx = lane; idx < n; idx += 64) mx = fmaxf(mx, S[idx]);
    mx = stride_max(mx, H);
    float sm = 0.f;
    for (int idx = lane; idx < n; idx += 64) {
        const float ex = fast_exp(S[idx] - mx);
        S[idx] = ex;
        sm += ex;
    }
    sm = stride_sum(sm, H);
    const float rsm = __builtin_amdgcn_rcpf(sm + 1e-16f);
    if constexpr (!IN_LDS) __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    unsigned long long dkey = 0;
    if constexpr (DROP) dkey = (unsigned long long)drop.key[0];
    for (int idx = lane; idx < n; idx += 64) {
        const float nrm = outdeg ? sqrtf((float)outdeg[src[e0 + idx / H]]) * inv_sqrt_f : inv_sqrt_f;
        attn_put<DROP>(a, drop, dkey, (size_t)e0 * H + idx, S[idx] * rsm * nrm);
    }
}

// the wave's target (four consecutive targets per workgroup) and where its scores live
template <bool ASILU, int FC, bool DROP>
__device__ __forceinline__ void attn_softmax_wave_target(GN_ATTN_ARGS, const AttnDrop& drop) {
    __shared__ float strips[4 * ATTN_W_STRIP];
    const int act = ASILU ? (int)GN_ACT_SILU : act_rt;
    const int grp = xcd_item(blockIdx.x, (N + 3) >> 2);
    if (grp < 0) return;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = 4 * grp + wave;
    if (i >= N) return;
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    if (e1 == e0) return;
    float* sc = strips + wave * ATTN_W_STRIP;
    if ((e1 - e0) * H <= ATTN_W_STRIP)
        attn_softmax_wave_body<true, ASILU, FC, DROP>(q, k, ldqk, ta, ldt, src, outdeg, i, e0, e1, F, H, inv_sqrt_f, a, sc, act, drop);
    else
        attn_softmax_wave_body<false, ASILU, FC, DROP>(q, k, ldqk, ta, ldt, src, outdeg, i, e0, e1, F, H, inv_sqrt_f, a, sc, act, drop);
}
template <bool ASILU, int FC = 0>
__global__ __launch_bounds__(256) void attn_softmax_wave_kernel(GN_ATTN_ARGS) {
    attn_softmax_wave_target<ASILU, FC, false>(GN_ATTN_PASS, AttnDrop{});
}
template <bool ASILU>
__global__ __launch_bounds__(256) void attn_softmax_drop_wave_kernel(GN_ATTN_ARGS, const AttnDrop drop) {
    attn_softmax_wave_target<ASILU, 0, true>(GN_ATTN_PASS, drop);
}

// the [E,H] multipliers alone (what a test or a user needs to reproduce a step)
__global__ __launch_bounds__(256) void attn_dropout_mask_kernel(const long long* __restrict__ key, unsigned layer, unsigned thresh,
                                                                float scale, int all, unsigned long long n, float* __restrict__ m) {
    const unsigned long long k = (unsigned long long)key[0];
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (unsigned long long)gridDim.x * 256)
        m[idx] = drop_mult((unsigned)k, (unsigned)(k >> 32), layer, thresh, scale, all, idx);
}

// ------------------------------------------------------------------ K6 message + aggregate
// M F-wide blocks of the value vector: 0 = scalar; direction gate of degree l: block
// (SEP_DIR ? l : 1); tensor gate: block 1 + ND + (SEP_TENSOR ? l-1 : 0), ND = SEP_DIR ? LMAX : 1.
// The gate of a block, the lane's head in it and the residual-add rows are gn_highl.h's (msg_gate, block_head,
// add_h_row / add_X_row); the two kernels below keep their own edge loops, which are different schedules on purpose.
// The cross-slot sum is the loop of reduce_rows (gn_highl.h) with CH rows per pass, but it stays written out in both: as
// a call of reduce_rows with the writer as a [&] lambda, message_aggregate_kernel<4, true, true, true, 256> went from 150
// to 168 VGPRs with 2 spilled; with the writer as a struct held by value the registers stayed and every epilogue stored
// its 16-byte rows as 4 + 12 bytes.  Written out, all 44 instantiations keep their instruction streams.
#define GN_MSG_ARGS                                                                                         \
    const float *__restrict__ x, const float *__restrict__ v, int ldxv, const float *__restrict__ tf, int ldt,            \
        const float *__restrict__ a, const float *__restrict__ rl, const float *__restrict__ cut, const int *__restrict__ rowptr,    \
        const int *__restrict__ src, const float *__restrict__ h_in, const float *__restrict__ X_in,                     \
        float *__restrict__ h_out, float *__restrict__ X_out, int N, int F_rt, int H
#define GN_MSG_PASS x, v, ldxv, tf, ldt, a, rl, cut, rowptr, src, h_in, X_in, h_out, X_out, N, F_rt, H

// ---- every row in one launch: lmax <= 2, and the zero-X_in form at every lmax <= 4
// FIRST: X_in is identically zero (the first interaction of GotenNet.forward, gotennet.py:992): the tensor-gate blocks
// of t_filter / x / v and the X_in rows are not read (0 * gate contributes nothing) and X_out = the aggregated update.
// Same bits as the general kernel on a zero X_in.
template <int LMAX, bool SEP_DIR, bool SEP_TENSOR, bool FIRST = false, int FC = 0>
__global__ __launch_bounds__(256) GN_WPE(GN_W_K6) void message_aggregate_kernel(GN_MSG_ARGS) {
    constexpr int D = (LMAX + 1) * (LMAX + 1) - 1;
    constexpr int ND = SEP_DIR ? LMAX : 1;
    constexpr int NT = SEP_TENSOR ? LMAX : 1;
    constexpr int M = 1 + ND + NT;
    constexpr int ROWS = 1 + D;
    constexpr int CH = ROWS < 9 ? ROWS : 9;         // rows reduced per LDS pass (<= 36 KiB)
    __shared__ __attribute__((aligned(16))) float red[CH * 1024];

    const int F = FC ? FC : F_rt;
    const int i = xcd_item(blockIdx.x, N);
    if (i < 0) return;
    GN_SLOT_GEOMETRY(FC);
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    const int per_head = (M * F) / H;

    int hb[M];
#pragma unroll
    for (int b = 0; b < M; ++b) hb[b] = block_head(b, F, c0, per_head);

    float4 acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = zero4();

    for (int e = e0 + slot; e < e1; e += ns) {
        const int j = src[e];
        const float ce = cut[e];
        const float* xr = x + (size_t)j * ldxv + c0;
        const float* vr = v + (size_t)j * ldxv + c0;
        const float* tr = tf + (size_t)e * ldt + c0;
        const float* ar = a + (size_t)e * H;
        const float* Xj = X_in + (size_t)j * D * F + c0;
        const float* re = rl + (size_t)e * D;
        float4 o[M];
#pragma unroll
        for (int b = 0; b < (FIRST ? 1 + ND : M); ++b) o[b] = msg_gate(tr, xr, vr, ar, ce, b, F, hb[b]);
        acc[0] = acc[0] + o[0];
        int m = 0;
#pragma unroll
        for (int l = 1; l <= LMAX; ++l) {
            const float4 od = o[SEP_DIR ? l : 1];
#pragma unroll
            for (int mm = 0; mm < 2 * l + 1; ++mm, ++m) {
                // gotennet.py:538-558: rl * o_d + X_j * o_t
                if constexpr (FIRST)
                    acc[1 + m] = acc[1 + m] + od * re[m];
                else
                    acc[1 + m] = acc[1 + m] + fma4(ld4(Xj + (size_t)m * F), o[1 + ND + (SEP_TENSOR ? l - 1 : 0)], od * re[m]);
            }
        }
    }
    // fixed-order reduction over slots, CH rows per pass; slot s finishes rows s, s+ns, ... (reduce_rows, written out: see above)
#pragma unroll
    for (int base = 0; base < ROWS; base += CH) {
        if (base) __syncthreads();
#pragma unroll
        for (int r = 0; r < CH; ++r)
            if (base + r < ROWS) st4(&red[r * 1024 + slot * F + c0], acc[base + r]);
        __syncthreads();
        for (int r = slot; r < CH && base + r < ROWS; r += ns) {
            const float4 s = red4(red + r * 1024, c0, F, ns);
            const int row = base + r;
            if (row == 0) add_h_row(h_out, h_in, i, F, c0, s);
            else add_X_row<FIRST>(X_out, X_in, i, D, row - 1, F, c0, s);
        }
    }
}

// ---- lmax >= 3 with an X_in: degree groups
// One launch covers the degrees LLO..LHI (and the scalar row when SCALAR): the (1 + D) accumulator rows are cut into
// the groups {scalar,1,2}, {3} (lmax 3) or {3,4} (lmax 4) so that a launch keeps <= 9 float4 accumulators per lane
// (3+ waves/SIMD instead of 2 at 246 VGPRs), 16 in the {3,4} group.  Gates are per degree, so the groups re-read nothing
// but the per-edge scalars.
template <int LMAX, bool SEP_DIR, bool SEP_TENSOR, int LLO, int LHI, bool SCALAR, int FC>
__device__ __forceinline__ void message_aggregate_group_body(GN_MSG_ARGS) {
    constexpr int D = (LMAX + 1) * (LMAX + 1) - 1;
    constexpr int ND = SEP_DIR ? LMAX : 1;
    constexpr int NT = SEP_TENSOR ? LMAX : 1;
    constexpr int M = 1 + ND + NT;
    constexpr int XROWS = (LHI + 1) * (LHI + 1) - LLO * LLO;     // rows of degrees LLO..LHI
    constexpr int ROWS = (SCALAR ? 1 : 0) + XROWS;
    constexpr int M0 = LLO * LLO - 1;                             // first X row of the group
    constexpr int CH = ROWS < GN_K6G_CH ? ROWS : GN_K6G_CH;       // rows reduced per LDS pass (4 KiB each)
    __shared__ __attribute__((aligned(16))) float red[CH * 1024];

    const int F = FC ? FC : F_rt;
    const int i = xcd_item(blockIdx.x, N);
    if (i < 0) return;
    GN_SLOT_GEOMETRY(FC);
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    const int per_head = (M * F) / H;

    int hb[M];                                      // attention head of this lane's channels in block b
#pragma unroll
    for (int b = 0; b < M; ++b) hb[b] = block_head(b, F, c0, per_head);

    float4 acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = zero4();

    for (int e = e0 + slot; e < e1; e += ns) {
        const int j = src[e];
        const float ce = cut[e];
        const float* xr = x + (size_t)j * ldxv + c0;
        const float* vr = v + (size_t)j * ldxv + c0;
        const float* tr = tf + (size_t)e * ldt + c0;
        const float* ar = a + (size_t)e * H;
        const float* Xj = X_in + (size_t)j * D * F + c0;
        const float* re = rl + (size_t)e * D;
        auto gate = [&](int b) { return msg_gate(tr, xr, vr, ar, ce, b, F, hb[b]); };
        // all gate loads first (independent, issued back to back), then the X_j rows
        constexpr int NL = LHI - LLO + 1;
        float4 gd[NL], gt[NL];
#pragma unroll
        for (int l = LLO; l <= LHI; ++l) {
            gd[l - LLO] = (SEP_DIR || l == LLO) ? gate(SEP_DIR ? l : 1) : gd[0];
            gt[l - LLO] = (SEP_TENSOR || l == LLO) ? gate(1 + ND + (SEP_TENSOR ? l - 1 : 0)) : gt[0];
        }
        if (SCALAR) acc[0] = acc[0] + gate(0);
#pragma unroll
        for (int l = LLO; l <= LHI; ++l) {
#pragma unroll
            for (int mm = 0; mm < 2 * l + 1; ++mm) {
                const int m = l * l - 1 + mm;
                // gotennet.py:538-558: rl * o_d + X_j * o_t
                acc[(SCALAR ? 1 : 0) + m - M0] = acc[(SCALAR ? 1 : 0) + m - M0] +
                                                 fma4(ld4(Xj + (size_t)m * F), gt[l - LLO], gd[l - LLO] * re[m]);
            }
        }
    }
    // fixed-order reduction over slots, CH rows per pass; slot s finishes rows s, s+ns, ... (reduce_rows, written out: see above)
#pragma unroll
    for (int base = 0; base < ROWS; base += CH) {
        if (base) __syncthreads();
#pragma unroll
        for (int r = 0; r < CH; ++r)
            if (base + r < ROWS) st4(&red[r * 1024 + slot * F + c0], acc[base + r]);
        __syncthreads();
        for (int r = slot; r < CH && base + r < ROWS; r += ns) {
            const float4 s = red4(red + r * 1024, c0, F, ns);
            const int row = base + r;
            if (SCALAR && row == 0) add_h_row(h_out, h_in, i, F, c0, s);
            else add_X_row(X_out, X_in, i, D, M0 + row - (SCALAR ? 1 : 0), F, c0, s);
        }
    }
}

// one degree group per launch; the two-degree group {3,4} (16 accumulator rows) gets its own occupancy target
template <int LMAX, bool SEP_DIR, bool SEP_TENSOR, int LLO, int LHI, bool SCALAR, int FC = 0>
__global__ __launch_bounds__(256) GN_WPE(GN_W_K6_G) void message_aggregate_group_kernel(GN_MSG_ARGS) {
    message_aggregate_group_body<LMAX, SEP_DIR, SEP_TENSOR, LLO, LHI, SCALAR, FC>(GN_MSG_PASS);
}
template <int LMAX, bool SEP_DIR, bool SEP_TENSOR, int LLO, int LHI, bool SCALAR, int FC = 0>
__global__ __launch_bounds__(256) GN_WPE(GN_W_K6_G34) void message_aggregate_group34_kernel(GN_MSG_ARGS) {
    message_aggregate_group_body<LMAX, SEP_DIR, SEP_TENSOR, LLO, LHI, SCALAR, FC>(GN_MSG_PASS);
}

// ------------------------------------------------------------------ K7 HTR edge weights
// gotennet.py:351-364, 580-609 (sep_htr, rejection on).  LMAX <= 2: the literal two-rejection form
//   w_l = sum_m (EQ - (EQ.r) r)_m (EK - (EK.r) r)_m.
// LMAX >= 3: the algebraically equal closed form of gn_highl.h (HtrBlock) -- 3 instead of 5 float4 FMAs per row and no
// second pass over the rows; its rounding differs from the literal form at the 1e-7 level.  Measured (round 4, in the
// step):
//   lmax 3 (C5), degree by degree: 98.0 -> 90.5 us against the literal form (126 VGPRs, 4 waves/SIMD instead of 132 / 3);
//     with every row requested first 92.4 us.
//   lmax 4: degree by degree the closed form LOSES, 105.9 -> 140.4 us at the same 2 waves/SIMD (the literal form keeps all
//     24 row loads of an edge in flight, the compiler serialises the closed form's); with every row of the edge requested
//     before the first use (a sched_barrier keeps the loads together) 108.4 -> 90 us.
// Both were switches once (closed form on / off, and the lmax from which all rows go first); the losing sides are gone.
template <int LMAX, int FC = 0>
__global__ __launch_bounds__(256) GN_WPE(GN_W_HTR_EDGE) void htr_edge_kernel(
    const float* __restrict__ EQ, const float* __restrict__ EK, const float* __restrict__ rl,
    const int* __restrict__ rowptr, const int* __restrict__ src, int N, int F_rt, float* __restrict__ w) {
    constexpr int D = (LMAX + 1) * (LMAX + 1) - 1;
    const int F = FC ? FC : F_rt;
    const int i = xcd_item(blockIdx.x, N);
    if (i < 0) return;
    GN_SLOT_GEOMETRY(FC);
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    float4 eq[D];
#pragma unroll
    for (int m = 0; m < D; ++m) eq[m] = ld4(EQ + ((size_t)i * D + m) * F + c0);
    for (int e = e0 + slot; e < e1; e += ns) {
        const float* kj = EK + (size_t)src[e] * D * F + c0;
        const float* re = rl + (size_t)e * D;
        float4 wsum = zero4();
        if constexpr (LMAX >= 4) {                  // closed form, every row of the edge first
            float4 eka[D];
            float ra[D];
#pragma unroll
            for (int m = 0; m < D; ++m) { eka[m] = ld4(kj + (size_t)m * F); ra[m] = re[m]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int l = 1; l <= LMAX; ++l) {
                // HtrBlock (gn_highl.h) written out: through the struct this kernel alone compiled to other code (443 -> 441 instructions)
                float4 pq = zero4(), pk = zero4(), ab = zero4();
                float rr = 0.f;
#pragma unroll
                for (int mm = 0; mm < 2 * l + 1; ++mm) {
                    const int m = l * l - 1 + mm;
                    rr = fmaf(ra[m], ra[m], rr);
                    pq = fma4(ra[m], eq[m], pq);
                    pk = fma4(ra[m], eka[m], pk);
                    ab = fma4(eq[m], eka[m], ab);
                }
                wsum = wsum + (ab + (pq * pk) * (rr - 2.0f));
            }
        } else {
            int m0 = 0;
#pragma unroll
            for (int l = 1; l <= LMAX; ++l) {
                float4 ek[2 * LMAX + 1];
                float r[2 * LMAX + 1];
                if constexpr (LMAX == 3) {          // closed form, degree by degree
                    HtrBlock blk;
#pragma unroll
                    for (int mm = 0; mm < 2 * l + 1; ++mm) {
                        ek[mm] = ld4(kj + (size_t)(m0 + mm) * F);
                        r[mm] = re[m0 + mm];
                    }
#pragma unroll
                    for (int mm = 0; mm < 2 * l + 1; ++mm) blk.row(r[mm], eq[m0 + mm], ek[mm]);
                    wsum = wsum + blk.w();
                } else {                            // literal form
                    float4 pq = zero4(), pk = zero4();
#pragma unroll
                    for (int mm = 0; mm < 2 * l + 1; ++mm) {
                        ek[mm] = ld4(kj + (size_t)(m0 + mm) * F);
                        r[mm] = re[m0 + mm];
                        pq = fma4(r[mm], eq[m0 + mm], pq);
                        pk = fma4(-r[mm], ek[mm], pk);
                    }
#pragma unroll
                    for (int mm = 0; mm < 2 * l + 1; ++mm) {
                        const float4 a_ = eq[m0 + mm] + pq * (-r[mm]);       // EQ - proj * rl
                        const float4 b_ = ek[mm] + pk * r[mm];               // EK - proj' * (-rl)
                        wsum = fma4(a_, b_, wsum);
                    }
                }
                m0 += 2 * l + 1;
            }
        }
        st4_nt(w + (size_t)e * F + c0, wsum);
    }
}

}  // namespace gn

// ====================================================================================== C ABI
static bool feature_dim_ok(int F) { return F >= 16 && F <= 1024 && gn::is_pow2(F); }

// p -> (threshold, multiplier, "drops everything"); false for a p that is no probability
static bool drop_params(double p, unsigned& thresh, float& scale, int& all) {
    if (!(p >= 0.0)) return false;
    all = p >= 1.0 ? 1 : 0;
    thresh = all ? 0xffffffffu : (unsigned)floor(p * 4294967296.0);
    scale = all ? 0.f : (float)(1.0 / (1.0 - p));
    return true;
}

// argument check and choice of form for gn_attn_softmax (drop == NULL) and gn_attn_softmax_dropout
static int attn_softmax_launch(const float* q, const float* k, int ldqk, const float* t_attn, int ldt, const int* rowptr,
                               const int* src, const int* outdeg, int N, int F, int H, float* a, int act,
                               const gn::AttnDrop* drop, hipStream_t st) {
    if (!feature_dim_ok(F) || N < 0 || H <= 0 || !gn::is_pow2(H) || (F / 4) % H || (F / 4) / H > 64 ||
        (ldqk & 3) || (ldt & 3) || act < 0 || act >= GN_ACT_COUNT)
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    const float inv_sqrt_f = (float)(1.0 / sqrt((double)F));
    // one wave per target where a wave covers an edge row and the strip's head-per-lane map holds (-DGN_ATTN_WAVE=0
    // builds the workgroup-per-target kernel only, for an A/B: tools/variants.py)
    const bool wave = GN_ATTN_WAVE && F <= 256 && H <= 64, silu = act == GN_ACT_SILU;
    const dim3 grid(gn::xcd_grid(wave ? (N + 3) / 4 : N));
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, q, k, ldqk, t_attn, ldt, rowptr, src, outdeg, N, F, H, inv_sqrt_f, a,
                           act, extra...);
    };
    if (wave && drop) silu ? launch(gn::attn_softmax_drop_wave_kernel<true>, *drop) : launch(gn::attn_softmax_drop_wave_kernel<false>, *drop);
    else if (wave && silu && F == 256) launch(gn::attn_softmax_wave_kernel<true, 256>);   // width as a compile-time constant, inference only
    else if (wave) silu ? launch(gn::attn_softmax_wave_kernel<true>) : launch(gn::attn_softmax_wave_kernel<false>);
    else if (drop) silu ? launch(gn::attn_softmax_drop_kernel<true>, *drop) : launch(gn::attn_softmax_drop_kernel<false>, *drop);
    else silu ? launch(gn::attn_softmax_kernel<true>) : launch(gn::attn_softmax_kernel<false>);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_attn_softmax(const float* q, const float* k, int ldqk, const float* t_attn, int ldt,
                               const int* rowptr, const int* src, const int* outdeg,
                               int N, int F, int H, float* a, int act, void* stream) {
    return attn_softmax_launch(q, k, ldqk, t_attn, ldt, rowptr, src, outdeg, N, F, H, a, act, nullptr, (hipStream_t)stream);
}

extern "C" int gn_attn_softmax_dropout(const float* q, const float* k, int ldqk, const float* t_attn, int ldt,
                                       const int* rowptr, const int* src, const int* outdeg,
                                       int N, int F, int H, float* a_soft, float* a, const long long* key, int layer, double p,
                                       int act, void* stream) {
    gn::AttnDrop d{a_soft, key, (unsigned)layer, 0u, 0.f, 0};
    if (!key || !a_soft || a_soft == a || layer < 0 || !drop_params(p, d.thresh, d.scale, d.all)) return GN_ERR_BAD_ARG;
    return attn_softmax_launch(q, k, ldqk, t_attn, ldt, rowptr, src, outdeg, N, F, H, a, act, &d, (hipStream_t)stream);
}

extern "C" int gn_attn_dropout_mask(const long long* key, int layer, double p, long E, int H, float* m_out, void* stream) {
    unsigned thresh; float scale; int all;
    if (!key || layer < 0 || E < 0 || H <= 0 || !drop_params(p, thresh, scale, all)) return GN_ERR_BAD_ARG;
    const unsigned long long n = (unsigned long long)E * (unsigned long long)H;
    if (n == 0) return GN_OK;
    const unsigned long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(gn::attn_dropout_mask_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                       (hipStream_t)stream, key, (unsigned)layer, thresh, scale, all, n, m_out);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

struct MsgFwdArgs {                                 // the kernels' arguments, in their order
    const float *x, *v; int ldxv; const float* t_filter; int ldt; const float *a, *rl, *cut; const int *rowptr, *src;
    const float *h_in, *X_in; float *h_out, *X_out; int N, F, H;
};
template <typename Kernel>
static void message_launch_one(Kernel kernel, const MsgFwdArgs& p, hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3(gn::xcd_grid(p.N)), dim3(256), 0, st, p.x, p.v, p.ldxv, p.t_filter, p.ldt, p.a, p.rl, p.cut,
                       p.rowptr, p.src, p.h_in, p.X_in, p.h_out, p.X_out, p.N, p.F, p.H);
}
// One (lmax, sep_dir, sep_tensor) shape; only the forms that are launched are instantiated.  A zero X_in (NULL) is one
// launch at every lmax: 1 + D rows of rl * o_d only.  Otherwise lmax <= 2 is one launch and lmax >= 3 the degree groups
// {scalar,1,2} + {3} / {3,4}.  Degrees 3 and 4 of lmax 4 in ONE launch (16 accumulator rows, 2 waves/SIMD), against a
// launch each: C2 message stage 245.9 -> ~235 us (two launches: 60 + 64 us for 111 MB of t_filter each); it was a switch
// once, the separate {3}, {4} launches are gone.
template <int L, bool SD, bool ST, int FC>
static void message_launch(const MsgFwdArgs& p, hipStream_t st) {
    if (!p.X_in) {
        message_launch_one(gn::message_aggregate_kernel<L, SD, ST, true, FC>, p, st);
    } else if constexpr (L <= 2) {
        message_launch_one(gn::message_aggregate_kernel<L, SD, ST, false, FC>, p, st);
    } else {
        message_launch_one(gn::message_aggregate_group_kernel<L, SD, ST, 1, 2, true, FC>, p, st);
        if constexpr (L == 3) message_launch_one(gn::message_aggregate_group_kernel<L, SD, ST, 3, 3, false, FC>, p, st);
        else message_launch_one(gn::message_aggregate_group34_kernel<L, SD, ST, 3, 4, false, FC>, p, st);
    }
}
// FC = 256: the compile-time-width instantiations, at lmax 1 and for the reference's defaults (sep_dir, sep_tensor) only
template <int FC>
static void message_aggregate_launch(const MsgFwdArgs& p, int lmax, int sep_dir, int sep_tensor, hipStream_t st) {
    switch (lmax * 4 + (sep_dir ? 2 : 0) + (sep_tensor ? 1 : 0)) {
        case 4: case 5: case 6: case 7: message_launch<1, false, false, FC>(p, st); break;   // lmax = 1: flags are no-ops
        case 8: message_launch<2, false, false, 0>(p, st); break;
        case 9: message_launch<2, false, true, 0>(p, st); break;
        case 10: message_launch<2, true, false, 0>(p, st); break;
        case 11: message_launch<2, true, true, FC>(p, st); break;
        case 12: message_launch<3, false, false, 0>(p, st); break;
        case 13: message_launch<3, false, true, 0>(p, st); break;
        case 14: message_launch<3, true, false, 0>(p, st); break;
        case 15: message_launch<3, true, true, FC>(p, st); break;
        case 16: message_launch<4, false, false, 0>(p, st); break;
        case 17: message_launch<4, false, true, 0>(p, st); break;
        case 18: message_launch<4, true, false, 0>(p, st); break;
        default: message_launch<4, true, true, FC>(p, st); break;
    }
}

extern "C" int gn_message_aggregate(const float* x, const float* v, int ldxv, const float* t_filter, int ldt,
                                    const float* a, const float* rl, const float* cut,
                                    const int* rowptr, const int* src,
                                    const float* h_in, const float* X_in, float* h_out, float* X_out,
                                    int N, int F, int H, int lmax_arg, int sep_dir, int sep_tensor, void* stream) {
    const int lmax = lmax_arg & 0xff;               // GN_LMAX_SLICED / _MEAN / _MAX may ride in the argument (gn_use_highl)
    const int aggr = (lmax_arg & GN_LMAX_MEAN) ? 1 : ((lmax_arg & GN_LMAX_MAX) ? 2 : 0);
    if ((lmax_arg & ~(0xff | GN_LMAX_SLICED | GN_LMAX_MEAN | GN_LMAX_MAX)) ||
        ((lmax_arg & GN_LMAX_MEAN) && (lmax_arg & GN_LMAX_MAX)) || !feature_dim_ok(F) || N < 0 || H <= 0 || lmax < 1 ||
        lmax > 8 || (ldxv & 3) || (ldt & 3) || X_in == X_out)
        return GN_ERR_BAD_ARG;
    if (!X_in && gn_use_highl(lmax_arg)) return GN_ERR_BAD_ARG;   // the zero-X_in form: register-tiled kernels only (lmax <= 4)
    const int M = 1 + (sep_dir ? lmax : 1) + (sep_tensor ? lmax : 1);
    if ((M * F) % H || ((M * F) / H) % 4) return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    if (gn_use_highl(lmax_arg))                        // degrees 5..8: one launch per degree (gn_highl.hip)
        return gn_highl_message(x, v, ldxv, t_filter, ldt, a, rl, cut, rowptr, src, h_in, X_in, h_out, X_out, N, F, H,
                                lmax, sep_dir, sep_tensor, aggr, (hipStream_t)stream);
    const MsgFwdArgs p{x, v, ldxv, t_filter, ldt, a, rl, cut, rowptr, src, h_in, X_in, h_out, X_out, N, F, H};
    if (F == 256) message_aggregate_launch<256>(p, lmax, sep_dir, sep_tensor, (hipStream_t)stream);
    else message_aggregate_launch<0>(p, lmax, sep_dir, sep_tensor, (hipStream_t)stream);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

template <int FC>
static void htr_edge_launch(const float* EQ, const float* EK, const float* rl, const int* rowptr, const int* src, int N, int F,
                            int lmax, float* w, hipStream_t st) {
    const dim3 grid(gn::xcd_grid(N)), block(256);
    switch (lmax) {
        case 1: hipLaunchKernelGGL((gn::htr_edge_kernel<1, FC>), grid, block, 0, st, EQ, EK, rl, rowptr, src, N, F, w); break;
        case 2: hipLaunchKernelGGL((gn::htr_edge_kernel<2, FC>), grid, block, 0, st, EQ, EK, rl, rowptr, src, N, F, w); break;
        case 3: hipLaunchKernelGGL((gn::htr_edge_kernel<3, FC>), grid, block, 0, st, EQ, EK, rl, rowptr, src, N, F, w); break;
        default: hipLaunchKernelGGL((gn::htr_edge_kernel<4, FC>), grid, block, 0, st, EQ, EK, rl, rowptr, src, N, F, w); break;
    }
}

extern "C" int gn_htr_edge(const float* EQ, const float* EK, const float* rl, const int* rowptr, const int* src,
                           int N, int F, int lmax_arg, int mode, float* w_raw, float* w, void* stream) {
    const int lmax = lmax_arg & 0xff;
    if ((lmax_arg & ~(0xff | GN_LMAX_SLICED)) || !feature_dim_ok(F) || N < 0 || lmax < 1 || lmax > 8 || mode < 0 || mode > 15)
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (gn_use_highl(lmax_arg)) return gn_highl_htr_edge(EQ, EK, rl, rowptr, src, N, F, lmax, mode, w_raw, w, st);
    if (mode) return gn_htr_edge_general(EQ, EK, rl, rowptr, src, N, F, lmax, mode, w_raw, w, st);
    if (F == 256) htr_edge_launch<256>(EQ, EK, rl, rowptr, src, N, F, lmax, w, st);
    else htr_edge_launch<0>(EQ, EK, rl, rowptr, src, N, F, lmax, w, st);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
