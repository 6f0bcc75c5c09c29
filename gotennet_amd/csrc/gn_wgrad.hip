// gn_wgrad.hip -- parameter gradients of the Dense products, the embeddings and the LayerNorm affines (first-order
// training).  Every reduction runs in a fixed order with no atomics: identical inputs give identical
// bits.
#include <algorithm>

#include "gn_common.h"

namespace gn {

// ---------------------------------------------------------------------------------- weight gradients
// dW[n, k] = sum_r dY[r, y_off + n] A[r, a_off + k] on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulation).  The
// reduction axis is the ROW axis of both operands: lane l of the MFMA's A operand holds dY[r0 + (l>>5)][n0 + (l&31)],
// lane l of its B operand A[r0 + (l>>5)][k0 + (l&31)] -- both plain row reads of row-major tiles staged through LDS.
// Workgroup tile: 64 outputs x 64 inputs (four waves, 32 x 32 each), WG_ROWS rows per LDS stage.  The rows are split into
// S contiguous ranges (split-K over rows; S from the problem shape alone): each split writes its partial tile to the
// workspace, and wgrad_reduce_kernel sums the splits in the order s = 0..S-1.
constexpr int WG_T = 64;          // output tile edge (nout and K)
constexpr int WG_ROWS = 32;       // rows per LDS stage
constexpr int WG_LDS = WG_T + 32; // padded LDS row: lanes l and l + 32 read rows r and r + 1 in different banks
constexpr int WG_MAXP = 8;        // problems per launch
typedef float wg_f32x16 __attribute__((ext_vector_type(16)));

struct WgradProb {
    const float* dY; const float* A; float* dW; float* db;
    float* part;                  // [S][nout * K + nout] partial sums (workspace)
    int ldy, y_off, lda, a_off, ldw;
    int rows, nout, K;
    int cnt, gstride, goff;
    int S, rows_per_split, tiles_n, tiles_k;
    int blk0;                     // first block of this problem in the launch
    long red0;                    // first element of this problem in the reduction launch
};
struct WgradArgs {
    WgradProb p[WG_MAXP];
    int n;
};

__device__ __forceinline__ long wg_row(const WgradProb& p, int r) {
    return p.cnt == 1 ? (long)r * p.gstride + p.goff : (long)(r / p.cnt) * p.gstride + p.goff + r % p.cnt;
}

__global__ __launch_bounds__(256) void wgrad_partial_kernel(const WgradArgs args) {
    __shared__ float sY[WG_ROWS][WG_LDS];
    __shared__ float sA[WG_ROWS][WG_LDS];
    int pi = 0;
    while (pi + 1 < args.n && (int)blockIdx.x >= args.p[pi + 1].blk0) ++pi;
    const WgradProb& p = args.p[pi];
    const int b = blockIdx.x - p.blk0;
    const int tiles = p.tiles_n * p.tiles_k;
    const int s = b / tiles, tile = b % tiles;
    const int n0 = (tile / p.tiles_k) * WG_T, k0 = (tile % p.tiles_k) * WG_T;
    const int r_begin = min(p.rows, s * p.rows_per_split), r_end = min(p.rows, r_begin + p.rows_per_split);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave & 1, wk = wave >> 1;
    const int col = tid & 63, rsub = tid >> 6;         // staging: 4 rows x 64 columns per pass, 8 passes
    const bool ny = n0 + col < p.nout, ka = k0 + col < p.K;
    const bool bias = p.db != nullptr && wk == 0 && (tile % p.tiles_k) == 0;   // waves 0/1 of a k0 = 0 tile keep sum_r dY
    wg_f32x16 acc = {};
    float bsum = 0.f;
    float ry[8], ra[8];
    auto load = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = r0 + rsub + 4 * i;
            const bool in = r < r_end;
            const long pr = in ? wg_row(p, r) : 0;
            ry[i] = (in && ny) ? p.dY[pr * p.ldy + p.y_off + n0 + col] : 0.f;
            ra[i] = (in && ka) ? p.A[pr * p.lda + p.a_off + k0 + col] : 0.f;
        }
    };
    if (r_begin < r_end) load(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += WG_ROWS) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sY[rsub + 4 * i][col] = ry[i];
            sA[rsub + 4 * i][col] = ra[i];
        }
        __syncthreads();
        if (r0 + WG_ROWS < r_end) load(r0 + WG_ROWS);  // next stage's global reads overlap this stage's MFMAs
#pragma unroll
        for (int kk = 0; kk < WG_ROWS / 2; ++kk) {
            const float a = sY[2 * kk + (lane >> 5)][wn * 32 + (lane & 31)];
            const float bb = sA[2 * kk + (lane >> 5)][wk * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
        }
        if (bias && lane < 32) {
            for (int r = 0; r < WG_ROWS; ++r) bsum += sY[r][wn * 32 + lane];
        }
        __syncthreads();
    }
    // C/D map of the 32x32 MFMA: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* part = p.part + (long)s * ((long)p.nout * p.K + p.nout);
    const int kc = k0 + wk * 32 + (lane & 31);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + wn * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (n < p.nout && kc < p.K) part[(long)n * p.K + kc] = acc[reg];
    }
    if (bias && lane < 32 && n0 + wn * 32 + lane < p.nout)
        part[(long)p.nout * p.K + n0 + wn * 32 + lane] = bsum;
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WgradArgs args, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int pi = 0;
    while (pi + 1 < args.n && i >= args.p[pi + 1].red0) ++pi;
    const WgradProb& p = args.p[pi];
    const long j = i - p.red0, nk = (long)p.nout * p.K, stride = nk + p.nout;
    if (j >= nk && p.db == nullptr) return;
    float v = 0.f;
    for (int s = 0; s < p.S; ++s) v += p.part[(long)s * stride + j];
    if (j < nk) p.dW[(j / p.K) * p.ldw + j % p.K] = v;
    else p.db[j - nk] = v;
}

// the split of the rows: at least 512 rows per split, and about 1024 workgroups for the problem
static void wgrad_shape(const gn_wgrad_desc& d, int& S, int& rps, int& tn, int& tk) {
    tn = (d.nout + WG_T - 1) / WG_T;
    tk = (d.K + WG_T - 1) / WG_T;
    const int want = std::max(1, 1024 / (tn * tk));
    S = std::max(1, std::min(want, (d.rows + 511) / 512));
    rps = ((d.rows + S - 1) / S + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
    if (rps == 0) rps = WG_ROWS;
    S = std::max(1, (d.rows + rps - 1) / rps);
}

static long wgrad_floats(const gn_wgrad_desc& d) {
    int S, rps, tn, tk;
    wgrad_shape(d, S, rps, tn, tk);
    return (long)S * ((long)d.nout * d.K + d.nout);
}

// ---------------------------------------------------------------------------------- embeddings
// P[j, c] = sum over the by-source entries of j (stable order), self-loops skipped: g_ctx[i, F + c] feat[e, c] cut[e]
__global__ __launch_bounds__(256) void emb_source_kernel(
    const float* __restrict__ g_ctx, const float* __restrict__ feat, int ldf, const float* __restrict__ cut,
    const int* __restrict__ dst, const int* __restrict__ colptr, const int* __restrict__ perm, int N, int F,
    float* __restrict__ P) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * F) return;
    const int j = (int)(t / F), c = (int)(t % F);
    float acc = 0.f;
    for (int q = colptr[j]; q < colptr[j + 1]; ++q) {
        const int e = perm[q], i = dst[e];
        if (i == j) continue;
        acc = fmaf(g_ctx[(long)i * 2 * F + F + c], feat[(long)e * ldf + c] * cut[e], acc);
    }
    P[t] = acc;
}

// out[s, c] = sum over the atoms of species s (order[sp_ptr[s] .. sp_ptr[s+1]), ascending atom index) of X[atom, c]
__global__ __launch_bounds__(256) void emb_species_kernel(
    const float* __restrict__ X, int ldx, const int* __restrict__ order, const int* __restrict__ sp_ptr,
    int n_species, int F, int zero_row0, float* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n_species * F) return;
    const int sp = (int)(t / F), c = (int)(t % F);
    float acc = 0.f;
    if (!(zero_row0 && sp == 0))
        for (int q = sp_ptr[sp]; q < sp_ptr[sp + 1]; ++q) acc += X[(long)order[q] * ldx + c];
    out[t] = acc;
}

// ---------------------------------------------------------------------------------- LayerNorm affine
constexpr int LN_ROWS = 64;       // rows per partial

// per chunk of LN_ROWS rows: dgamma_part[c] = sum_r g_z x_hat, dbeta_part[c] = sum_r g_z, g_z = g_out act'(x_hat gamma + beta)
__global__ __launch_bounds__(256) void ln_param_partial_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    const float* __restrict__ gout, int N, int C, int act, float* __restrict__ part) {
    __shared__ float mu[LN_ROWS], rs[LN_ROWS];
    const int r0 = blockIdx.x * LN_ROWS, nr = min(LN_ROWS, N - r0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int rr = wave; rr < nr; rr += 4) {        // row statistics: one wave per row, two passes
        const float* xr = x + (long)(r0 + rr) * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        const float m = s / C;
        float v = 0.f;
        for (int c = lane; c < C; c += 64) { const float d = xr[c] - m; v += d * d; }
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) { mu[rr] = m; rs[rr] = 1.0f / sqrtf(v / C + eps); }
    }
    __syncthreads();
    const int nch = (N + LN_ROWS - 1) / LN_ROWS;
    for (int c = threadIdx.x; c < C; c += 256) {
        float dg = 0.f, db = 0.f;
        for (int rr = 0; rr < nr; ++rr) {
            const long o = (long)(r0 + rr) * C + c;
            const float xh = (x[o] - mu[rr]) * rs[rr];
            float g = gout[o];
            if (act != GN_ACT_NONE) g *= act == GN_ACT_SILU ? dsilu(xh * gamma[c] + beta[c]) : dact_generic(xh * gamma[c] + beta[c], act);
            dg = fmaf(g, xh, dg);
            db += g;
        }
        part[(long)blockIdx.x * C + c] = dg;
        part[((long)nch + blockIdx.x) * C + c] = db;
    }
}

__global__ __launch_bounds__(256) void ln_param_reduce_kernel(const float* __restrict__ part, int nch, int C,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float dg = 0.f, db = 0.f;
    for (int k = 0; k < nch; ++k) {
        dg += part[(long)k * C + c];
        db += part[((long)nch + k) * C + c];
    }
    dgamma[c] = dg;
    if (dbeta) dbeta[c] = db;
}

}  // namespace gn

extern "C" long gn_weight_grad_workspace(const gn_wgrad_desc* d, int n) {
    long total = 0;
    for (int i = 0; i < n; ++i) total += gn::wgrad_floats(d[i]);
    return total;
}

extern "C" int gn_weight_grad_group(const gn_wgrad_desc* d, int n, float* work, long work_floats, void* stream) {
    if (n < 0 || (n > 0 && (d == nullptr || work == nullptr))) return GN_ERR_BAD_ARG;
    if (gn_weight_grad_workspace(d, n) > work_floats) return GN_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i) {
        const gn_wgrad_desc& q = d[i];
        if (q.rows < 0 || q.nout < 1 || q.K < 1 || q.row_cnt < 1 || q.dW == nullptr || q.ldw < q.K ||
            (q.rows > 0 && (q.dY == nullptr || q.A == nullptr)))
            return GN_ERR_BAD_ARG;
    }
    float* wp = work;
    for (int i0 = 0; i0 < n; i0 += gn::WG_MAXP) {
        gn::WgradArgs ga;
        ga.n = std::min(gn::WG_MAXP, n - i0);
        int blocks = 0;
        long red = 0;
        for (int j = 0; j < ga.n; ++j) {
            const gn_wgrad_desc& q = d[i0 + j];
            gn::WgradProb& p = ga.p[j];
            gn::wgrad_shape(q, p.S, p.rows_per_split, p.tiles_n, p.tiles_k);
            p.dY = q.dY; p.A = q.A; p.dW = q.dW; p.db = q.db; p.part = wp;
            p.ldy = q.ldy; p.y_off = q.y_off; p.lda = q.lda; p.a_off = q.a_off; p.ldw = q.ldw;
            p.rows = q.rows; p.nout = q.nout; p.K = q.K;
            p.cnt = q.row_cnt; p.gstride = q.row_gstride; p.goff = q.row_goff;
            p.blk0 = blocks;
            p.red0 = red;
            blocks += p.S * p.tiles_n * p.tiles_k;
            red += (long)q.nout * q.K + q.nout;
            wp += gn::wgrad_floats(q);
        }
        hipLaunchKernelGGL(gn::wgrad_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ga);
        GN_LAUNCH_CHECK();
        hipLaunchKernelGGL(gn::wgrad_reduce_kernel, dim3((unsigned)((red + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           ga, red);
        GN_LAUNCH_CHECK();
    }
    return GN_OK;
}

extern "C" int gn_embedding_grad(const float* g_ctx, const float* feat, int ldf, const float* cut, const int* dst,
                                 const int* colptr, const int* perm, const int* order, const int* sp_ptr, int n_species,
                                 int N, int F, float* work, float* dA_na, float* dA_nbr, void* stream) {
    if (N < 0 || F < 1 || n_species < 1 || ldf < 2 * F) return GN_ERR_BAD_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const long nf = (long)N * F, sf = (long)n_species * F;
    if (nf > 0) {
        hipLaunchKernelGGL(gn::emb_source_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st,
                           g_ctx, feat, ldf, cut, dst, colptr, perm, N, F, work);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gn::emb_species_kernel, dim3((unsigned)((sf + 255) / 256)), dim3(256), 0, st,
                       g_ctx, 2 * F, order, sp_ptr, n_species, F, 1, dA_na);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(gn::emb_species_kernel, dim3((unsigned)((sf + 255) / 256)), dim3(256), 0, st,
                       work, F, order, sp_ptr, n_species, F, 0, dA_nbr);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" long gn_layernorm_param_grad_workspace(int N, int C) {
    return 2L * ((N + gn::LN_ROWS - 1) / gn::LN_ROWS) * (long)C;
}

extern "C" int gn_layernorm_param_grad(const float* x, const float* gamma, const float* beta, float eps, const float* g_out,
                                       int N, int C, int act, float* work, float* dgamma, float* dbeta, void* stream) {
    if (N < 0 || C < 1 || act < 0 || act >= GN_ACT_COUNT || (act != GN_ACT_NONE && beta == nullptr)) return GN_ERR_BAD_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const int nch = (N + gn::LN_ROWS - 1) / gn::LN_ROWS;
    if (nch > 0) {
        hipLaunchKernelGGL(gn::ln_param_partial_kernel, dim3(nch), dim3(256), 0, st, x, gamma, beta, eps, g_out, N, C, act, work);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gn::ln_param_reduce_kernel, dim3((C + 255) / 256), dim3(256), 0, st, work, nch, C, dgamma, dbeta);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
