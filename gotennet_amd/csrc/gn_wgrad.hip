// gn_wgrad.hip -- parameter gradients of the Dense products, the embeddings and the LayerNorm affines (first-order
// training).  Every reduction runs in a fixed order with no atomics: identical inputs give identical
// bits.
#include <algorithm>

#include "gn_common.h"
#include "gn_gemm.h"

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

// ---------------------------------------------------------------------------------- weight gradients, f16x2 arithmetic
// The same product as three fp16 MFMAs (v_mfma_f32_32x32x16_f16: hi*hi + hi*lo + lo*hi, fp32 accumulation) on operands
// scaled by power-of-two block exponents and split into two fp16 planes (split4_f16, gn_gemm.h).
//
// Tile.  A workgroup of eight waves owns 128 outputs (nout) x 256 inputs (K): wave w accumulates the outputs
// [32 (w & 3), +32) x the inputs [128 (w >> 2), +128) as four 32 x 32 tiles (64 accumulator registers).  For K <= 256
// every dY element is fetched once per launch and every A element ceil(nout / 128) times.
//
// Exponents.  One per 32-column block and side (4 of dY, 8 of A): the running maximum, along the rows staged so far, of
// the block's binary exponent, so that |x 2^-e| < 2^15.  They only grow; when one grows the accumulators that carry it
// are rescaled by the exact power of two 2^-(growth) <= 1, and the epilogue multiplies by 2^(eY + eA).  A block whose
// maximum is 0 gets the smallest exponent: 0 * 2^120 = 0, its products are exact zeros.  The maxima are combined over
// the workgroup with LDS atomic max on the bit pattern of |x| (order-independent: identical inputs, identical bits).
//
// LDS.  Each stage of 32 rows is kept as row-major fp16 images (planes hi, lo) and the MFMA operands -- 8 consecutive
// ROWS of one column per lane, for both sides -- are read with the transposed read of gfx950 (ds_read_b64_tr_b16): the
// global reads stay row-contiguous and the stores are plain 8-byte writes of four neighbouring columns, where a
// transposing store would need one 2-byte write per element.  Per 16 lanes a read takes 4 rows x 16 columns; lane
// 4q + p supplies the address of row q, columns 4p .. 4p+3 (8 bytes, 8-byte aligned: the pitches are multiples of 4
// elements) and lane i receives column i.  The images are padded to the full tile with zeros, so every lane of every
// read is in bounds and no lane is masked (the read needs EXEC all ones; the only branches around it are wave-uniform).
// Banks: a 32-lane half reads 4 rows x 64 contiguous bytes; the pitches (320 and 576 bytes) are 16 banks mod 64, so the
// four rows fall in the four quarters of the 64 banks: conflict-free.
constexpr int WH_TN = 128;                // output tile: nout
constexpr int WH_TK = 256;                // output tile: K
constexpr int WH_ROWS = 32;               // rows per LDS stage (two MFMA k-steps)
constexpr int WH_PY = WH_TN + 32;         // fp16 per LDS row of a dY plane
constexpr int WH_PA = WH_TK + 32;         // fp16 per LDS row of an A plane
constexpr int WH_NBY = WH_TN / 32, WH_NBA = WH_TK / 32;
constexpr int WH_EMIN = -120, WH_EMAX = 113;
typedef short wh_i16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f16x4 lds_tr4(const _Float16* p) {
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) wh_i16x4*)p));
}
__device__ __forceinline__ f16x8 lds_tr8(const _Float16* p, int pitch) {      // rows 0..3 and 4..7 of the lane's block
    const f16x4 a = lds_tr4(p), b = lds_tr4(p + 4 * pitch);
    return f16x8{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
// maximum over each group of 8 consecutive lanes, valid in the group's last lane (row_shr 1/2/4, zero-filled)
__device__ __forceinline__ unsigned group8_umax(unsigned v) {
    auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = mx(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    return v;
}
__device__ __forceinline__ float absmax4(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
// block exponent of a maximum given as its bit pattern: |x| < 2^(e + 15)
__device__ __forceinline__ int wh_exp(unsigned bits) {
    const int e = (int)((bits >> 23) & 0xffu) - 126 - 15;
    return e < WH_EMIN ? WH_EMIN : (e > WH_EMAX ? WH_EMAX : e);
}
// four consecutive columns from column c of a row with ncols valid columns; one 16-byte load only where `vec` says the
// address is 16-byte aligned and all four are valid
__device__ __forceinline__ float4 wh_load4(const float* q, int c, int ncols, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c + 3 < ncols && vec) return *reinterpret_cast<const float4*>(q);
    if (c < ncols) v.x = q[0];
    if (c + 1 < ncols) v.y = q[1];
    if (c + 2 < ncols) v.z = q[2];
    if (c + 3 < ncols) v.w = q[3];
    return v;
}

__global__ __launch_bounds__(512) void wgrad_f16_partial_kernel(const WgradArgs args) {
    __shared__ __attribute__((aligned(16))) _Float16 sY[2][WH_ROWS][WH_PY];   // planes hi, lo
    __shared__ __attribute__((aligned(16))) _Float16 sA[2][WH_ROWS][WH_PA];
    __shared__ unsigned smax[WH_NBY + WH_NBA];       // running block maxima (bit patterns of |x|)
    int pi = 0;
    while (pi + 1 < args.n && (int)blockIdx.x >= args.p[pi + 1].blk0) ++pi;
    const WgradProb& p = args.p[pi];
    const int b = blockIdx.x - p.blk0;
    const int tiles = p.tiles_n * p.tiles_k;
    const int s = b / tiles, tile = b % tiles;
    const int n0 = (tile / p.tiles_k) * WH_TN, k0 = (tile % p.tiles_k) * WH_TK;
    const int r_begin = min(p.rows, s * p.rows_per_split), r_end = min(p.rows, r_begin + p.rows_per_split);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 3, wk = wave >> 2;
    // this wave's tiles that hold any output (wave-uniform): the others are neither multiplied nor stored
    const int krem = p.K - k0 - wk * 128;
    const int nkt = (n0 + wn * 32 < p.nout && krem > 0) ? min(4, (krem + 31) / 32) : 0;
    // staging: dY as 2 x (16 rows x 32 column quads), A as 4 x (8 rows x 64 column quads); four columns per thread
    const int yq = tid & 31, yr = tid >> 5, aq = tid & 63, ar = tid >> 6;
    const int yc = n0 + 4 * yq, ac = k0 + 4 * aq;
    const bool yvec = (((size_t)p.dY | (size_t)(4 * p.ldy) | (size_t)(4 * p.y_off)) & 15) == 0;
    const bool avec = (((size_t)p.A | (size_t)(4 * p.lda) | (size_t)(4 * p.a_off)) & 15) == 0;
    const bool bias = p.db != nullptr && (tile % p.tiles_k) == 0;
    f32x16 acc[4] = {};
    int eYw = WH_EMIN, eAw[4] = {WH_EMIN, WH_EMIN, WH_EMIN, WH_EMIN};   // exponents the accumulators carry
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ry[2], ra[4];
    auto load = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r0 + yr + 16 * i;
            ry[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < r_end && yc < p.nout) ry[i] = wh_load4(p.dY + wg_row(p, r) * p.ldy + p.y_off + yc, yc, p.nout, yvec);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + ar + 8 * i;
            ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < r_end && ac < p.K) ra[i] = wh_load4(p.A + wg_row(p, r) * p.lda + p.a_off + ac, ac, p.K, avec);
        }
    };
    if (tid < WH_NBY + WH_NBA) smax[tid] = 0u;
    if (r_begin < r_end) load(r_begin);
    __syncthreads();
    // lane addresses of the transposed reads: row 8 (lane >> 5) + ((lane & 15) >> 2), column 16 ((lane >> 4) & 1) + 4 (lane & 3)
    const int trow = 8 * (lane >> 5) + ((lane & 15) >> 2), tcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    for (int r0 = r_begin; r0 < r_end; r0 += WH_ROWS) {
        {   // block maxima of this stage join the running ones (8 lanes share a 32-column block on either side)
            const unsigned uy = group8_umax(__float_as_uint(fmaxf(absmax4(ry[0]), absmax4(ry[1]))));
            const unsigned ua = group8_umax(__float_as_uint(fmaxf(fmaxf(absmax4(ra[0]), absmax4(ra[1])), fmaxf(absmax4(ra[2]), absmax4(ra[3])))));
            if ((lane & 7) == 7) {
                atomicMax(&smax[yq >> 3], uy);
                atomicMax(&smax[WH_NBY + (aq >> 3)], ua);
            }
        }
        __syncthreads();       // maxima complete; the previous stage's LDS reads are done
        {
            const int ey = wh_exp(smax[yq >> 3]), ea = wh_exp(smax[WH_NBY + (aq >> 3)]);
            const float scy = __uint_as_float((unsigned)(127 - ey) << 23), sca = __uint_as_float((unsigned)(127 - ea) << 23);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f16x4 h, l;
                split4_f16(ry[i], scy, h, l);
                *reinterpret_cast<f16x4*>(&sY[0][yr + 16 * i][4 * yq]) = h;
                *reinterpret_cast<f16x4*>(&sY[1][yr + 16 * i][4 * yq]) = l;
                if (bias) { bsum.x += ry[i].x; bsum.y += ry[i].y; bsum.z += ry[i].z; bsum.w += ry[i].w; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f16x4 h, l;
                split4_f16(ra[i], sca, h, l);
                *reinterpret_cast<f16x4*>(&sA[0][ar + 8 * i][4 * aq]) = h;
                *reinterpret_cast<f16x4*>(&sA[1][ar + 8 * i][4 * aq]) = l;
            }
            // the exponents of this wave's tiles: rescale what has been accumulated under smaller ones
            const int ny = __builtin_amdgcn_readfirstlane(wh_exp(smax[wn]));
            const int dy = ny - eYw;
            eYw = ny;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const int na = __builtin_amdgcn_readfirstlane(wh_exp(smax[WH_NBY + 4 * wk + kt]));
                const int d = dy + na - eAw[kt];
                eAw[kt] = na;
                if (d > 0 && kt < nkt) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) acc[kt][reg] = ldexpf(acc[kt][reg], -d);
                }
            }
        }
        __syncthreads();
        if (r0 + WH_ROWS < r_end) load(r0 + WH_ROWS);    // next stage's global reads overlap this stage's MFMAs
        if (nkt > 0) {
#pragma unroll
            for (int ks = 0; ks < WH_ROWS / 16; ++ks) {
                const _Float16* yb = &sY[0][16 * ks + trow][32 * wn + tcol];
                const f16x8 yh = lds_tr8(yb, WH_PY), yl = lds_tr8(yb + WH_ROWS * WH_PY, WH_PY);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    if (kt < nkt) {
                        const _Float16* ab = &sA[0][16 * ks + trow][128 * wk + 32 * kt + tcol];
                        const f16x8 ah = lds_tr8(ab, WH_PA), al = lds_tr8(ab + WH_ROWS * WH_PA, WH_PA);
                        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yh, al, acc[kt], 0, 0, 0);
                        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yl, ah, acc[kt], 0, 0, 0);
                        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yh, ah, acc[kt], 0, 0, 0);
                    }
                }
            }
        }
    }
    // C/D map of the 32x32 MFMA: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* part = p.part + (long)s * ((long)p.nout * p.K + p.nout);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt < nkt) {
            const int kc = k0 + wk * 128 + kt * 32 + (lane & 31);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int n = n0 + wn * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                if (n < p.nout && kc < p.K) part[(long)n * p.K + kc] = ldexpf(acc[kt][reg], eYw + eAw[kt]);
            }
        }
    }
    if (bias) {                // db: plain fp32 column sums; the 16 row groups of the staging are added in order
        float* sB = reinterpret_cast<float*>(&sY[0][0][0]);      // [16][WH_TN] floats = 8 KiB of the dY images
        __syncthreads();
        *reinterpret_cast<float4*>(sB + yr * WH_TN + 4 * yq) = bsum;
        __syncthreads();
        if (tid < WH_TN && n0 + tid < p.nout) {
            float v = 0.f;
            for (int g = 0; g < 16; ++g) v += sB[g * WH_TN + tid];
            part[(long)p.nout * p.K + n0 + tid] = v;
        }
    }
}

// the split of the rows for the f16x2 kernel: at least 512 rows per split, and about 512 workgroups for the problem
static void wgrad_shape_f16(const gn_wgrad_desc& d, int& S, int& rps, int& tn, int& tk) {
    tn = (d.nout + WH_TN - 1) / WH_TN;
    tk = (d.K + WH_TK - 1) / WH_TK;
    const int want = std::max(1, 512 / (tn * tk));
    S = std::max(1, std::min(want, (d.rows + 511) / 512));
    rps = ((d.rows + S - 1) / S + WH_ROWS - 1) / WH_ROWS * WH_ROWS;
    if (rps == 0) rps = WH_ROWS;
    S = std::max(1, (d.rows + rps - 1) / rps);
}

static void wgrad_shape_mode(const gn_wgrad_desc& d, int mode, int& S, int& rps, int& tn, int& tk) {
    if (mode == GN_WGRAD_F16X2) wgrad_shape_f16(d, S, rps, tn, tk);
    else wgrad_shape(d, S, rps, tn, tk);
}

static long wgrad_floats(const gn_wgrad_desc& d, int mode) {
    int S, rps, tn, tk;
    wgrad_shape_mode(d, mode, S, rps, tn, tk);
    return (long)S * ((long)d.nout * d.K + d.nout);
}

// ---------------------------------------------------------------------------------- embeddings
// P[j, c] = sum over the by-source entries of j (stable order), self-loops skipped: g_ctx[i, F + c] feat[e, c] cut[e]
__global__ __launch_bounds__(256) void emb_source_kernel(
    const float* __restrict__ g_ctx, const float* __restrict__ feat, int ldf, const float* __restrict__ cut,
    const int* __restrict__ dst, const int* __restrict__ colptr, const int* __restrict__ perm, int N, int F,
    const float* __restrict__ loop_dist, float* __restrict__ P) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * F) return;
    const int j = (int)(t / F), c = (int)(t % F);
    float acc = 0.f;
    for (int q = colptr[j]; q < colptr[j + 1]; ++q) {
        const int e = perm[q], i = dst[e];
        if (self_loop(j, i, loop_dist, e)) continue;
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

static bool wgrad_mode_ok(int mode) { return mode == GN_WGRAD_F32 || mode == GN_WGRAD_F16X2; }

static long wgrad_workspace(const gn_wgrad_desc* d, int n, int mode) {
    long total = 0;
    for (int i = 0; i < n; ++i) total += gn::wgrad_floats(d[i], mode);
    return total;
}

static int wgrad_group(const gn_wgrad_desc* d, int n, int mode, float* work, long work_floats, void* stream) {
    if (n < 0 || (n > 0 && (d == nullptr || work == nullptr))) return GN_ERR_BAD_ARG;
    if (wgrad_workspace(d, n, mode) > work_floats) return GN_ERR_BAD_ARG;
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
            gn::wgrad_shape_mode(q, mode, p.S, p.rows_per_split, p.tiles_n, p.tiles_k);
            p.dY = q.dY; p.A = q.A; p.dW = q.dW; p.db = q.db; p.part = wp;
            p.ldy = q.ldy; p.y_off = q.y_off; p.lda = q.lda; p.a_off = q.a_off; p.ldw = q.ldw;
            p.rows = q.rows; p.nout = q.nout; p.K = q.K;
            p.cnt = q.row_cnt; p.gstride = q.row_gstride; p.goff = q.row_goff;
            p.blk0 = blocks;
            p.red0 = red;
            blocks += p.S * p.tiles_n * p.tiles_k;
            red += (long)q.nout * q.K + q.nout;
            wp += gn::wgrad_floats(q, mode);
        }
        if (mode == GN_WGRAD_F16X2)
            hipLaunchKernelGGL(gn::wgrad_f16_partial_kernel, dim3(blocks), dim3(512), 0, (hipStream_t)stream, ga);
        else
            hipLaunchKernelGGL(gn::wgrad_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ga);
        GN_LAUNCH_CHECK();
        hipLaunchKernelGGL(gn::wgrad_reduce_kernel, dim3((unsigned)((red + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           ga, red);
        GN_LAUNCH_CHECK();
    }
    return GN_OK;
}

extern "C" long gn_weight_grad_workspace(const gn_wgrad_desc* d, int n) { return wgrad_workspace(d, n, GN_WGRAD_F32); }

extern "C" int gn_weight_grad_group(const gn_wgrad_desc* d, int n, float* work, long work_floats, void* stream) {
    return wgrad_group(d, n, GN_WGRAD_F32, work, work_floats, stream);
}

extern "C" long gn_weight_grad_workspace_mode(const gn_wgrad_desc* d, int n, int mode) {
    return wgrad_mode_ok(mode) ? wgrad_workspace(d, n, mode) : -1;
}

extern "C" int gn_weight_grad_group_mode(const gn_wgrad_desc* d, int n, int mode, float* work, long work_floats, void* stream) {
    if (!wgrad_mode_ok(mode)) return GN_ERR_BAD_ARG;
    return wgrad_group(d, n, mode, work, work_floats, stream);
}

extern "C" int gn_embedding_grad(const float* g_ctx, const float* feat, int ldf, const float* cut, const int* dst,
                                 const int* colptr, const int* perm, const int* order, const int* sp_ptr, int n_species,
                                 int N, int F, float* work, float* dA_na, float* dA_nbr, void* stream) {
    return gn_embedding_grad_images(g_ctx, feat, ldf, cut, dst, colptr, perm, order, sp_ptr, n_species, N, F, nullptr, work,
                                    dA_na, dA_nbr, stream);
}

extern "C" int gn_embedding_grad_images(const float* g_ctx, const float* feat, int ldf, const float* cut, const int* dst,
                                        const int* colptr, const int* perm, const int* order, const int* sp_ptr,
                                        int n_species, int N, int F, const float* edge_diff, float* work, float* dA_na,
                                        float* dA_nbr, void* stream) {
    if (N < 0 || F < 1 || n_species < 1 || ldf < 2 * F) return GN_ERR_BAD_ARG;
    if (!sp_ptr || !dA_na || !dA_nbr) return GN_ERR_BAD_ARG;      // read and written at N = 0 too: plain stores of zeros
    if (N > 0 && (!g_ctx || !feat || !cut || !dst || !colptr || !perm || !order || !work)) return GN_ERR_BAD_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const long nf = (long)N * F, sf = (long)n_species * F;
    if (nf > 0) {
        hipLaunchKernelGGL(gn::emb_source_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st,
                           g_ctx, feat, ldf, cut, dst, colptr, perm, N, F, edge_diff, work);
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
