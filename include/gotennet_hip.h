/*
 * gotennet_hip.h -- C ABI of libgotennet_hip.so (gfx950 / MI355X only).
 *
 * Drop-in boundary for ONE path of sarpaykent/GotenNet: the equivariant
 * interaction stack GotenNet.forward(atomic_numbers, edge_index, edge_diff,
 * edge_vec) -> (h, X)   (reference gotennet/models/representation/gotennet.py:956-1010).
 * The reference has no FFI of its own (it is pure Python on ATen); each entry
 * point below replaces the run of ATen/PyG ops cited next to it, and is what a
 * ctypes binding on the reference side would bind.
 *
 * Contract:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch
 *     `tensor.data_ptr()`), fp32 row-major with the feature axis F fastest;
 *     indices are int32 unless stated; the library never allocates, frees or
 *     synchronises (safe inside hipGraph capture);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - return value: 0 on success, otherwise a hipError_t (launch errors) or
 *     GN_ERR_* (argument errors); no C++ exceptions cross the ABI;
 *   - re-entrant, no global mutable state: no entry point reads the process environment or a mutable static; every
 *     choice of kernel is a function of the arguments (GN_LMAX_SLICED below) or a build-time constant.
 *
 * Symbols: N atoms, E directed edges in CSR-by-target order (edge e runs
 * src[e] = j  ->  dst = i, rowptr[i] <= e < rowptr[i+1]), F = n_atom_basis,
 * H = num_heads, lmax in [1,8] (the range of the reference's TensorInit, layers.py:805-1494), D = (lmax+1)^2 - 1,
 * M = multiplier (number of F-wide blocks in the value vector, gotennet.py:197-203), R = n_rbf.
 * lmax <= 4 runs the register-tiled kernels (the benchmarked configurations); lmax 5..8 the degree-sliced ones
 * (gn_highl.hip: one launch per degree, same arithmetic per row, same fixed-order reductions) behind the SAME
 * entry points.
 */
#ifndef GOTENNET_HIP_H
#define GOTENNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_OK 0
#define GN_ERR_BAD_ARG 10001     /* shape/flag combination the kernels do not implement */
#define GN_ABI_VERSION 11
/* OR-ed into the `lmax` ARGUMENT of gn_message_aggregate, gn_message_backward(_groups), gn_htr_edge and
 * gn_htr_backward: run this call on the degree-sliced kernel family at lmax <= 4 as well (the family that serves
 * lmax 5..8).  An explicit per-call request -- the library reads no environment variable and keeps no switch; every
 * tuning value of the launchers is a build-time constant (csrc/gn_tune.h). */
#define GN_LMAX_SLICED 0x100
/* The reference's `aggr` constructor argument (gotennet.py:84,129,638: PyG scatter reduce of the messages), also carried in
 * the `lmax` argument: default "add"; GN_LMAX_MEAN = "mean" (sum / in-degree, 0 for atoms without incoming edges) in
 * gn_message_aggregate AND gn_message_backward; GN_LMAX_MAX = "max" (element-wise maximum over the incoming edges, 0 without)
 * in gn_message_aggregate only (no backward: GN_ERR_BAD_ARG).  Both run on the degree-sliced kernel family at every lmax. */
#define GN_LMAX_MEAN 0x200
#define GN_LMAX_MAX 0x400

/* `act`: the element-wise activation of the reference's `activation` constructor argument (str2act, layers.py:596-700;
 * shifted_softplus layers.py:40-50).  Wherever an entry point below says SiLU, it means this kind. */
enum {
    GN_ACT_SILU = 0, GN_ACT_SSP = 1, GN_ACT_RELU = 2, GN_ACT_TANH = 3, GN_ACT_SIGMOID = 4, GN_ACT_ELU = 5,
    GN_ACT_SELU = 6, GN_ACT_MISH = 7, GN_ACT_GELU = 8, GN_ACT_SOFTPLUS = 9, GN_ACT_LEAKY = 10,
    GN_ACT_NONE = 11 /* identity: a head without hidden layer */, GN_ACT_COUNT = 12
};

/* Library identity: returns GN_ABI_VERSION; *arch_out (if non-NULL) receives "gfx950". */
int gn_abi_version(const char** arch_out);

/* ---- graph plumbing ------------------------------------------------------------------ */

/* CSR row pointer from the target column of a target-sorted edge list, plus int32
 * copies of both columns.  edge_index is the reference's int64 [2,E] tensor
 * (row 0 = source j, row 1 = target i; gotennet.py:412-424 gathers _j/_i this way).
 * Replaces PyG's implicit index handling in MessagePassing.propagate. */
int gn_build_csr(const int64_t* edge_index, int E, int N, int* src, int* dst, int* rowptr, void* stream);

/* Validation of a caller-supplied edge list (the reference gets this for free from PyG's scatter, which accepts any
 * order; the CSR kernels here need target-major order): *flag (zeroed by the caller) |= 1 when edge_index[1] is not
 * non-decreasing, |= 2 when any index lies outside [0, N).  GotenNet.forward / EnergyForces sort or raise on it. */
int gn_check_edges(const int64_t* edge_index, int E, int N, int* flag, void* stream);

/* By-source (CSC) view of a target-major edge list for the force backward's by-source passes: colptr [N + 1],
 * perm [E] = the CSR edge ids of every source in increasing order (what a stable sort of `src` gives), tgt_by_src [E] =
 * dst[perm].  Built without a sort (count, one-workgroup scan, scatter, per-bucket ranking): four small launches and a
 * memset instead of the ~18 of torch.sort / index_add_ / cumsum.  work: N + E ints of scratch.  Integer arithmetic only. */
int gn_build_csc(const int* src, const int* dst, int E, int N, int* colptr, int* perm, int* tgt_by_src, int* work,
                 void* stream);

/* Offsets of the molecules in a SORTED int64 batch vector (the heads' segment boundaries, outputs.py:349-357 scatter over
 * `batch`): mol_ptr [n_mol + 1], mol_ptr[m] = first atom whose batch index is >= m.  One launch, no host read. */
int gn_molecule_ptr(const int64_t* batch, int N, int n_mol, int* mol_ptr, void* stream);

/* Out-degree of every node counted over ALL edges incl. self-loops
 * (gotennet.py:986-989: scatter(ones, edge_index[0])).  outdeg must be zeroed by the caller. */
int gn_out_degree(const int* src, int E, int* outdeg, void* stream);

/* ---- a radius graph rebuilt inside a recorded step ------------------------------------------------------------------
 * The searches below (gn_radius_count* / gn_radius_fill*) take rowptr and E as arguments and hold every slot to E, so a list
 * of FIXED capacity can be refilled on the device: count over the N real atoms -> gn_degree_scan -> fill with E = capacity
 * -> gn_padded_tail -> gn_graph_refresh.  Every entry point here is kernel launches only (no memset, no copy, no host
 * read): a recorded chain of them holds kernel nodes only.  The sizes are graph.PaddedLayout's: capacity = e_bound + n_pad
 * slots, n_pad dummy atoms N .. N + n_pad - 1 behind the real ones, which own the slots a step does not use. */

/* Exclusive scan of the int32 degrees deg [N] into int64 rowptr64 [N + 1] (what gn_radius_fill* reads), the total also into
 * the device word n_edges [1].  One workgroup (the scan of gn_build_csc, carry across trips of 1024 entries): what
 * torch.cumsum and a host read of its last entry do for graph.distance. */
int gn_degree_scan(const int* deg, int N, int64_t* rowptr64, int* n_edges, void* stream);

/* The inert tail of a padded list.  E_real = rowptr64[N] is read on the device; the slots [E_real, capacity) of edge_index
 * int64 [2, capacity], edge_shift int32 [capacity, 3] (NULL: a list without shifts), edge_vec [capacity, 3] and edge_diff
 * [capacity] become self-loops of the dummy atoms -- src = dst = N + k, shift 0, vector 0, distance 0 -- in the balanced
 * contiguous partition of graph.PaddedLayout.tail_degrees: of the P = capacity - E_real slots the first P % n_pad dummies
 * get P / n_pad + 1 each, the others P / n_pad, so the list stays target-major and every dummy row holds at least one edge.
 * One thread per slot over a grid sized by capacity - N, closed-form integer arithmetic, no atomics.  E_real outside
 * [N, capacity - n_pad] (a count PaddedLayout's bound excludes): nothing is written and the sticky word state[0] is set. */
int gn_padded_tail(const int64_t* rowptr64, int N, int n_pad, int64_t capacity, int64_t* edge_index, int* edge_shift,
                   float* edge_vec, float* edge_diff, int* state, void* stream);

/* gn_build_csr + gn_out_degree (outdeg NULL: not wanted) + gn_build_csc of the target-major edge_index int64 [2, E] into
 * buffers that exist already, bit for bit what those three write; the counters are zeroed in a kernel.  work: N + E ints. */
int gn_graph_refresh(const int64_t* edge_index, int E, int N, int* src, int* dst, int* rowptr, int* outdeg, int* colptr,
                     int* perm, int* tgt_by_src, int* work, void* stream);

/* CosineCutoff alone (layers.py:149-152): cut[e] = 0.5 (cos(pi d / cutoff) + 1) for d < cutoff, else 0.  Used when a
 * caller drives ONE GATA layer (GATA.forward, gotennet.py:366-450, takes r_ij and applies the cutoff inside message). */
int gn_cosine_cutoff(const float* dist, int E, float cutoff, float* cut, void* stream);

/* ---- K1 edge geometry ---------------------------------------------------------------- */
/* unit vector on non-self edges (gotennet.py:978-980), TensorInit real harmonics
 * (layers.py:805-902), ExpNormalSmearing (layers.py:744-746), CosineCutoff (layers.py:149-152).
 * rl [E,D], phi [E,R], cut [E]. edge_vec is NOT modified. */
int gn_edge_geometry(const float* edge_vec, const float* edge_diff, const int* src, const int* dst, int E,
                     int lmax, int R, int basis, const float* means, const float* betas, float cutoff,
                     float* rl, float* phi, float* cut, void* stream);

/* ---- K2/K3 initialisation ------------------------------------------------------------ */
/* The two radial projections W_ndp phi + b (layers.py:1668) and W_erp phi + b (layers.py:1710) are
 * plain gn_gemm calls on phi [E,R]; `feat` below is a row of that product (leading dim ldf). */

/* NodeInit message + aggregate (layers.py:1658-1675) fused with the A_na embedding
 * lookup (gotennet.py:973): ctx[n, 0:F] = A_na[z[n]],
 * ctx[n, F:2F] = sum_{j->n, j!=n} A_nbr[z_j] * (feat_e * cut_e).  ctx is [N, 2F]. */
int gn_node_init(const int* z, const int* rowptr, const int* src, const float* feat, int ldf,
                 const float* cut, const float* A_na, const float* A_nbr,
                 int N, int F, float* ctx, void* stream);

/* EdgeInit.message (layers.py:1709-1710): t[e] = (h[i] + h[j]) * feat_e for all edges. */
int gn_edge_init(const float* h, const int* rowptr, const int* src, const float* feat, int ldf,
                 int N, int F, float* t, void* stream);

/* y = SiLU(LayerNorm(x) * gamma + beta) row-wise over F (Dense with norm='layer',
 * layers.py:518-529, inside NodeInit's W_nrd_nru).  In place allowed (y == x). */
int gn_layernorm_silu(const float* x, const float* gamma, const float* beta, float eps,
                      int N, int F, float* y, int act /* GN_ACT_* */, void* stream);

/* ---- optional GATA input norms (gotennet.py:305-315, 397-398; off by default) ----------- */
/* y = LayerNorm(x) * gamma + beta (nn.LayerNorm(F), `layernorm != ""`). */
int gn_layernorm(const float* x, const float* gamma, const float* beta, float eps,
                 int N, int F, float* y, void* stream);
/* TensorLayerNorm (layers.py:1497-1563, `steerable_norm != ""`): per atom and degree block l,
 * s_f = |X_l[:, f]|, c_f = max(s_f, eps), n_f = (c_f - min_f c) / (max_f c - min_f c) (denominator 1 if equal),
 * Y = relu(n_f) * X / c_f * weight_f.  X, Y are [N,D,F]; eps = 1e-12 in the reference. */
int gn_tensor_norm(const float* X, const float* weight, float eps, int N, int F, int lmax, float* Y, void* stream);

/* ---- dense projections (K4/K5/K7/K8), fp32 MFMA --------------------------------------- */
/* C[r, n] = epi( sum_k A[r, k] * W[n, k] + bias[n] )      (nn.Linear layout W[out,in]; Dense, layers.py:457-529)
 *   rows:  logical row r in [0, Mrows) maps to physical row (r / row_cnt) * row_gstride + row_goff + r % row_cnt
 *          in both A (leading dim lda) and C (ldc); pass (1,1,0) for the identity.  This addresses the
 *          degree-l' rows of an [N, D, F] tensor for W_vk[l'] (gotennet.py:432-441).
 *   epi:   SiLU on output columns [act_lo, act_hi); then, if gate != NULL,
 *          C = res + value * gate  (res, gate: same addressing as C; HTR update t += SiLU(W t + b) * w,
 *          gotennet.py:445,611).  bias may be NULL.  K must be a multiple of 4. */
int gn_gemm(const float* A, int lda, const float* W, const float* bias, float* C, int ldc,
            int Mrows, int Nout, int K, int act_lo, int act_hi,
            int row_cnt, int row_gstride, int row_goff,
            const float* res, const float* gate, void* stream);

/* Extended form used by the pipeline.  Extra epilogue: pre_out (if non-NULL) receives the value BEFORE
 * the activation (same addressing as C); `res` alone (gate == NULL) gives C = res + value; gate_mode 1
 * multiplies by SiLU'(gate) instead of gate (backward through an activation, applied once per output
 * element in the PRODUCER's epilogue; res may then be NULL).  Prologue on A,
 * applied while staging, on A columns [pro_lo, pro_hi): pro_mode 1: A <- SiLU(A) (activations are stored
 * pre-activation); pro_mode 2: A <- A * SiLU'(a_pre) (backward through a SiLU; a_pre has A's row addressing
 * with leading dim ldp); and A <- A * a_gate on every column when a_gate != NULL (leading dim ldg). */
int gn_gemm_ex(const float* A, int lda, const float* W, const float* bias, float* C, int ldc,
               int Mrows, int Nout, int K, int act_lo, int act_hi,
               int row_cnt, int row_gstride, int row_goff,
               const float* res, const float* gate, int gate_mode, float* pre_out,
               int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
               const float* a_gate, int ldg, int act_kind /* GN_ACT_* */, void* stream);

/* Several INDEPENDENT gn_gemm_ex problems (Dense products, layers.py:457-529; call sites gotennet.py:400-407, 432-441,
 * 611, 728, 738) in one launch (no problem may read what another writes).  The atom-sized
 * products of a layer (x / v, EQ / EK_l / X W_vu^T, and the matching input-gradient products) fill a fraction of the
 * 256 CUs one at a time; a group walks all their tiles with one persistent grid.  n <= 4; every field has the meaning
 * of the gn_gemm_ex argument of the same name. */
typedef struct gn_gemm_desc {
    const float* A; int lda;
    const float* W; const float* bias;
    float* C; int ldc;
    int M, N, K;
    int act_lo, act_hi;
    int row_cnt, row_gstride, row_goff;
    const float* res; const float* gate; int gate_mode;
    float* pre_out;
    int pro_mode, pro_lo, pro_hi;
    const float* a_pre; int ldp;
    const float* a_gate; int ldg;
    /* K-segmented A: when a_seg != 0 the logical A columns [s a_seg, (s+1) a_seg) come from A, A2, A3 (s = 0, 1, 2;
     * same row addressing; a_seg % 32 == 0; no prologue): C = res + A W_0^T + A2 W_1^T + A3 W_2^T with the
     * weights concatenated along K.  The last segment may be narrower than a_seg (a_seg < K <= 2 a_seg: two segments;
     * 2 a_seg < K <= 3 a_seg: three).  Used for gX = gX + gXp W_vu + gEQ W_vq + gEK_l W_vk_l and, with lda2, for
     * dL/dt = gt + g_eproj W_e + g_pre_t W_t. */
    const float* A2; const float* A3; int a_seg;
    int act_kind;                /* GN_ACT_*: activation of the [act_lo, act_hi) columns, of gate_mode 1 and of the prologues */
    int lda2;                    /* leading dimension of A2 and A3 (a multiple of 4); 0: the same as lda */
} gn_gemm_desc;
int gn_gemm_group(const gn_gemm_desc* problems, int n, void* stream);

/* 3 x bf16 split variant of the same Dense products (layers.py:457-529): same contract as
 * gn_gemm_ex / gn_gemm_group, but every weight is passed as the bf16 planes written ONCE per weight by
 * gn_split_bf16x3 (W = hi + mid + lo exactly, each plane bf16; stored in the order the matrix cores consume them:
 * [column block of 32][k-step of 16, padded to an even count][plane][lane][8], gn_split_bf16x3_size(N, K) bf16
 * elements).  The product is accumulated in fp32 from the six plane pairs of order <= 2 on the bf16 matrix cores
 * (v_mfma_f32_32x32x16_bf16): fp32-class error (<= 1e-6 relative to an fp64 product) at 16/6 of the exact-fp32
 * MFMA rate.  A is split on the fly; K must be a multiple of 4 as for gn_gemm_ex. */
long gn_split_bf16x3_size(int N, int K);
int gn_split_bf16x3(const float* w /* [N][K] fp32 */, int N, int K, unsigned short* out, void* stream);
int gn_gemm_split(const float* A, int lda, const unsigned short* W3, const float* bias, float* C, int ldc,
                  int Mrows, int Nout, int K, int act_lo, int act_hi,
                  int row_cnt, int row_gstride, int row_goff,
                  const float* res, const float* gate, int gate_mode, float* pre_out,
                  int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
                  const float* a_gate, int ldg, int act_kind, void* stream);
/* gn_gemm_group on the split path: every problems[i].W points to gn_split_bf16x3 planes (cast to const float*). */
int gn_gemm_group_split(const gn_gemm_desc* problems, int n, void* stream);

/* 2 x fp16 split variant with block exponents: the same contract again, every weight passed as the buffer written
 * ONCE per weight by gn_split_f16x2 (a 256-byte header holding the tensor's binary exponent, then two fp16 planes
 * hi + lo of w * 2^-exponent in the same fragment-major order; gn_split_f16x2_size(N, K) 16-bit elements; the amax is
 * found on the device, no host read-back).  A is scaled per (staging wave, K-slab of 32 columns) by the running maximum
 * of that block's binary exponent (exact powers of two, accumulators rescaled when it grows): wave q of four stages rows
 * 8q..8q+7 of every 32-row MFMA tile of the workgroup tile, so 16 rows (64-row tiles) or 32 rows (128-row tiles) share
 * an exponent (the eight-wave 128 x 256 tile, GN_GEMM_FORM_BIG8 below: 16 rows) -- results are bit-reproducible but depend at the 1e-7 level on which rows are neighbours (INTEGRATION.md:
 * batch-position contract; per-row bound: tests/test_hip_parity.py::test_fp16_block_exponent_per_row_bound).  Each scaled
 * operand is split into two fp16 planes, and
 * the product accumulated in fp32 from THREE plane pairs on v_mfma_f32_32x32x16_f16 -- half the matrix work of the
 * bf16 split; 22 significand bits per operand: <= 2e-7 of the output's max-norm against an fp64 product. */
long gn_split_f16x2_size(int N, int K);
int gn_split_f16x2(const float* w /* [N][K] fp32 */, int N, int K, unsigned short* out, void* stream);
int gn_gemm_f16x2(const float* A, int lda, const unsigned short* W2, const float* bias, float* C, int ldc,
                  int Mrows, int Nout, int K, int act_lo, int act_hi,
                  int row_cnt, int row_gstride, int row_goff,
                  const float* res, const float* gate, int gate_mode, float* pre_out,
                  int pro_mode, int pro_lo, int pro_hi, const float* a_pre, int ldp,
                  const float* a_gate, int ldg, int act_kind, void* stream);
int gn_gemm_group_f16x2(const gn_gemm_desc* problems, int n, void* stream);
/* The same group on a NAMED 128-row tile of the slab kernel instead of the routed kernel (no prologue for BIG8; otherwise
 * GN_ERR_BAD_ARG): GN_GEMM_FORM_BIG = 128 x 128, four waves, 32 rows per block exponent; GN_GEMM_FORM_BIG8 = 128 x 256, eight
 * waves -- an A slab is scaled and split once per row panel; the eight staging waves each keep their own exponent, so 16 rows
 * (rows 8q..8q+7 of the M-tiles i and i + 2 of the panel) share one: same per-row bound, not the same bits as BIG.
 * gn_gemm_group_f16x2 routes edge-sized groups with N <= 256 and a K-heavy leading problem to BIG8 (csrc/gn_tune.h).  For A/B
 * probes and for tests that hold one form against the other at small shapes. */
#define GN_GEMM_FORM_BIG 1
#define GN_GEMM_FORM_BIG8 2
int gn_gemm_group_f16x2_form(const gn_gemm_desc* problems, int n, int form, void* stream);

/* ---- K6 GATA message / softmax / aggregate -------------------------------------------- */
/* Attention weights (gotennet.py:497-511): s[e,h] = sum_{c in head h} q[i,c] k[j,c] t_attn[e,c];
 * a = exp(s - max) / (sum + 1e-16) over the incoming edges of i (PyG softmax), then
 * a *= 1/sqrt(F)  or  sqrt(outdeg[j])/sqrt(F) when outdeg != NULL (scale_edge).  a is [E,H].
 * q,k are rows of ldqk floats; t_attn rows of ldt floats hold the PRE-activation W_re t + b
 * (the kernel applies SiLU while loading). */
int gn_attn_softmax(const float* q, const float* k, int ldqk, const float* t_attn, int ldt,
                    const int* rowptr, const int* src, const int* outdeg,
                    int N, int F, int H, float* a, int act /* GN_ACT_*: t_attn = act(.) */, void* stream);

/* ---- attention dropout (training mode; reference gotennet.py:513, F.dropout on the attention weights) ----------
 * The mask is a pure, counter-based function of (key, layer, e, h): nothing is stored, the forward and whoever wants to
 * reproduce a step evaluate the same function.  For element n = e * H + h (a 64-bit count; e = the edge's index in the
 * TARGET-MAJOR order the kernels run on, i.e. the CSR edge id):
 *     word = output word 0 of Philox4x32-10 with counter (lo32(n), hi32(n), layer, 0) and key (lo32(key[0]), hi32(key[0]))
 *     m[e,h] = word >= floor(p * 2^32) ? 1 / (1 - p) : 0          (1 / (1 - p) in double, rounded once to fp32)
 * p >= 1 drops everything (m = 0, as torch does); p = 0 keeps everything with m = 1; p < 0 or NaN: GN_ERR_BAD_ARG.
 * `key` is a DEVICE pointer to two int64 values {seed, reserved (ignored)}: the kernels read it on the device, no value
 * crosses to the host, and a captured launch replays with whatever the buffer then holds.
 *
 * gn_attn_softmax_dropout: gn_attn_softmax that writes a_soft [E,H] = the weights above (softmax * norm) AND
 * a [E,H] = a_soft * m in the same final pass (a_soft != a).  Everything downstream of the softmax (gn_message_aggregate,
 * the message backward) takes `a`; only the softmax backward also reads a_soft (gn_message_backward_dropout). */
int gn_attn_softmax_dropout(const float* q, const float* k, int ldqk, const float* t_attn, int ldt,
                            const int* rowptr, const int* src, const int* outdeg,
                            int N, int F, int H, float* a_soft, float* a, const long long* key, int layer, double p,
                            int act, void* stream);
/* The multipliers m [E,H] alone. */
int gn_attn_dropout_mask(const long long* key, int layer, double p, long E, int H, float* m_out, void* stream);

/* Message + segmented reduction + residual (gotennet.py:516-559, 613-640, 426-427):
 *   o[c]   = t_filter[e,c] * x[j,c] * cut[e] + a[e, c / (M F / H)] * v[j,c],  c in [0, M F)
 *   h_out[i]     = h_in[i] + sum_e o[0:F]
 *   X_out[i,m,:] = X_in[i,m,:] + sum_e ( rl[e,m] * o[dblk(l(m))] + X_in[j,m,:] * o[tblk(l(m))] )
 * with dblk/tblk the F-wide block of the direction / tensor gate of degree l (sep_dir / sep_tensor).
 * x, v rows of ldxv floats; t_filter rows of ldt floats.  X_out must not alias X_in.
 * X_in == NULL (lmax <= 4) means "X_in is identically zero" -- the first interaction of GotenNet.forward, which starts
 * from X = 0 (gotennet.py:992): the tensor-gate blocks of t_filter / x / v are then NOT READ (they may be unwritten)
 * and X_out = the aggregated update; same bits as passing a zero tensor. */
int gn_message_aggregate(const float* x, const float* v, int ldxv, const float* t_filter, int ldt,
                         const float* a, const float* rl, const float* cut,
                         const int* rowptr, const int* src,
                         const float* h_in, const float* X_in, float* h_out, float* X_out,
                         int N, int F, int H, int lmax, int sep_dir, int sep_tensor, void* stream);

/* ---- EQFF node chains as one kernel each (gotennet.py:716-748 after X_p = X W_vu^T) ------------------------------ */
/* Forward: n = sqrt(sum_D X_p^2 + eps); [m1 | m2] = W_1 SiLU(W_0 [h | n] + b_0) + b_1; h += m1; X += m2 * X_p -- the
 * sequence gn_eqff_context -> gn_gemm(gamma_m.0) -> gn_gemm(gamma_m.1) -> gn_eqff_update as ONE launch (8 atoms per
 * workgroup, both products on MFMA in the plane arithmetics, W0p / W1p = planes written by gn_split_bf16x3 /
 * gn_split_f16x2 of gamma_m.0.weight [F, 2F] and gamma_m.1.weight [2F, F]).  ctx_out [N,2F], pre_out [N,F] (the
 * pre-activation of the hidden layer), mm_out [N,2F]: what the backward needs, or NULL.
 * Backward: gn_eqff_backward_a -> W_1^T -> W_0^T -> gn_eqff_backward_b as one launch: given g_h, g_X [N,D,F] of the
 * block's outputs returns g_Xp [N,D,F] (gradient w.r.t. X_p, not yet through W_vu) and g_h1 = g_h + d/dh through gamma_m;
 * W1Tp / W0Tp = planes of the TRANSPOSED weights ([F, 2F] and [2F, F]).  g_Xp must not alias g_X.
 * Supported: F in {128, 256}, SiLU, arith 1 (3 x bf16) or 2 (2 x fp16); otherwise callers keep the launch sequence. */
int gn_eqff_fused_supported(int F, int act, int arith);
int gn_eqff_fused_forward(const float* Xp, const void* W0p, const float* b0, const void* W1p, const float* b1,
                          float eps, int N, int F, int D, float* h, float* X,
                          float* ctx_out, float* pre_out, float* mm_out, int arith, void* stream);
int gn_eqff_fused_backward(const float* gh, const float* gX, const float* mm, const float* Xp, const float* ctx,
                           const float* pre_g1, const void* W1Tp, const void* W0Tp, int N, int F, int D,
                           float* gXp, float* gh1, int arith, void* stream);

/* ---- K7 HTR edge weights -------------------------------------------------------------- */
/* w[e,f] = sum_l sum_m P(EQ[i])_m * P(EK[j])_m with P(a) = a - (a . rl_l) rl_l per degree block
 * (gotennet.py:351-364, 580-609; sep_htr=True, rejection on).  EQ, EK are [N,D,F]; w is [E,F]. */
/* `mode` selects the reference's non-default edge-update variants (gotennet.py:139-190, 285-291, 580-599):
 *   GN_HTR_JOINT  sep_htr=False: one rejection block over all D rows instead of one per degree;
 *   GN_HTR_NOREJ  "norej": no vector rejection;
 *   GN_HTR_GATE_* gamma_w applied to w: "gated" sigmoid, "gatedt" tanh, "act" SiLU.
 * mode = 0 is the default path.  w_raw (optional, may be NULL) receives w before the gate (the backward needs it
 * when a gate is set). */
#define GN_HTR_JOINT 1
#define GN_HTR_NOREJ 2
#define GN_HTR_GATE_SIGMOID (1 << 2)
#define GN_HTR_GATE_TANH (2 << 2)
#define GN_HTR_GATE_SILU (3 << 2)
#define GN_HTR_DIRECT 16 /* gn_htr_backward only: g_t_out already is dL/dw [E,F]; pre_t, w, w_raw, g_pre_t unused */
int gn_htr_edge(const float* EQ, const float* EK, const float* rl, const int* rowptr, const int* src,
                int N, int F, int lmax, int mode, float* w_raw, float* w, void* stream);

/* ---- K8 EQFF node-local pieces -------------------------------------------------------- */
/* ctx[n, 0:F] = h[n]; ctx[n, F:2F] = sqrt(sum_m Xp[n,m,:]^2 + eps)   (gotennet.py:731-735) */
int gn_eqff_context(const float* h, const float* Xp, float eps, int N, int F, int D, float* ctx, void* stream);
/* h += m[:, 0:F];  X += m[:, F:2F] (broadcast over D) * Xp           (gotennet.py:741-746); m is [N,2F] */
int gn_eqff_update(const float* m, const float* Xp, int N, int F, int D, float* h, float* X, void* stream);

/* ---- K10 force backward (input gradients only; what torch.autograd.grad does for the reference at
 *      outputs.py:365-375).  Needs the by-source (CSC) view: tgt_by_src[pp] is the TARGET of by-source entry pp
 *      (= dst[perm[pp]], stored so that the source passes chase one index less per edge) and
 *      perm[colptr[j] .. colptr[j+1]) lists the CSR
 *      edge ids whose source is j.  F <= 256.  Every kernel WRITES its g_rl [E,D] / g_cut [E] contribution to
 *      the slice it is given (plain stores, no read-modify-write); gn_edge_geometry_backward sums the slices. */

/* HTR (gotennet.py:561-611) backward: g_t_out = dL/dt' [E,F], pre_t = W_t t + b and w (saved), w.r.t. EQ, EK,
 * rl, and g_pre_t = g_t_out * w * SiLU'(pre_t) [E,F] (the operand of the W_t^T product). */
int gn_htr_backward(const float* g_t_out, const float* pre_t, const float* w, const float* w_raw,
                    const float* EQ, const float* EK,
                    const float* rl, const int* rowptr, const int* src, const int* tgt_by_src,
                    const int* colptr, const int* perm, int N, int F, int lmax, int mode,
                    float* gEQ, float* gEK, float* g_rl, float* g_pre_t, int act /* GN_ACT_* of gamma_t */, void* stream);

/* GATA message/softmax/aggregate (gotennet.py:452-559, 613-640) backward.  Inputs: saved x, v [N,MF];
 * eproj [E,(1+M)F] = (pre-activation of t_attn | t_filter); a [E,H]; qk rows with q at column 0 and k at
 * column F; X_in [N,D,F]; upstream g_h1 [N,F], g_X1 [N,D,F].  Outputs: g_eproj [E,(1+M)F] (gradient w.r.t.
 * the t_attn pre-activation | t_filter), g_s [E,H] scratch, g_nproj rows (ldn) with g_q at column 0 and g_k
 * at column F, g_x, g_v [N,MF], g_X_out = g_X1 + (tensor-gate path), g_rl [E,D] and g_cut [E] slices.
 * X_in == NULL (lmax <= 4, SiLU): X_in identically zero (first interaction); one g_cut slice is written (not one per degree group).  The tensor-gate blocks of eproj / x / v
 * are not read, the tensor-gate columns of g_eproj are NOT WRITTEN (take the K-prefix (2 + ND) F of the W_e^T product
 * that consumes it), those blocks of g_x / g_v are written as zeros, g_X_out is not written (may be NULL). */
int gn_message_backward(const float* x, const float* v, int ldxv, const float* eproj, int lde, const float* a,
                        const float* qk, int ldqk, const float* X_in, const float* rl, const float* cut,
                        const int* outdeg, const float* g_h1, const float* g_X1,
                        const int* rowptr, const int* src, const int* tgt_by_src, const int* colptr, const int* perm,
                        float* g_eproj, float* g_s, float* g_nproj, int ldn, float* g_x, float* g_v,
                        float* g_X_out, float* g_rl, float* g_cut, float* ga_parts, long E,
                        int N, int F, int H, int lmax, int sep_dir, int sep_tensor, int act, void* stream);
/* ... of a layer whose forward ran gn_attn_softmax_dropout: a = the dropped weights (what the message stage used), a_soft the
 * undropped ones.  With dot = sum_e' a[e'] g_a[e'] over the target's edges, g_s[e] = a[e] g_a[e] - (a_soft[e] / nrm_e) dot;
 * every other term is gn_message_backward's with `a`.  No random numbers are drawn. */
int gn_message_backward_dropout(const float* x, const float* v, int ldxv, const float* eproj, int lde, const float* a,
                                const float* a_soft,
                                const float* qk, int ldqk, const float* X_in, const float* rl, const float* cut,
                                const int* outdeg, const float* g_h1, const float* g_X1,
                                const int* rowptr, const int* src, const int* tgt_by_src, const int* colptr, const int* perm,
                                float* g_eproj, float* g_s, float* g_nproj, int ldn, float* g_x, float* g_v,
                                float* g_X_out, float* g_rl, float* g_cut, float* ga_parts, long E,
                                int N, int F, int H, int lmax, int sep_dir, int sep_tensor, int act, void* stream);
/* Number of degree groups G the message backward uses for these flags (1 = monolithic kernels, lmax >= 5, and every
 * activation other than GN_ACT_SILU -- those run the degree-sliced kernels; lmax 3..4 with sep_dir and sep_tensor
 * and SiLU: {scalar,1,2}, {3}, {4}).  g_cut must then hold G consecutive [E] slices and ga_parts
 * G x [E,H] floats of workspace.  With G = 1, ga_parts ([E,H] floats) selects the single-read form of the register-tiled
 * kernels (the by-source kernel does the per-edge work, then attention backward, then g_k: t_filter is read once);
 * ga_parts = NULL keeps the by-target / by-source pair (t_filter read by both).  The same holds for X_in == NULL (the first
 * interaction) at every lmax <= 4: with ga_parts ([E,H] floats) the single-read kernel runs in its form without the tensor-gate
 * blocks, without it the zero-X_in forms of the pair.  Same gradients either way (summation order aside).
 * More than eight heads (H > 8) with G > 1: the degree-group kernels carry eight head sums per edge, so the call runs the
 * degree-sliced kernels instead; they write ONE g_cut slice and the launcher zeroes the other G - 1, the caller's sizes
 * and its sum over G slices stay as they are.
 * GN_LMAX_MAX in `lmax` (the reference's aggr = "max", gotennet.py:638-639): ga_parts is instead a workspace of
 * E x (1 + D) x F floats -- the upstream gradient of every per-edge MESSAGE, routed to the arg-max edge(s) of each output
 * element (evenly among exact ties, as torch's amax) before the degree-sliced backward kernels run; G = 1, X_in required. */
int gn_message_backward_groups(int lmax, int sep_dir, int sep_tensor, int act);

/* EQFF (gotennet.py:716-748) backward, node-local halves around the two gamma_m GEMMs:
 * a: g_m = [g_h | sum_m g_X Xp], g_Xp = g_X * m2;   b: g_Xp += g_ctx[:,F:] Xp / n, g_h1 = g_h + g_ctx[:, :F].
 * g_X == NULL in (a): dL/dX of the block's output is identically zero (an energy head that reads h only,
 * outputs.py:333-346): g_m = [g_h | 0], g_Xp = 0, nothing is read in its place. */
int gn_eqff_backward_a(const float* g_h, const float* g_X, const float* m, const float* Xp,
                       int N, int F, int D, float* g_m, float* g_Xp, void* stream);
int gn_eqff_backward_b(const float* g_ctx, const float* ctx, const float* Xp, const float* g_h,
                       int N, int F, int D, float* g_Xp, float* g_h1, void* stream);

/* EdgeInit (layers.py:1709-1710) backward: g_feat[e, F:2F] = g_t0 (h_i + h_j); g_h[n] += in- and out-edge sums
 * of g_t0 * feat[e, F:2F].  feat/g_feat are the [E, 2F] radial projections (W_ndp | W_erp). */
int gn_edge_init_backward(const float* g_t0, const float* h, const float* feat, int ldf,
                          const int* rowptr, const int* src, const int* colptr, const int* perm,
                          int N, int F, float* g_feat, float* g_h, void* stream);
/* NodeInit aggregate (layers.py:1666-1675) backward: g_feat[e, 0:F] and the g_cut [E] slice from g_ctx[:, F:2F]. */
int gn_node_init_backward(const float* g_ctx, const int* z, const float* feat, int ldf, const float* cut,
                          const float* A_nbr, const int* rowptr, const int* src, int N, int F,
                          float* g_feat, float* g_cut, void* stream);
int gn_layernorm_silu_backward(const float* x, const float* gamma, const float* beta, float eps,
                               const float* g_out, int N, int F, float* g_x, int act, void* stream);
/* input-gradients of gn_layernorm / gn_tensor_norm (x / X are the un-normalised inputs).  torch.max / torch.min
 * route their gradient to one channel: the first extremal one. */
int gn_layernorm_backward(const float* x, const float* gamma, float eps,
                          const float* g_out, int N, int F, float* g_x, void* stream);
int gn_tensor_norm_backward(const float* X, const float* weight, const float* g_Y, float eps, int N, int F,
                            int lmax, float* g_X, void* stream);

/* ---- element-wise pieces of the composed edge update (gotennet.py:236-291: gamma_t as a 2-layer MLP "mlp"/"mlpa",
 *      gamma_w = [LayerNorm "ln"] [act "linwa"] W_edp "linw" [LayerNorm "postln"] [gate]); n = element count, n % 4 = 0.
 *      kind: 0 identity, 1 sigmoid, 2 tanh, 3 SiLU. */
int gn_gate(const float* x, int kind, long n, float* y, void* stream);
int gn_gate_backward(const float* g, const float* x, int kind, long n, float* g_x, void* stream);
/* t' = t + act(pre) * wg  ->  g_pre = g act'(pre) wg,  g_wg = g act(pre);  act in {0, 3}. */
int gn_edge_gate_backward(const float* g, const float* pre, int act, const float* wg, long n,
                          float* g_pre, float* g_wg, void* stream);

/* Edge geometry (K1) backward: (sum of the n_rl slices g_rl [n_rl,E,D], sum of the n_cut slices g_cut [n_cut,E],
 * g_phi [E,R]) -> g_vec [E,3] through the unit vector and harmonics, g_diff [E] through cutoff and radial
 * basis.  Self-loops get zeros. */
int gn_edge_geometry_backward(const float* edge_vec, const float* edge_diff, const int* src, const int* dst,
                              int E, int lmax, int R, int basis, const float* means, const float* betas, float cutoff,
                              const float* g_rl, int n_rl, const float* g_cut, int n_cut, const float* g_phi,
                              float* g_vec, float* g_diff, void* stream);
/* out[n] = sign * ( sum_{src(e)=n} gv_e - sum_{dst(e)=n} gv_e ), gv = g_vec + g_diff * edge_vec/|edge_vec|
 * (Distance.forward, layers.py:1593-1600: edge_vec = pos[j]-pos[i], edge_weight = |edge_vec|). sign=-1: forces. */
int gn_pos_scatter(const float* g_vec, const float* g_diff, const float* edge_vec,
                   const int* rowptr, const int* colptr, const int* perm, int N, float sign,
                   float* out, void* stream);

/* ---- K10 energy head (Atomwise, outputs.py:323-376; SchnetMLP layers.py:225-273, 2 layers, SiLU) ------- */
/* y_n = scale * (sum_k SiLU(pre1[n,k]) W2[k] + b2) + shift (+ atomref[z_n]); energy[b] = sum_{n in molecule b} y_n + mol_shift.
 * Atomwise (outputs.py:323-376) standardises per atom: scale = stddev, shift = mean, mol_shift = 0.  AtomwiseV3
 * (outputs.py:96-229) scales per atom and adds its mean AFTER the aggregation: scale = stddev, shift = 0, mol_shift = mean.
 * pre1 = W1 h + b1 comes from gn_gemm.  mol_ptr [n_mol+1] int32.  head_grad: g_pre1 = scale W2 SiLU'(pre1). */
int gn_head_energy(const float* pre1, const float* W2, float b2, float scale, float shift, float mol_shift,
                   const float* atomref, const int* z, const int* mol_ptr, int n_mol, int Hd,
                   float* y, float* energy, int mean /* aggregation_mode "mean": energy / atoms of the molecule */,
                   float* atom_scale /* [N] or NULL: d energy / d y_n (1 or 1 / atoms) for gn_head_grad */,
                   int act /* GN_ACT_* of the head MLP (GN_ACT_NONE: no hidden layer) */, void* stream);
int gn_head_grad(const float* pre1, const float* W2, float scale, const float* atom_scale /* [N] or NULL */, int N, int Hd,
                 float* g_pre1, int act, void* stream);

/* ---- vector-representation read-outs of the QM9 task (QM9Task.py:168-187) ---------------------------------------
 * GatedEquivariantBlock (outputs.py:24-93) around two gn_gemm products:
 *   vmix [N*3, ldv] = mix_vectors(vectors): V at column 0, W at column w_off, each n_vout wide;
 *   gn_geb_context:  ctx [N, ldc] = [scalars (n_sin) | ||V||_2 over the 3 components (n_vout) | zeros];
 *   x [N, ldx] = scalar_net(ctx) = [s (n_sout) | gate (n_vout) | padding]            (gn_gemm, twice);
 *   gn_geb_gate:     s_out = sactivation(s) (sact = GN_ACT_* or -1 for none), v_out [N*3, ldo] = gate * W.
 * gn_geb_context writes every column of ctx (the padding [n_sin + n_vout, ldc) as 0: the product that follows reads
 * whole rows); gn_geb_gate writes columns [0, n_sout) of s_out and [0, n_vout) of v_out and leaves the rest alone.
 * GN_ERR_BAD_ARG before any launch: a width <= 0, a leading dimension below its width (ldc < n_sin + n_vout,
 * ldx < n_sout + n_vout, ldv < w_off + n_vout), w_off < 0, an unknown sact, and -- once N > 0 -- a NULL pointer.
 * N = 0: GN_OK, nothing read or written. */
int gn_geb_context(const float* s, int lds, int n_sin, const float* vmix, int ldv, int n_vout, int N,
                   float* ctx, int ldc, void* stream);
int gn_geb_gate(const float* x, int ldx, int n_sout, int n_vout, const float* vmix, int ldv, int w_off, int N,
                int sact, float* s_out, int lds, float* v_out, int ldo, void* stream);
/* Dipole (outputs.py:430-468): y_b = sum_{n in molecule b} (mu_n + pos_n q_n), q_n = scale q_n + shift when
 * standardise; y [n_mol,3], or [n_mol] = |y_b| when magnitude; y_vec [n_mol,3] = sum mu_n (or NULL).
 * mu [N*3, ldm] and q [N, ldq]: column 0 is read.  An empty molecule gives zeros.  GN_ERR_BAD_ARG before any launch:
 * n_mol < 0, ldm or ldq <= 0, y NULL, and -- once n_mol > 0 -- mu, q, pos or mol_ptr NULL.  n_mol = 0: GN_OK, nothing
 * read or written. */
int gn_dipole_reduce(const float* mu, int ldm, const float* q, int ldq, const float* pos, const int* mol_ptr,
                     int n_mol, float scale, float shift, int standardise, int magnitude, float* y, float* y_vec,
                     void* stream);
/* ElectronicSpatialExtentV2 (outputs.py:516-545): c_b = mass-weighted centroid, y_b = sum_n |pos_n - c_b|^2 x_n;
 * mass [n_mass] indexed by atomic number (z < 0 or >= n_mass: mass 0).  A molecule whose masses sum to 0 (an empty one
 * too) gets c_b = 0, no 0 / 0.  GN_ERR_BAD_ARG before any launch: n_mol < 0, n_mass <= 0, y NULL, and -- once
 * n_mol > 0 -- x, pos, z, mass or mol_ptr NULL.  n_mol = 0: GN_OK, nothing read or written. */
int gn_ese_reduce(const float* x, const float* pos, const int* z, const float* mass, int n_mass, const int* mol_ptr,
                  int n_mol, float* y, void* stream);
/* Backward of the four kernels above (first-order training of the read-outs).  Node-local or one
 * workgroup per molecule with sums in a fixed order, no atomics: identical inputs give identical bits.
 *   gn_geb_gate_backward: from g_s_out [N, ldgs] and g_v_out [N*3, ldgo] with the saved x and vmix:
 *     g_x [N, ldgx] = [g_s_out sact'(s) | sum_m g_v_out[m] W[m] | zeros] and the W half of g_vmix [N*3, ldgv]:
 *     columns [w_off, ldgv) = gate g_v_out, zeros past n_vout.
 *   gn_geb_context_backward: g_s [N, lds] = g_ctx[:, :n_sin] and the V half of g_vmix: columns [0, w_off) =
 *     g_ctx[n_sin + f] V[m, f] / ||V_f|| (exactly 0 where the norm is 0, torch.norm's subgradient), zeros past n_vout.
 *   Together the two write every element of g_vmix. */
int gn_geb_gate_backward(const float* g_s_out, int ldgs, const float* g_v_out, int ldgo, const float* x, int ldx,
                         int n_sout, int n_vout, const float* vmix, int ldv, int w_off, int N, int sact,
                         float* g_x, int ldgx, float* g_vmix, int ldgv, void* stream);
int gn_geb_context_backward(const float* g_ctx, int ldc, int n_sin, const float* vmix, int ldv, int n_vout, int w_off,
                            int N, float* g_s, int lds, float* g_vmix, int ldgv, void* stream);
/* Dipole: d_b recomputed in the forward's order; g_d = g_y[b] d_b / |d_b| (magnitude; 0 where |d_b| = 0) or g_y[b, :];
 * g_mu[n, m] = g_d[m] + g_yvec[b, m] (g_yvec may be NULL), g_q[n] = scale sum_m g_d[m] pos[n, m] (scale applies
 * when standardise). */
int gn_dipole_reduce_backward(const float* g_y, const float* g_yvec, const float* mu, int ldm, const float* q, int ldq,
                              const float* pos, const int* mol_ptr, int n_mol, float scale, float shift,
                              int standardise, int magnitude, float* g_mu, int ldgm, float* g_q, int ldgq,
                              void* stream);
/* ElectronicSpatialExtentV2: u[n] = g_y[b] |pos_n - c_b|^2 with the centroid computed as in gn_ese_reduce. */
int gn_ese_reduce_backward(const float* g_y, const float* pos, const int* z, const float* mass, int n_mass,
                           const int* mol_ptr, int n_mol, float* u, void* stream);

/* ---- adjacent: radius graph (Distance.forward, layers.py:1588-1604) ----------------------- */
/* torch_cluster.radius_graph(pos, r, batch, loop=True, max_num_neighbors) semantics: edges j->i with
 * ||pos_j - pos_i||^2 < cutoff^2 (fp32) inside one molecule (batch sorted, int64), target-major,
 * sources ascending, first max_nbr sources per target.  Pass 1 counts deg[i]; the caller scans it
 * into rowptr[N+1] (int64) and sizes the outputs; pass 2 writes edge_index int64 [2,E],
 * edge_vec = pos[j]-pos[i] [E,3] and edge_diff [E] (norm; 0 on self-loops). */
int gn_radius_count(const float* pos, const int64_t* batch, int N, float cutoff, int max_nbr,
                    int* deg, void* stream);
int gn_radius_fill(const float* pos, const int64_t* batch, int N, float cutoff, int max_nbr,
                   const int64_t* rowptr, int64_t E, int64_t* edge_index, float* edge_vec,
                   float* edge_diff, void* stream);
/* Edge vectors of a FIXED edge list for new positions (static-topology MD steps replayed from a hipGraph; the
 * arithmetic of Distance.forward, layers.py:1593-1600):
 * edge_vec[e] = pos[src[e]] - pos[dst[e]], edge_diff[e] = |edge_vec[e]| (0 on self-loops); the arithmetic of
 * gn_radius_fill, so a replayed step is bit-identical to an eager one on the same edge list. */
int gn_edge_vectors(const float* pos, const int* src, const int* dst, int E, float* edge_vec, float* edge_diff,
                    void* stream);

/* ---- periodic boundary conditions: radius graph, fixed-list edge vectors, virial ---------------------------------
 * Conventions: `cell` is fp32 [n_mol, 3, 3], its ROWS are the lattice vectors a, b, c, one cell per entry of `batch` (a
 * "molecule" is a periodic box); `edge_shift` is int32 [E, 3]; edge_vec[e] = pos[j] - pos[i] + edge_shift[e] @ cell[batch[i]].
 * gn_radius_count_pbc / gn_radius_fill_pbc look at the minimum image only: every perpendicular width V / |a_j x a_k| of every
 * cell must be at least 2 * cutoff (checked by the caller on the host: graph.check_cell); narrower cells go to the *_images
 * entry points below.  Each pair then has at most one image inside the cutoff, the one whose fractional
 * coordinates all lie in (-1/2, 1/2): n_k = rintf(d . column k of inv_cell), d = pos[j] - pos[i], shift = -n.  No atom sees
 * an image of itself; the self-loop (i, i, shift 0) stays, with edge_diff = 0.  Positions need not be wrapped into the cell.
 * One device helper computes v = d + shift @ cell (fmaf in the order a, b, c) and |v|^2 (x, y, z) for the count, the fill
 * and the fixed-list kernel: the three agree bit for bit.  mol_ptr [n_mol + 1] is gn_molecule_ptr's; batch entries outside
 * [0, n_mol) are clamped (a wrong list, never an out-of-bounds access). */
/* inv_cell [n_mol, 3, 3] = cell^-1 and volume [n_mol] = |det cell|, one thread per box (on the device, so a recorded step
 * follows a changing cell). */
int gn_cell_prepare(const float* cell, int n_mol, float* inv_cell, float* volume, void* stream);
/* The neighbour rule of gn_radius_count / gn_radius_fill (target-major, sources ascending, strict d^2 < r^2 in fp32, the
 * first max_nbr sources in source order, the self-loop counts against the cap) over the minimum images of a box's atoms.
 * One wave64 per target: ballot + prefix popcount give each hit its slot, a running count applies the cap; deterministic,
 * no atomics.  The fill also writes edge_shift. */
int gn_radius_count_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                        const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, int* deg, void* stream);
int gn_radius_fill_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                       const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, const int64_t* rowptr,
                       int64_t E, int64_t* edge_index, int* edge_shift, float* edge_vec, float* edge_diff, void* stream);
/* Several images per pair: cells narrower than 2 * cutoff, where a pair has more than one image inside the cutoff and an atom
 * sees images of itself.  The rule above, extended: within a (target, source) pair the images ascend lexicographically in
 * (sx, sy, sz) -- a lattice vector added to both atoms moves every image of the pair alike, so wrapping does not change
 * the order; the first max_nbr hits of a target in (source, image) order are kept.  The self-loop is the edge j == i with
 * shift 0: always a hit, inside the cap, edge_diff exactly 0.  An atom's own image (j == i, shift != 0) is an ordinary edge
 * with edge_diff = sqrtf(d^2) > 0.  d^2 comes from the helper the minimum-image and the fixed-list kernels use: a stored and a
 * searched shift give the same bits, and on cells of width >= 2 * cutoff the list is gn_radius_fill_pbc's, bit for bit.
 * img_range int32 [n_mol, 3]: R_k per box and axis; the candidates of a pair are s_k = -rintf(f_k) + t_k, t_k in [-R_k, R_k],
 * f = d @ inv_cell.  An image inside the cutoff has |(f_k + s_k) w_k| < cutoff (w_k: perpendicular width), and
 * |f_k - rint(f_k)| <= 1/2, so |t_k| < cutoff / w_k + 1/2: the caller passes R_k = floor(cutoff / w_k + 1/2 + slack), computed
 * in fp64, the slack covering the fp32 error of f (graph.image_ranges: 1/64).  R_k > GN_PBC_MAX_IMAGE_RANGE (a width below
 * about cutoff / 3) is for the caller to refuse; the kernel clamps it.  One wave64 per target over the flattened
 * (source, image) candidates; ballot + prefix popcount + a running count, no atomics: deterministic.  Count and fill are
 * one templated body. */
#define GN_PBC_MAX_IMAGE_RANGE 3      /* at most 7^3 = 343 images per pair */
int gn_radius_count_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                               const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff, int max_nbr,
                               int* deg, void* stream);
int gn_radius_fill_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                              const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff, int max_nbr,
                              const int64_t* rowptr, int64_t E, int64_t* edge_index, int* edge_shift, float* edge_vec,
                              float* edge_diff, void* stream);
/* gn_edge_vectors for a periodic list: the stored shift, no image search; the arithmetic of gn_radius_fill_pbc.  edge_diff
 * is exactly 0 on the self-loop (j == i and shift 0) only. */
int gn_edge_vectors_pbc(const float* pos, const int* src, const int* dst, const int* shift, const float* cell,
                        const int64_t* batch, int E, int n_mol, float* edge_vec, float* edge_diff, void* stream);
/* out[m] (3 x 3, row-major) = (1 / volume[m]) sum_{e in box m} r_e (x) dE/dr_e with dE/dr_e = g_vec[e] + g_diff[e] r_e / |r_e|
 * (second term when g_diff != 0: gn_pos_scatter's expression) = (1/V) dE/d(strain), ASE's sign, not symmetrised.  Box m
 * covers the edges rowptr[mol_ptr[m]] .. rowptr[mol_ptr[m + 1]] of a target-major list.  One workgroup per box, fixed-order
 * sums, no atomics: identical inputs give identical bits; an empty box gives zeros. */
int gn_virial(const float* g_vec, const float* g_diff, const float* edge_vec, const int* rowptr, const int* mol_ptr,
              int n_mol, const float* volume, float* out, void* stream);
/* Is a stored list still the radius graph of these positions?  One entry per search (gn_radius_count, _pbc, _pbc_images),
 * with that search's arguments plus the stored list in the engine's CSR form: rowptr int32 [N + 1], src int32 [E] (and
 * shift int32 [E, 3]) of a target-major list, as gn_build_csr writes them.  Every target walks its search's candidates in
 * the search's order through the search's own device predicates, so the verdict at the threshold is the rebuilt list's, bit
 * for bit: hit number k (k < max_nbr; the self-loop counts) must be stored entry k of the row -- source, and shift -- and
 * the number of kept hits must be the row's degree.  Thread mapping as the searches (a thread / a wave64 per target).
 * Outputs: row_flag int32 [N] (work: 1 where the row differs), changed int32 [n_mol] = flagged targets per molecule
 * (mol_ptr [n_mol + 1] of gn_molecule_ptr; a wave per molecule, integer count), and the STICKY word state[0], set to 1 by
 * plain stores when any row differs and never cleared on the device (the gn_md_* kernels below are predicated on it; the
 * host clears it).  Stored indices are read inside [0, E) only, whatever rowptr holds. */
int gn_radius_verify(const float* pos, const int64_t* batch, const int* mol_ptr, int N, int n_mol, float cutoff,
                     int max_nbr, const int* rowptr, const int* src, int E, int* row_flag, int* changed, int* state,
                     void* stream);
int gn_radius_verify_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                         const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, const int* rowptr,
                         const int* src, const int* shift, int E, int* row_flag, int* changed, int* state, void* stream);
int gn_radius_verify_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff, int max_nbr,
                                const int* rowptr, const int* src, const int* shift, int E, int* row_flag, int* changed,
                                int* state, void* stream);
/* Edge lists with self-images (the *_images radius graph): the five kernels that single out the self-loop -- the unit-vector
 * normalisation of gn_edge_geometry, the NodeInit sum and its backward, gn_edge_geometry_backward, the neighbour-embedding
 * gradient -- tell it by `src == dst AND edge_diff == 0` instead of `src == dst`.  On a list without self-images the two rules
 * pick the same edges and the results are the same bits.  Same arguments as the entry points they are named after, plus
 * edge_diff [E] where those do not receive it. */
int gn_edge_geometry_images(const float* edge_vec, const float* edge_diff, const int* src, const int* dst, int E,
                            int lmax, int R, int basis, const float* means, const float* betas, float cutoff,
                            float* rl, float* phi, float* cut, void* stream);
int gn_node_init_images(const int* z, const int* rowptr, const int* src, const float* feat, int ldf, const float* cut,
                        const float* A_na, const float* A_nbr, int N, int F, const float* edge_diff, float* ctx, void* stream);
int gn_node_init_backward_images(const float* g_ctx, const int* z, const float* feat, int ldf, const float* cut,
                                 const float* A_nbr, const int* rowptr, const int* src, int N, int F,
                                 const float* edge_diff, float* g_feat, float* g_cut, void* stream);
int gn_edge_geometry_backward_images(const float* edge_vec, const float* edge_diff, const int* src, const int* dst,
                                     int E, int lmax, int R, int basis, const float* means, const float* betas,
                                     float cutoff, const float* g_rl, int n_rl, const float* g_cut, int n_cut,
                                     const float* g_phi, float* g_vec, float* g_diff, void* stream);
int gn_embedding_grad_images(const float* g_ctx, const float* feat, int ldf, const float* cut, const int* dst,
                             const int* colptr, const int* perm, const int* order, const int* sp_ptr, int n_species,
                             int N, int F, const float* edge_diff, float* work, float* dA_na, float* dA_nbr, void* stream);

/* ---- molecular dynamics: the integrator around a recorded energy + force step (gotennet_amd/md.py) ---------------
 * state int32 [2]: state[0] the sticky stale-list word of gn_radius_verify*, state[1] the number of completed steps.
 * Every kernel below reads state[0] first and does NOTHING when it is set (gn_md_kick / _drift / _kinetic accept
 * state == NULL: never frozen): a replay on a stale list moves no atom, velocity, counter or log row.  mass fp32 [n_mass]
 * is indexed by the atomic number z int32 [N]; an atom whose z is outside the table or whose mass is not positive is left
 * alone (the caller refuses such inputs).  No atomics, fixed-order sums: identical inputs give identical bits. */
/* vel += s * force / mass[z]  (s = dt / 2 * force_scale, rounded once on the host) */
int gn_md_kick(float* vel, const float* force, const int* z, const float* mass, int n_mass, int N, float s,
               const int* state, void* stream);
/* pos += dt * vel */
int gn_md_drift(float* pos, const float* vel, int N, float dt, const int* state, void* stream);
/* The noise: xi(key, step, draw, atom, component) is a pure function, independent of the launch geometry.  One
 * Philox4x32-10 evaluation per (atom, pair) with counter (atom, pair + 2 * draw, step, lo32(key[1])) and key
 * (lo32(key[0]), hi32(key[0])); u1, u2 = ((word0 >> 8) + 1) * 2^-24, ((word1 >> 8) + 1) * 2^-24, uniform in (0, 1];
 * Box-Muller r = sqrtf(-2 logf(u1)), t = 2 pi u2: pair 0 gives the components x = r cosf(t), y = r sinf(t), pair 1 gives
 * z = r cosf(t).  `key` is a DEVICE pointer to two int64 values, `draw` numbers the draws inside one step (the two
 * Langevin halves of md.MDRun are draws 0 and 1), step is 32 bits wide.
 * gn_md_langevin: the O step vel = c1 * vel + c2 * sqrtf(1 / mass[z]) * xi with step = state[1]; the host passes
 * c1 = exp(-gamma h), c2 = sqrt(kT force_scale (1 - c1^2)) computed in fp64.  gn_md_noise: out [N, 3] = xi. */
int gn_md_langevin(float* vel, const int* z, const float* mass, int n_mass, int N, float c1, float c2,
                   const long long* key, int draw, const int* state, void* stream);
int gn_md_noise(const long long* key, long step, int draw, int N, float* out, void* stream);
/* ke[m] = (1/2) sum_{a in molecule m} mass[z_a] |vel_a|^2 / force_scale: one workgroup per molecule, fixed-order sums. */
int gn_md_kinetic(const float* vel, const int* z, const float* mass, int n_mass, const int* mol_ptr, int N, int n_mol,
                  float force_scale, float* ke, const int* state, void* stream);
/* End of a step (one workgroup): with k = state[1], row k % log_len of log [log_len, n_mol, 2] receives (energy[m], ke[m]),
 * force [N, 3] / energy [n_mol] / stress [n_mol, 9] (NULL: none) are copied into their *_keep buffers -- what the next
 * kick reads and what the host reads, whatever a later stale replay leaves in the step's own outputs -- and state[1] = k + 1. */
int gn_md_finish(int* state, const float* force, float* force_keep, int N, const float* energy, const float* ke,
                 float* energy_keep, const float* stress, float* stress_keep, float* log, int log_len, int n_mol,
                 void* stream);
/* Constant pressure: isotropic stochastic cell rescaling in eps = ln V (Bernetti and Bussi, J. Chem. Phys. 153, 114107,
 * 2020), one move per step, predicated on state[0] like the kernels above.  reason int32 [n_mol] says why a box stopped
 * the run (plain stores of one value, never cleared on the device): 1 = the moved cell no longer satisfies the search
 * parameters, 2 = a move beyond max_step.
 * gn_npt_pressure, one thread per box: pressure[m] = 2 ke[m] / (3 volume[m]) - trace(stress[m]) / 3 (stress [n_mol, 9] =
 * (1/V) dE/d(strain), tensile positive: gn_virial's), formed in fp64 and rounded once; with k = state[1], row k % log_len of
 * log [log_len, n_mol, 2] receives (volume[m], pressure[m]) (log NULL or state NULL: no row; state NULL: never frozen).
 * Launched before gn_md_finish moves the counter. */
int gn_npt_pressure(const float* ke, const float* stress, const float* volume, int n_mol, float* pressure, float* log,
                    int log_len, const int* state, void* stream);
/* gn_npt_barostat, one workgroup, a thread per box, fp64 from the fp32 inputs:
 *   d_eps = -(beta / tau) (p0 - pressure[m]) dt + sqrt(2 kT beta dt / (volume[m] tau)) xi,
 * xi = the first normal of the noise above with atom = m, pair 0, draw 2, step = state[1] (gn_md_noise(key, step, 2,
 * n_mol)[:, 0]); kT == 0 is the deterministic weak-coupling limit and `key` (a DEVICE pointer, as above) is not read.
 * s[m] = fp32(exp(d_eps / 3)), inv_s[m] = fp32(1 / exp(d_eps / 3)), and the nine entries of cell[m] are multiplied by s[m] in
 * fp32.  If some box's d_eps is not finite or |d_eps| > max_step, reason[m] = 2 for every such box, state[0] = 1 and
 * NOTHING else is written for any box.  Reads none of pos / vel / force: where in the step it runs before gn_npt_rescale
 * does not change a bit. */
int gn_npt_barostat(float* cell, const float* volume, const float* pressure, int n_mol, double p0, double beta, double tau,
                    double dt, double kT, double max_step, const long long* key, float* s, float* inv_s, int* state,
                    int* reason, void* stream);
/* pos[a] *= s[batch[a]], vel[a] *= inv_s[batch[a]] in fp32, one thread per component (batch entries clamped to
 * [0, n_mol)); state NULL: never frozen. */
int gn_npt_rescale(float* pos, float* vel, const int64_t* batch, const float* s, const float* inv_s, int N, int n_mol,
                   const int* state, void* stream);
/* gn_npt_cell_guard, one thread per box, fp64: the perpendicular widths w_k = V / |a_i x a_j| of cell[m] against the search
 * parameters in use -- img_range NULL (the minimum-image kernels): every w_k >= 2 cutoff; else
 * floor(cutoff / w_k + 1/2 + 2^-6) <= img_range[m, k] -- and the volume finite and non-zero.  A violation stores
 * reason[m] = 1 and state[0] = 1. */
int gn_npt_cell_guard(const float* cell, int n_mol, double cutoff, const int* img_range, int* state, int* reason,
                      void* stream);
/* gn_cell_image_ranges, one workgroup, a thread per box, fp64, the guard's widths: the image ranges of the moved cell for a
 * search that is rebuilt inside the step (pipeline.RebuiltStep(cell_moves=True)), launched behind gn_cell_prepare and in
 * front of gn_radius_count_pbc_images.  img_range[m, k] = floor(cutoff / w_k + 1/2 + 2^-6) (graph.image_ranges' rule).  A box
 * whose volume is zero or not finite, or with some R_k > max_range (at most GN_PBC_MAX_IMAGE_RANGE), keeps its row of
 * img_range and stores reason[m] = 1 and state[0] = 1; the other boxes of that launch are written.  state[0] != 0 on
 * entry: nothing is written.  (R_k <= 3 holds down to w_k = cutoff / (3.5 - 2^-6), a little below the cutoff / 3 at which the
 * host's graph.image_ranges refuses: the range is what the search needs, the host's bound is the round one.) */
int gn_cell_image_ranges(const float* cell, int n_mol, double cutoff, int max_range, int* img_range, int* state,
                        int* reason, void* stream);

/* ---- FIRE relaxation around a recorded energy + force step (gotennet_amd/relax.py; Bitzek et al., PRL 97, 170201, the
 * variant ASE's FIRE implements, unit masses) ----------------------------------------------------------------------
 * `state` is the pair above; plan, move and finish read state[0] first and do NOTHING when it is set.  Per-molecule state,
 * caller-allocated, [n_mol] each: dt fp32 (time step), alpha fp32 (mixing coefficient), n_pos int32 (steps since the last
 * P <= 0; -1: no step taken yet), status int32 (0 active, 1 converged, 2 a force that is not finite; 1 and 2 are sticky on
 * the device), converged_at int32 (state[1] when the status left 0; -1 until then).  fixed uint8 [N] (NULL: none) marks
 * frozen atoms: their force counts as zero in every reduction and they never move.  mol_ptr int32 [n_mol + 1] of
 * gn_molecule_ptr; every index derived from it is clamped to [0, N].  One workgroup of 256 threads per molecule (finish: one
 * workgroup), no atomics, fixed-order sums, plain stores: identical inputs give identical bits. */
/* out[m] = max over the free atoms of |force_a| (|f|^2 accumulated x, y, z in fp32, then sqrtf); 0 for an empty molecule. */
int gn_fire_fmax(const float* force, const unsigned char* fixed, const int* mol_ptr, int N, int n_mol, float* out,
                 void* stream);
/* The decision of step k = state[1], from the KEPT forces and the velocities.  Over the free atoms: P = sum f.v,
 * ff = sum |f|^2, vv = sum |v|^2 in fp64 from the fp32 inputs (products included), fm2 = max |f_a|^2 as gn_fire_fmax forms
 * it.  Every molecule writes row k % log_len of log [log_len, n_mol, 2] = (energy_keep[m], sqrtf(fm2)): the state BEFORE the
 * move of step k (log NULL or log_len 0: no row).  A molecule whose status is not 0 writes coef[m][3] = 0 and nothing else.
 * Otherwise: fm2 not finite -> status 2, converged_at = k, no move;  fm2 <= fmax^2 (compared in fp64) -> status 1,
 * converged_at = k, no move;  n_pos < 0 -> n_pos = 0, c_v = 1, c_f = 0;  P > 0 -> c_v = 1 - alpha, c_f = alpha sqrt(vv / ff)
 * with the OLD alpha, then, if n_pos > n_min, dt = min(dt f_inc, dt_max) and alpha *= f_alpha, then n_pos += 1;  else
 * c_v = c_f = 0, alpha = alpha_start, dt *= f_dec, n_pos = 0.  coef fp32 [n_mol, 4] = {c_v, c_f, dt, active (1 or 0)}, every
 * number formed in fp64 and rounded once. */
int gn_fire_plan(const float* force, const float* vel, const unsigned char* fixed, const int* mol_ptr, int N, int n_mol,
                 double fmax, double dt_max, int n_min, double f_inc, double f_dec, double alpha_start, double f_alpha,
                 float* dt, float* alpha, int* n_pos, int* status, int* converged_at, float* coef,
                 const float* energy_keep, float* log, int log_len, const int* state, void* stream);
/* The move of the molecules with coef[m][3] != 0: per free component vel = fmaf(dt, f, fmaf(c_f, f, c_v * vel)) in fp32; the
 * squared length of the displacement sum (dt vel)^2 over the molecule in fp64; scale = fp32(min(1, max_step / length));
 * pos += scale * (dt * vel) in fp32.  The clamp acts on the displacement of the whole molecule, not on the velocity. */
int gn_fire_move(float* pos, float* vel, const float* force, const unsigned char* fixed, const int* mol_ptr, int N,
                 int n_mol, const float* coef, double max_step, const int* state, void* stream);
/* End of a step (one workgroup): state[1] += 1, and force [N, 3] / energy [n_mol] / stress [n_mol, 9] (NULL: none) are
 * copied into their *_keep buffers for the molecules whose status is 0 (batch int64 [N], entries clamped to [0, n_mol)): a
 * frozen molecule keeps the values it was judged on. */
int gn_fire_finish(int* state, const int* status, const int64_t* batch, const float* force, float* force_keep, int N,
                   const float* energy, float* energy_keep, const float* stress, float* stress_keep, int n_mol,
                   void* stream);

/* ---- variable-cell relaxation: FIRE over the atoms and the cell of every periodic box (gotennet_amd/relax.py, CellRelax;
 * ASE's UnitCellFilter for row vectors) ---------------------------------------------------------------------------------
 * Per box m: the reference cell cell0[m] (the start), the deformation gradient F, the reference coordinates x~;
 * pos = x~ F, cell = cell0 F.  The extended arrays x_ext / g_ext fp32 [N + 3 n_mol, 3] hold, for box m, rows
 * [mol_ptr[m] + 3 m, mol_ptr[m + 1] + 3 (m + 1)): its atom rows (x~; the generalised forces on them), then three cell rows
 * (U = weight[m] F; the generalised forces G on them), so gn_fire_plan and gn_fire_move run on them with
 * mol_ptr_ext[m] = mol_ptr[m] + 3 m as on molecules of n_m + 3 atoms.  mol_ptr int32 [n_mol + 1] is the REAL one; every index
 * derived from it is clamped to [0, N].  weight fp32 [n_mol] > 0.  One workgroup of 256 threads per box, fp64 from the fp32
 * inputs, every stored value rounded once, plain stores in a fixed order: identical inputs give identical bits.  `state` is
 * the pair above: both read state[0] first and do NOTHING when it is set. */
/* g_ext of the kept force [N, 3] and stress [n_mol, 9] (sigma = (1/V) sum r (x) dE/dr, not symmetrised) at the current cell
 * [n_mol, 9], F = cell rows of x_ext / weight:  atom rows g_ai = sum_j F_ij f_aj (0 for an atom of fixed uint8 [N], NULL:
 * none);  cell rows G = -(V / weight) F^-T S with V = |det cell| and S = (sigma + sigma^T) / 2 + pressure I, with
 * hydrostatic != 0 S <- (tr S / 3) I, and then exactly 0 where cell_mask uint8 [9] (NULL: all ones) is 0.  That is
 * -dH/d(x~, U) of H = E + pressure V.  A stress that is not finite gives cell rows that are not finite. */
int gn_cellrelax_forces(const float* force, const float* stress, const float* cell, const float* x_ext, const float* weight,
                        double pressure, int hydrostatic, const unsigned char* cell_mask, const unsigned char* fixed,
                        const int* mol_ptr, int N, int n_mol, float* g_ext, const int* state, void* stream);
/* Behind gn_fire_move on x_ext: a box with coef[m][3] == 1 (gn_fire_plan's) reads F from its moved cell rows and writes
 * pos = x~ F for every one of its atoms, fixed ones included, and cell[m] = cell0[m] F; any other box writes nothing. */
int gn_cellrelax_apply(const float* x_ext, const float* cell0, const float* weight, const float* coef, const int* mol_ptr,
                       int N, int n_mol, float* pos, float* cell, const int* state, void* stream);

/* ---- nudged elastic band on the batched FIRE step (gotennet_amd/neb.py; improved tangent of Henkelman and Jonsson,
 * J. Chem. Phys. 113, 9978) ---------------------------------------------------------------------------------------------
 * Molecules b n_img .. (b + 1) n_img - 1 are the images of band b (n_img >= 3, n_mol a multiple of n_img); atom a of an
 * image pairs with the atom at the same offset from mol_ptr in the two neighbouring images.  gn_fire_plan and gn_fire_move
 * run unchanged on g_out with a band pointer (every n_img-th entry of mol_ptr) and per-band state.  `state` is the pair
 * above: both entries read state[0] first and do NOTHING when it is set.  No atomics, fixed-order fp64 sums from the fp32
 * inputs (products included), plain stores: identical inputs give identical bits. */
/* g_out fp32 [N, 3] from the positions, the KEPT force [N, 3] and the KEPT energy [n_mol]; one workgroup of 256 per image.
 * Interior image i, t+ = R_{i+1} - R_i, t- = R_i - R_{i-1}, the fp32 energies compared as they are:  E+ > E > E-: t = t+;
 * E+ < E < E-: t = t-;  otherwise dmax / dmin = the larger / smaller of |E+ - E|, |E- - E| and t = dmax t+ + dmin t- when
 * E+ > E-, else (ties included) t = dmin t+ + dmax t-.  All sums run over the free atoms (fixed uint8 [N], NULL: none).
 * g = f - (f.t / |t|^2) t + k (|t+| - |t-|) t / |t|;  the climbing image (climb != 0: the interior image with the largest
 * energy, the first of equal ones) gets g = f - 2 (f.t / |t|^2) t;  |t|^2 == 0: g = f;  one of the three energies not
 * finite: g = NaN.  Rows of the two end images, of fixed atoms and of atoms beyond the shortest of the three images: 0.
 * The workgroup of a band's first image writes e_band_out[b] (the largest energy of the band, a NaN wins) and climb_out[b]
 * (the climbing image's index in the band, -1 when climb == 0).  k finite and >= 0. */
int gn_neb_forces(const float* pos, const float* force, const float* energy, const unsigned char* fixed, const int* mol_ptr,
                  int N, int n_mol, int n_img, double k, int climb, float* g_out, float* e_band_out, int* climb_out,
                  const int* state, void* stream);
/* gn_fire_finish with status int32 [n_mol / n_img] indexed per band: state[1] += 1, and force / energy / stress are copied
 * into their *_keep buffers for the images m with status[m / n_img] == 0. */
int gn_neb_finish(int* state, const int* status, const int64_t* batch, const float* force, float* force_keep, int N,
                  const float* energy, float* energy_keep, const float* stress, float* stress_keep, int n_mol, int n_img,
                  void* stream);

/* ---- parameter gradients (first-order training: a loss on energies and / or (h, X)) -------------
 * Every reduction below runs in a fixed order and uses no atomics: identical inputs give identical bits. */
/* dW = dY^T A and db = sum_r dY of a Dense product y = A W^T + b (layers.py:457-529): several independent problems in
 * one launch.  dW[n * ldw + k] = sum_{r < rows} dY[row(r), y_off + n] A[row(r), a_off + k] and, when db != NULL,
 * db[n] = sum_r dY[row(r), y_off + n]; row(r) = (r / row_cnt) * row_gstride + row_goff + r % row_cnt is the row map of
 * gn_gemm_desc and addresses both operands (per-degree W_vk_l rows of X [N, D, F]; (1, 1, 0) = every row).  Any
 * rows >= 0 (0 writes zeros), nout >= 1, K >= 1.  Exact fp32 (v_mfma_f32_32x32x2_f32, fp32 accumulation) whatever
 * the projection arithmetic of the model: both operands are run-time activations.  The rows are split across
 * workgroups by the problem shape alone; the partial tiles go to the caller's workspace (gn_weight_grad_workspace
 * floats for the same problems) and are summed in split order; dW and db are overwritten. */
typedef struct gn_wgrad_desc {
    const float* dY; int ldy; int y_off;
    const float* A; int lda; int a_off;
    float* dW; int ldw;
    float* db;
    int rows, nout, K;
    int row_cnt, row_gstride, row_goff;
} gn_wgrad_desc;
long gn_weight_grad_workspace(const gn_wgrad_desc* problems, int n);
int gn_weight_grad_group(const gn_wgrad_desc* problems, int n, float* work, long work_floats, void* stream);
/* The same problems in a chosen arithmetic.  mode GN_WGRAD_F32 (0) forwards to the two entries above: same launches,
 * same bits.  mode GN_WGRAD_F16X2 (2, numbered like the `split` argument of the projection launcher): each operand as
 * two fp16 planes scaled by power-of-two exponents -- one per 32-column block and side, the running maximum along the
 * rows, accumulators rescaled when it grows -- and three v_mfma_f32_32x32x16_f16 per product (hi*hi + hi*lo + lo*hi,
 * fp32 accumulation) on a 128 (nout) x 256 (K) workgroup tile; an all-zero block gives exact zeros; db stays a plain
 * fp32 column sum.  Same descriptor contract, same partial-sum workspace layout and in-order reduction (no atomics in
 * global memory: identical inputs give identical bits); the row split, and so the workspace size, depends on the mode.
 * Any other mode: gn_weight_grad_group_mode returns GN_ERR_BAD_ARG, gn_weight_grad_workspace_mode -1. */
#define GN_WGRAD_F32 0
#define GN_WGRAD_F16X2 2
long gn_weight_grad_workspace_mode(const gn_wgrad_desc* problems, int n, int mode);
int gn_weight_grad_group_mode(const gn_wgrad_desc* problems, int n, int mode, float* work, long work_floats, void* stream);
/* Embedding gradients of NodeInit (layers.py:1658-1675; gotennet.py:969-975):
 * dA_na[s] = sum_{i: z_i = s} g_ctx[i, 0:F] (row 0, the padding_idx, is zero);
 * dA_nbr[s] = sum over the non-self-loop edges e = (j -> i) with z_j = s of g_ctx[i, F:2F] feat[e, 0:F] cut[e]: first per
 * source atom j over the by-source view (colptr / perm of gn_build_csc, into work [N, F]), then per species.
 * order [N]: a stable argsort of z; sp_ptr [n_species + 1]: the first sorted position of each species (host plumbing).
 * Species without atoms get zero rows, sources without out-edges zero rows of work.  dA_na and dA_nbr are plain
 * stores, not accumulations: N = 0 still writes both as zeros (sp_ptr is read).  GN_ERR_BAD_ARG before any launch:
 * N < 0, F < 1, n_species < 1, ldf < 2 F, sp_ptr, dA_na or dA_nbr NULL, and -- once N > 0 -- any other pointer NULL
 * (edge_diff of the _images variant stays optional: NULL = every src == dst edge is a self-loop). */
int gn_embedding_grad(const float* g_ctx, const float* feat, int ldf, const float* cut, const int* dst,
                      const int* colptr, const int* perm, const int* order, const int* sp_ptr, int n_species,
                      int N, int F, float* work, float* dA_na, float* dA_nbr, void* stream);
/* LayerNorm affine gradients (layers.py:518-529, gotennet.py:315, 397): dgamma[c] = sum_r g_z[r,c] x_hat[r,c],
 * dbeta[c] = sum_r g_z[r,c] with g_z = g_out * act'(x_hat gamma + beta) (act: the activation after the norm, as in
 * gn_layernorm_silu; GN_ACT_NONE for a bare nn.LayerNorm).  x [N, C] is the un-normalised input.  Two stages: 64-row
 * partials in work (gn_layernorm_param_grad_workspace floats), then a column sum in chunk order. */
long gn_layernorm_param_grad_workspace(int N, int C);
int gn_layernorm_param_grad(const float* x, const float* gamma, const float* beta, float eps, const float* g_out,
                            int N, int C, int act, float* work, float* dgamma, float* dbeta, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* GOTENNET_HIP_H */
