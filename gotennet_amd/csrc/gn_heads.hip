// gn_heads.hip -- the two vector-representation read-outs the reference's QM9 task builds on top of the path
// (models/tasks/QM9Task.py:168-187): Dipole (outputs.py:379-468: two GatedEquivariantBlocks, outputs.py:24-93) and
// ElectronicSpatialExtentV2 (outputs.py:471-545).  Node-local and tiny next to the interaction layers (a few [N,F]
// rows per atom): plain one-thread-per-element kernels, per-molecule sums in a fixed order (one workgroup per molecule,
// wave-level butterflies: no atomics).  The GEMMs of the blocks go through gn_gemm like every other projection.
#include "gn_common.h"

namespace gn {

// GatedEquivariantBlock, first half (outputs.py:78-82):  ctx = [scalars | ||V||_2 over the 3 components | 0-padding]
// vmix [N*3, ldv] holds mix_vectors(vectors): V at column 0, W at column w_off (each n_vout wide).
__global__ void geb_context_kernel(const float* __restrict__ s, int lds, int n_sin, const float* __restrict__ vmix,
                                   int ldv, int n_vout, int N, float* __restrict__ ctx, int ldc) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * ldc) return;
    const int n = (int)(idx / ldc), c = (int)(idx % ldc);
    float v = 0.f;
    if (c < n_sin) {
        v = s[(size_t)n * lds + c];
    } else if (c < n_sin + n_vout) {
        const int f = c - n_sin;
        const float a = vmix[((size_t)n * 3 + 0) * ldv + f], b = vmix[((size_t)n * 3 + 1) * ldv + f],
                    d = vmix[((size_t)n * 3 + 2) * ldv + f];
        v = sqrtf(a * a + b * b + d * d);            // torch.norm(vectors_V, dim=-2)
    }
    ctx[idx] = v;
}

// second half (outputs.py:84-91):  x = scalar_net(ctx) = [s_out | gate];  v_out = gate * W;  s_out = sactivation(s_out)
__global__ void geb_gate_kernel(const float* __restrict__ x, int ldx, int n_sout, int n_vout,
                                const float* __restrict__ vmix, int ldv, int w_off, int N, int sact,
                                float* __restrict__ s_out, int lds, float* __restrict__ v_out, int ldo) {
    const int per = n_sout + 3 * n_vout;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * per) return;
    const int n = (int)(idx / per), c = (int)(idx % per);
    if (c < n_sout) {
        const float v = x[(size_t)n * ldx + c];
        s_out[(size_t)n * lds + c] = sact < 0 ? v : act1(v, sact);
    } else {
        const int m = (c - n_sout) / n_vout, f = (c - n_sout) % n_vout;
        v_out[((size_t)n * 3 + m) * ldo + f] = x[(size_t)n * ldx + n_sout + f] * vmix[((size_t)n * 3 + m) * ldv + w_off + f];
    }
}

// Dipole read-out (outputs.py:449-468), one workgroup per molecule:
//   y_b = sum_n ( mu_n + pos_n * q_n ),  q_n = stddev * s_n + mean (when standardised),  mu_n = v_n[:, 0]
//   y_vec_b = sum_n mu_n;  magnitude: |y_b|
__global__ __launch_bounds__(64) void dipole_reduce_kernel(
    const float* __restrict__ mu, int ldm, const float* __restrict__ q, int ldq, const float* __restrict__ pos,
    const int* __restrict__ mol_ptr, float scale, float shift, int standardise, int magnitude,
    float* __restrict__ y, float* __restrict__ y_vec) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = mol_ptr[b], n1 = mol_ptr[b + 1];
    float d[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
    for (int n = n0 + lane; n < n1; n += 64) {
        float c = q[(size_t)n * ldq];
        if (standardise) c = scale * c + shift;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float a = mu[((size_t)n * 3 + m) * ldm];
            v[m] += a;
            d[m] += a + pos[(size_t)n * 3 + m] * c;
        }
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) { d[m] = wave_sum(d[m]); v[m] = wave_sum(v[m]); }
    if (lane == 0) {
        if (magnitude) y[b] = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        else { y[3 * b] = d[0]; y[3 * b + 1] = d[1]; y[3 * b + 2] = d[2]; }
        if (y_vec) { y_vec[3 * b] = v[0]; y_vec[3 * b + 1] = v[1]; y_vec[3 * b + 2] = v[2]; }
    }
}

// ElectronicSpatialExtentV2 read-out (outputs.py:526-545), one workgroup per molecule:
//   c_b = sum_n m_n pos_n / sum_n m_n,   y_b = sum_n |pos_n - c_b|^2 x_n
__global__ __launch_bounds__(64) void ese_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ pos, const int* __restrict__ z,
    const float* __restrict__ mass, int n_mass, const int* __restrict__ mol_ptr, float* __restrict__ y) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = mol_ptr[b], n1 = mol_ptr[b + 1];
    float mp[3] = {0.f, 0.f, 0.f}, ms = 0.f;
    for (int n = n0 + lane; n < n1; n += 64) {
        const int zn = z[n];
        const float m = (zn >= 0 && zn < n_mass) ? mass[zn] : 0.f;
        ms += m;
#pragma unroll
        for (int k = 0; k < 3; ++k) mp[k] += m * pos[(size_t)n * 3 + k];
    }
    ms = wave_sum(ms);
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ms > 0.f ? wave_sum(mp[k]) / ms : 0.f;      // (massless molecule: rejected by the host; no 0 / 0 here)
    float s = 0.f;
    for (int n = n0 + lane; n < n1; n += 64) {
        const float dx = pos[(size_t)n * 3] - c[0], dy = pos[(size_t)n * 3 + 1] - c[1], dz = pos[(size_t)n * 3 + 2] - c[2];
        const float r = sqrtf(dx * dx + dy * dy + dz * dz);      // torch.norm(...) ** 2, as the reference writes it
        s += (r * r) * x[n];
    }
    s = wave_sum(s);
    if (lane == 0) y[b] = s;
}

// ---------------------------------------------------------------------------------------------- backward (training)
// Adjoint of geb_gate_kernel.  One thread per element of g_x [N, ldgx] and of the W half of g_vmix (columns
// [w_off, ldgv) of its 3 rows per atom); padding columns are written as zeros (the products that follow read whole rows).
//   g_x[:, c] = g_s_out[:, c] sact'(s_raw[:, c]);  g_x[:, n_sout + f] = sum_m g_v_out[m, f] W[m, f];
//   g_vmix[m, w_off + f] = gate_f g_v_out[m, f]
__global__ void geb_gate_backward_kernel(const float* __restrict__ g_s_out, int ldgs, const float* __restrict__ g_v_out,
                                         int ldgo, const float* __restrict__ x, int ldx, int n_sout, int n_vout,
                                         const float* __restrict__ vmix, int ldv, int w_off, int N, int sact,
                                         float* __restrict__ g_x, int ldgx, float* __restrict__ g_vmix, int ldgv) {
    const int wv = ldgv - w_off, per = ldgx + 3 * wv;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * per) return;
    const int n = (int)(idx / per), c = (int)(idx % per);
    if (c < ldgx) {
        float v = 0.f;
        if (c < n_sout) {
            v = g_s_out[(size_t)n * ldgs + c];
            if (sact >= 0) v *= dact1(x[(size_t)n * ldx + c], sact);
        } else if (c < n_sout + n_vout) {
            const int f = c - n_sout;
#pragma unroll
            for (int m = 0; m < 3; ++m)
                v += g_v_out[((size_t)n * 3 + m) * ldgo + f] * vmix[((size_t)n * 3 + m) * ldv + w_off + f];
        }
        g_x[(size_t)n * ldgx + c] = v;
    } else {
        const int m = (c - ldgx) / wv, f = (c - ldgx) % wv;
        float v = 0.f;
        if (f < n_vout) v = x[(size_t)n * ldx + n_sout + f] * g_v_out[((size_t)n * 3 + m) * ldgo + f];
        g_vmix[((size_t)n * 3 + m) * ldgv + w_off + f] = v;
    }
}

// Adjoint of geb_context_kernel.  g_s = g_ctx[:, :n_sin]; the V half of g_vmix (columns [0, w_off)):
//   g_vmix[m, f] = g_ctx[n_sin + f] V[m, f] / ||V_f||, exactly 0 where the norm is 0 (torch.norm's subgradient)
__global__ void geb_context_backward_kernel(const float* __restrict__ g_ctx, int ldc, int n_sin,
                                            const float* __restrict__ vmix, int ldv, int n_vout, int w_off, int N,
                                            float* __restrict__ g_s, int lds, float* __restrict__ g_vmix, int ldgv) {
    const int per = n_sin + 3 * w_off;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * per) return;
    const int n = (int)(idx / per), c = (int)(idx % per);
    if (c < n_sin) {
        g_s[(size_t)n * lds + c] = g_ctx[(size_t)n * ldc + c];
        return;
    }
    const int m = (c - n_sin) / w_off, f = (c - n_sin) % w_off;
    float v = 0.f;
    if (f < n_vout) {
        const float a = vmix[((size_t)n * 3 + 0) * ldv + f], b = vmix[((size_t)n * 3 + 1) * ldv + f],
                    d = vmix[((size_t)n * 3 + 2) * ldv + f];
        const float nrm = sqrtf(a * a + b * b + d * d);
        if (nrm > 0.f) v = g_ctx[(size_t)n * ldc + n_sin + f] * (m == 0 ? a : m == 1 ? b : d) / nrm;
    }
    g_vmix[((size_t)n * 3 + m) * ldgv + f] = v;
}

// Adjoint of dipole_reduce_kernel, one workgroup per molecule.  d_b is recomputed in the forward's order;
//   g_d = g_y d_b / |d_b| (magnitude; 0 where |d_b| = 0) or g_y[b];  g_mu[n] = g_d + g_yvec[b];
//   g_q[n] = scale sum_m g_d[m] pos[n, m]   (scale = 1 when the charges are not standardised)
__global__ __launch_bounds__(64) void dipole_reduce_backward_kernel(
    const float* __restrict__ g_y, const float* __restrict__ g_yvec, const float* __restrict__ mu, int ldm,
    const float* __restrict__ q, int ldq, const float* __restrict__ pos, const int* __restrict__ mol_ptr, float scale,
    float shift, int standardise, int magnitude, float* __restrict__ g_mu, int ldgm, float* __restrict__ g_q, int ldgq) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = mol_ptr[b], n1 = mol_ptr[b + 1];
    float gd[3];
    if (magnitude) {
        float d[3] = {0.f, 0.f, 0.f};
        for (int n = n0 + lane; n < n1; n += 64) {
            float c = q[(size_t)n * ldq];
            if (standardise) c = scale * c + shift;
#pragma unroll
            for (int m = 0; m < 3; ++m) d[m] += mu[((size_t)n * 3 + m) * ldm] + pos[(size_t)n * 3 + m] * c;
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) d[m] = wave_sum(d[m]);
        const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const float gy = g_y[b];
#pragma unroll
        for (int m = 0; m < 3; ++m) gd[m] = nrm > 0.f ? gy * d[m] / nrm : 0.f;
    } else {
#pragma unroll
        for (int m = 0; m < 3; ++m) gd[m] = g_y[3 * b + m];
    }
    float gv[3] = {0.f, 0.f, 0.f};
    if (g_yvec) {
#pragma unroll
        for (int m = 0; m < 3; ++m) gv[m] = g_yvec[3 * b + m];
    }
    const float sc = standardise ? scale : 1.f;
    for (int n = n0 + lane; n < n1; n += 64) {
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            g_mu[((size_t)n * 3 + m) * ldgm] = gd[m] + gv[m];
            s += gd[m] * pos[(size_t)n * 3 + m];
        }
        g_q[(size_t)n * ldgq] = sc * s;
    }
}

// Adjoint of ese_reduce_kernel w.r.t. x, one workgroup per molecule: the centroid exactly as in the forward, then
//   u[n] = g_y[b] |pos_n - c_b|^2
__global__ __launch_bounds__(64) void ese_reduce_backward_kernel(
    const float* __restrict__ g_y, const float* __restrict__ pos, const int* __restrict__ z,
    const float* __restrict__ mass, int n_mass, const int* __restrict__ mol_ptr, float* __restrict__ u) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = mol_ptr[b], n1 = mol_ptr[b + 1];
    float mp[3] = {0.f, 0.f, 0.f}, ms = 0.f;
    for (int n = n0 + lane; n < n1; n += 64) {
        const int zn = z[n];
        const float m = (zn >= 0 && zn < n_mass) ? mass[zn] : 0.f;
        ms += m;
#pragma unroll
        for (int k = 0; k < 3; ++k) mp[k] += m * pos[(size_t)n * 3 + k];
    }
    ms = wave_sum(ms);
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ms > 0.f ? wave_sum(mp[k]) / ms : 0.f;
    const float gy = g_y[b];
    for (int n = n0 + lane; n < n1; n += 64) {
        const float dx = pos[(size_t)n * 3] - c[0], dy = pos[(size_t)n * 3 + 1] - c[1], dz = pos[(size_t)n * 3 + 2] - c[2];
        const float r = sqrtf(dx * dx + dy * dy + dz * dz);
        u[n] = gy * (r * r);
    }
}

}  // namespace gn

// ====================================================================================== C ABI
extern "C" int gn_geb_context(const float* s, int lds, int n_sin, const float* vmix, int ldv, int n_vout, int N,
                              float* ctx, int ldc, void* stream) {
    if (N < 0 || n_sin <= 0 || n_vout <= 0 || ldc < n_sin + n_vout || lds < n_sin || ldv < n_vout) return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    if (!s || !vmix || !ctx) return GN_ERR_BAD_ARG;
    const size_t tot = (size_t)N * ldc;
    hipLaunchKernelGGL(gn::geb_context_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       s, lds, n_sin, vmix, ldv, n_vout, N, ctx, ldc);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_geb_gate(const float* x, int ldx, int n_sout, int n_vout, const float* vmix, int ldv, int w_off, int N,
                           int sact, float* s_out, int lds, float* v_out, int ldo, void* stream) {
    if (N < 0 || n_sout <= 0 || n_vout <= 0 || w_off < 0 || ldx < n_sout + n_vout || lds < n_sout || ldo < n_vout ||
        ldv < w_off + n_vout || sact < -1 || sact >= GN_ACT_COUNT)
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    if (!x || !vmix || !s_out || !v_out) return GN_ERR_BAD_ARG;
    const size_t tot = (size_t)N * (n_sout + 3 * n_vout);
    hipLaunchKernelGGL(gn::geb_gate_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, ldx, n_sout, n_vout, vmix, ldv, w_off, N, sact, s_out, lds, v_out, ldo);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_dipole_reduce(const float* mu, int ldm, const float* q, int ldq, const float* pos, const int* mol_ptr,
                                int n_mol, float scale, float shift, int standardise, int magnitude, float* y,
                                float* y_vec, void* stream) {
    if (n_mol < 0 || ldm <= 0 || ldq <= 0 || !y) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    if (!mu || !q || !pos || !mol_ptr) return GN_ERR_BAD_ARG;      // (y_vec stays optional)
    hipLaunchKernelGGL(gn::dipole_reduce_kernel, dim3(n_mol), dim3(64), 0, (hipStream_t)stream,
                       mu, ldm, q, ldq, pos, mol_ptr, scale, shift, standardise, magnitude, y, y_vec);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_ese_reduce(const float* x, const float* pos, const int* z, const float* mass, int n_mass,
                             const int* mol_ptr, int n_mol, float* y, void* stream) {
    if (n_mol < 0 || n_mass <= 0 || !y) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    if (!x || !pos || !z || !mass || !mol_ptr) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::ese_reduce_kernel, dim3(n_mol), dim3(64), 0, (hipStream_t)stream,
                       x, pos, z, mass, n_mass, mol_ptr, y);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

// ---- backward of the read-outs (first-order training) ----------------------------------------------------------------
extern "C" int gn_geb_gate_backward(const float* g_s_out, int ldgs, const float* g_v_out, int ldgo, const float* x,
                                    int ldx, int n_sout, int n_vout, const float* vmix, int ldv, int w_off, int N,
                                    int sact, float* g_x, int ldgx, float* g_vmix, int ldgv, void* stream) {
    if (N < 0 || n_sout <= 0 || n_vout <= 0 || w_off < 0 || ldx < n_sout + n_vout || ldgx < n_sout + n_vout ||
        ldgs < n_sout || ldgo < n_vout || ldv < w_off + n_vout || ldgv < w_off + n_vout || sact < -1 ||
        sact >= GN_ACT_COUNT)
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    if (!g_s_out || !g_v_out || !x || !vmix || !g_x || !g_vmix) return GN_ERR_BAD_ARG;
    const size_t tot = (size_t)N * (ldgx + 3 * (size_t)(ldgv - w_off));
    hipLaunchKernelGGL(gn::geb_gate_backward_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, g_s_out, ldgs, g_v_out, ldgo, x, ldx, n_sout, n_vout, vmix, ldv, w_off, N,
                       sact, g_x, ldgx, g_vmix, ldgv);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_geb_context_backward(const float* g_ctx, int ldc, int n_sin, const float* vmix, int ldv, int n_vout,
                                       int w_off, int N, float* g_s, int lds, float* g_vmix, int ldgv, void* stream) {
    if (N < 0 || n_sin <= 0 || n_vout <= 0 || w_off < n_vout || ldc < n_sin + n_vout || lds < n_sin || ldv < n_vout ||
        ldgv < w_off)
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    if (!g_ctx || !vmix || !g_s || !g_vmix) return GN_ERR_BAD_ARG;
    const size_t tot = (size_t)N * (n_sin + 3 * (size_t)w_off);
    hipLaunchKernelGGL(gn::geb_context_backward_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, g_ctx, ldc, n_sin, vmix, ldv, n_vout, w_off, N, g_s, lds, g_vmix, ldgv);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_dipole_reduce_backward(const float* g_y, const float* g_yvec, const float* mu, int ldm, const float* q,
                                         int ldq, const float* pos, const int* mol_ptr, int n_mol, float scale,
                                         float shift, int standardise, int magnitude, float* g_mu, int ldgm, float* g_q,
                                         int ldgq, void* stream) {
    if (n_mol < 0 || ldm <= 0 || ldq <= 0 || ldgm <= 0 || ldgq <= 0) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    if (!g_y || !mu || !q || !pos || !mol_ptr || !g_mu || !g_q) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::dipole_reduce_backward_kernel, dim3(n_mol), dim3(64), 0, (hipStream_t)stream,
                       g_y, g_yvec, mu, ldm, q, ldq, pos, mol_ptr, scale, shift, standardise, magnitude, g_mu, ldgm,
                       g_q, ldgq);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_ese_reduce_backward(const float* g_y, const float* pos, const int* z, const float* mass, int n_mass,
                                      const int* mol_ptr, int n_mol, float* u, void* stream) {
    if (n_mol < 0 || n_mass <= 0) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    if (!g_y || !pos || !z || !mass || !mol_ptr || !u) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::ese_reduce_backward_kernel, dim3(n_mol), dim3(64), 0, (hipStream_t)stream,
                       g_y, pos, z, mass, n_mass, mol_ptr, u);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
