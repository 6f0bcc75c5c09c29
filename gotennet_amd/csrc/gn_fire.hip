// gn_fire.hip -- FIRE relaxation (Bitzek et al., PRL 97, 170201, in the variant ASE's FIRE implements) recorded around the
// energy + force step (gotennet_amd/relax.py): the per-molecule decision (plan), the move, the end-of-step bookkeeping and the
// largest force per molecule.
//
// Every molecule of a batch carries its own dt, alpha, counter of downhill steps and status (0 active, 1 converged, 2 a
// force that is not finite; 1 and 2 are sticky on the device), so each adapts and converges on its own and a finished one
// freezes while the rest go on.  state int32 [2] is gn_md.hip's: state[0] the sticky stale-list word, state[1] the number of
// completed steps.  plan, move and finish read state[0] first and do nothing when it is set.  One workgroup of 256 threads
// per molecule: per-thread partial results over a stride of 256, the wave, then the four waves in order through LDS
// (md_kinetic_kernel's scheme).  No atomics, fixed-order sums, plain stores: identical inputs, identical bits.  The sums
// P = sum f.v, sum |f|^2, sum |v|^2 and the squared length of the move are formed in fp64 from the fp32 inputs (products
// included), so the sign of P does not depend on the order of the sum; the largest |f_a|^2 is an fp32 number (x, y, z in
// order, as norm2 of gn_graph.hip) and a maximum is exact.
#include "gn_common.h"

namespace gn {

__device__ __forceinline__ bool fire_free(const unsigned char* __restrict__ fixed, int a) { return fixed == nullptr || fixed[a] == 0; }

// |f_a|^2 in fp32, 0 for a fixed atom
__device__ __forceinline__ float fire_f2(const float* __restrict__ force, const unsigned char* __restrict__ fixed, int a) {
    if (!fire_free(fixed, a)) return 0.0f;
    const float x = force[3 * a], y = force[3 * a + 1], z = force[3 * a + 2];
    float d = x * x;
    d += y * y;
    d += z * z;
    return d;
}

// the larger of two; a NaN wins and stays (fmaxf would drop it)
__device__ __forceinline__ float fire_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

__device__ __forceinline__ double fire_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float fire_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fire_max(v, __shfl_xor(v, o, 64));
    return v;
}

// max_a |f_a|^2 over the free atoms a0 <= a < a1 of one molecule, the same value in every thread of the workgroup of 256.
// `part`: four floats of LDS.  (A barrier in front: `part` may still be read from an earlier use.)
__device__ __forceinline__ float fire_block_fm2(const float* __restrict__ force, const unsigned char* __restrict__ fixed, int a0,
                                                int a1, float* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mx = 0.0f;
    for (int a = a0 + (int)threadIdx.x; a < a1; a += 256) mx = fire_max(mx, fire_f2(force, fixed, a));
    mx = fire_wave_max(mx);
    __syncthreads();
    if (lane == 0) part[wave] = mx;
    __syncthreads();
    return fire_max(fire_max(fire_max(part[0], part[1]), part[2]), part[3]);
}

__device__ __forceinline__ void fire_range(const int* __restrict__ mol_ptr, int m, int N, int& a0, int& a1) {
    a0 = min(max(mol_ptr[m], 0), N);
    a1 = min(max(mol_ptr[m + 1], a0), N);
}

__global__ __launch_bounds__(256) void fire_fmax_kernel(const float* __restrict__ force, const unsigned char* __restrict__ fixed,
                                                        const int* __restrict__ mol_ptr, int N, float* __restrict__ out) {
    __shared__ float part[4];
    int a0, a1;
    fire_range(mol_ptr, blockIdx.x, N, a0, a1);
    const float fm2 = fire_block_fm2(force, fixed, a0, a1, part);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrtf(fm2);
}

struct FireParams {
    double fmax2, dt_max, f_inc, f_dec, alpha_start, f_alpha;
    int n_min;
};

__global__ __launch_bounds__(256) void fire_plan_kernel(const float* __restrict__ force, const float* __restrict__ vel,
                                                        const unsigned char* __restrict__ fixed, const int* __restrict__ mol_ptr,
                                                        int N, int n_mol, FireParams p, float* __restrict__ dt,
                                                        float* __restrict__ alpha, int* __restrict__ n_pos, int* __restrict__ status,
                                                        int* __restrict__ converged_at, float* __restrict__ coef,
                                                        const float* __restrict__ energy_keep, float* __restrict__ log, int log_len,
                                                        const int* __restrict__ state) {
    __shared__ float part[4];
    __shared__ double sums[4][3];
    if (state[0] != 0) return;                         // (uniform over the launch)
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int a0, a1;
    fire_range(mol_ptr, m, N, a0, a1);
    double P = 0.0, ff = 0.0, vv = 0.0;
    for (int a = a0 + (int)threadIdx.x; a < a1; a += 256) {
        if (!fire_free(fixed, a)) continue;
        for (int c = 0; c < 3; ++c) {
            const double f = (double)force[3 * a + c], v = (double)vel[3 * a + c];
            P += f * v;
            ff += f * f;
            vv += v * v;
        }
    }
    P = fire_wave_sum(P);
    ff = fire_wave_sum(ff);
    vv = fire_wave_sum(vv);
    if (lane == 0) { sums[wave][0] = P; sums[wave][1] = ff; sums[wave][2] = vv; }
    const float fm2 = fire_block_fm2(force, fixed, a0, a1, part);      // (its barriers publish `sums` as well)
    if (threadIdx.x != 0) return;
    P = ((sums[0][0] + sums[1][0]) + sums[2][0]) + sums[3][0];
    ff = ((sums[0][1] + sums[1][1]) + sums[2][1]) + sums[3][1];
    vv = ((sums[0][2] + sums[1][2]) + sums[2][2]) + sums[3][2];
    const int step = state[1];
    if (log != nullptr && log_len > 0) {               // the state BEFORE the move of step `step`
        float* row = log + ((size_t)((unsigned)step % (unsigned)log_len) * (size_t)n_mol + (size_t)m) * 2;
        row[0] = energy_keep[m];
        row[1] = sqrtf(fm2);
    }
    float* cf = coef + 4 * (size_t)m;
    cf[3] = 0.0f;
    if (status[m] != 0) return;
    if (!isfinite(fm2) || (double)fm2 <= p.fmax2) {
        status[m] = isfinite(fm2) ? 1 : 2;
        converged_at[m] = step;
        return;
    }
    const double a_old = (double)alpha[m];
    double d = (double)dt[m], c_v, c_f;
    const int np = n_pos[m];
    if (np < 0) {                                      // the first step: v = 0
        n_pos[m] = 0;
        c_v = 1.0;
        c_f = 0.0;
    } else if (P > 0.0) {
        c_v = 1.0 - a_old;
        c_f = ff > 0.0 ? a_old * sqrt(vv / ff) : 0.0;
        if (np > p.n_min) {
            d = fmin(d * p.f_inc, p.dt_max);
            alpha[m] = (float)(a_old * p.f_alpha);
        }
        n_pos[m] = np + 1;
    } else {
        c_v = c_f = 0.0;
        alpha[m] = (float)p.alpha_start;
        d *= p.f_dec;
        n_pos[m] = 0;
    }
    const float dn = (float)d;
    dt[m] = dn;
    cf[0] = (float)c_v;
    cf[1] = (float)c_f;
    cf[2] = dn;
    cf[3] = 1.0f;
}

// v' = fmaf(dt, f, fmaf(c_f, f, c_v v)) per free component, then pos += scale (dt v') with scale = min(1, max_step / |dt v'|)
// over the whole molecule (the clamp acts on the displacement, not on the velocity; unit masses)
__global__ __launch_bounds__(256) void fire_move_kernel(float* __restrict__ pos, float* __restrict__ vel,
                                                        const float* __restrict__ force, const unsigned char* __restrict__ fixed,
                                                        const int* __restrict__ mol_ptr, int N, const float* __restrict__ coef,
                                                        double max_step, const int* __restrict__ state) {
    __shared__ double part[4];
    if (state[0] != 0) return;
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* cf = coef + 4 * (size_t)m;
    if (cf[3] == 0.0f) return;                         // (uniform over the workgroup)
    const float c_v = cf[0], c_f = cf[1], dt = cf[2];
    int a0, a1;
    fire_range(mol_ptr, m, N, a0, a1);
    double n2 = 0.0;
    for (int k = 3 * a0 + (int)threadIdx.x; k < 3 * a1; k += 256) {
        if (!fire_free(fixed, k / 3)) continue;
        const float f = force[k];
        const float v = fmaf(dt, f, fmaf(c_f, f, c_v * vel[k]));
        vel[k] = v;
        const double dr = (double)dt * (double)v;
        n2 += dr * dr;
    }
    n2 = fire_wave_sum(n2);
    if (lane == 0) part[wave] = n2;
    __syncthreads();
    n2 = ((part[0] + part[1]) + part[2]) + part[3];
    const double nrm = sqrt(n2);
    const float scale = (float)(nrm > max_step ? max_step / nrm : 1.0);
    for (int k = 3 * a0 + (int)threadIdx.x; k < 3 * a1; k += 256) {       // (each thread re-reads the velocities it stored)
        if (!fire_free(fixed, k / 3)) continue;
        const float dr = dt * vel[k];
        pos[k] += scale * dr;
    }
}

// end of a step, ONE workgroup: the counter moves on, and the step's forces / energies / stress become the kept ones for the
// molecules whose status is 0 -- a frozen molecule keeps the values it was judged on
__global__ __launch_bounds__(1024) void fire_finish_kernel(int* __restrict__ state, const int* __restrict__ status,
                                                           const int64_t* __restrict__ batch, const float* __restrict__ force,
                                                           float* __restrict__ force_keep, int n3, const float* __restrict__ energy,
                                                           float* __restrict__ energy_keep, const float* __restrict__ stress,
                                                           float* __restrict__ stress_keep, int n_mol) {
    if (state[0] != 0) return;                         // (uniform: nobody writes state[0] here)
    const int step = state[1];
    __syncthreads();                                   // every thread holds the counter before thread 0 moves it
    const int t = threadIdx.x;
    if (t == 0) state[1] = (int)((unsigned)step + 1u);
    for (int k = t; k < n3; k += 1024) {
        const int64_t b = batch[k / 3];
        const int m = b < 0 ? 0 : (b >= n_mol ? n_mol - 1 : (int)b);
        if (status[m] == 0) force_keep[k] = force[k];
    }
    for (int m = t; m < n_mol; m += 1024)
        if (status[m] == 0) energy_keep[m] = energy[m];
    if (stress != nullptr)
        for (int k = t; k < 9 * n_mol; k += 1024)
            if (status[k / 9] == 0) stress_keep[k] = stress[k];
}

}  // namespace gn

static bool fire_sizes_ok(int N, int n_mol) { return N >= 0 && N <= 0x7fffffff / 3 && n_mol >= 0 && n_mol <= 0x7fffffff / 9; }

extern "C" int gn_fire_fmax(const float* force, const unsigned char* fixed, const int* mol_ptr, int N, int n_mol, float* out,
                            void* stream) {
    if (!fire_sizes_ok(N, n_mol) || (N > 0 && !force) || (n_mol > 0 && (!mol_ptr || !out))) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::fire_fmax_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, force, fixed, mol_ptr, N, out);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_fire_plan(const float* force, const float* vel, const unsigned char* fixed, const int* mol_ptr, int N,
                            int n_mol, double fmax, double dt_max, int n_min, double f_inc, double f_dec, double alpha_start,
                            double f_alpha, float* dt, float* alpha, int* n_pos, int* status, int* converged_at, float* coef,
                            const float* energy_keep, float* log, int log_len, const int* state, void* stream) {
    if (!fire_sizes_ok(N, n_mol) || !state || log_len < 0 || !(fmax >= 0.0) || !(dt_max > 0.0) || n_min < 0 || !(f_inc >= 1.0) ||
        !(f_dec > 0.0 && f_dec < 1.0) || !(alpha_start > 0.0 && alpha_start <= 1.0) || !(f_alpha > 0.0 && f_alpha < 1.0) ||
        (N > 0 && (!force || !vel)) ||
        (n_mol > 0 && (!mol_ptr || !dt || !alpha || !n_pos || !status || !converged_at || !coef || !energy_keep)) ||
        (log_len > 0 && n_mol > 0 && !log))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    const gn::FireParams p{fmax * fmax, dt_max, f_inc, f_dec, alpha_start, f_alpha, n_min};
    hipLaunchKernelGGL(gn::fire_plan_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, force, vel, fixed, mol_ptr, N, n_mol,
                       p, dt, alpha, n_pos, status, converged_at, coef, energy_keep, log, log_len, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_fire_move(float* pos, float* vel, const float* force, const unsigned char* fixed, const int* mol_ptr, int N,
                            int n_mol, const float* coef, double max_step, const int* state, void* stream) {
    if (!fire_sizes_ok(N, n_mol) || !state || !(max_step > 0.0) || (N > 0 && (!pos || !vel || !force)) ||
        (n_mol > 0 && (!mol_ptr || !coef)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::fire_move_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, pos, vel, force, fixed, mol_ptr, N,
                       coef, max_step, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_fire_finish(int* state, const int* status, const int64_t* batch, const float* force, float* force_keep, int N,
                              const float* energy, float* energy_keep, const float* stress, float* stress_keep, int n_mol,
                              void* stream) {
    if (!fire_sizes_ok(N, n_mol) || !state || (N > 0 && (n_mol < 1 || !batch || !force || !force_keep)) ||
        (n_mol > 0 && (!status || !energy || !energy_keep)) || (stress && !stress_keep))
        return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::fire_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, state, status, batch, force,
                       force_keep, 3 * N, energy, energy_keep, stress, stress_keep, n_mol);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
