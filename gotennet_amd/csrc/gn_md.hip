// gn_md.hip -- the integrator of a molecular-dynamics step recorded around the energy + force step (gotennet_amd/md.py):
// velocity-Verlet kick and drift, the Langevin O step with its noise drawn on the device, the kinetic energy, the
// end-of-step bookkeeping and the barostat (gn_npt_*: the volume move, the rescaling, the internal pressure, the cell guard;
// gn_cell_image_ranges: the image ranges of a moved cell, on the guard's arithmetic).
//
// state int32 [2]: state[0] is the sticky "the stored neighbour list is stale" word of gn_radius_verify*, state[1] the number
// of completed steps.  Every kernel here reads state[0] first and does nothing when it is set: a replay on a stale list moves
// no atom, no velocity, no counter and no log row, so the host can repair the list and finish that step whenever it looks.
// Element-wise kernels are one thread per element, sums run in a fixed order, no atomics: identical inputs, identical bits.
#include "gn_common.h"
#include "gn_dropout.h"

namespace gn {

__device__ __forceinline__ bool md_frozen(const int* __restrict__ state) { return state != nullptr && state[0] != 0; }

// mass of atom a, 0 for an atomic number outside the table (the host refuses those; such an atom is left alone)
__device__ __forceinline__ float md_mass(const int* __restrict__ z, const float* __restrict__ mass, int n_mass, int a) {
    const int zz = z[a];
    return zz >= 0 && zz < n_mass ? mass[zz] : 0.0f;
}

// v += s f / m[z]   (s = dt / 2 * force_scale)
__global__ void md_kick_kernel(float* __restrict__ vel, const float* __restrict__ force, const int* __restrict__ z,
                               const float* __restrict__ mass, int n_mass, int n3, float s, const int* __restrict__ state) {
    if (md_frozen(state)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n3) return;
    const float m = md_mass(z, mass, n_mass, k / 3);
    if (m > 0.0f) vel[k] += s * force[k] / m;
}

// pos += dt v
__global__ void md_drift_kernel(float* __restrict__ pos, const float* __restrict__ vel, int n3, float dt,
                                const int* __restrict__ state) {
    if (md_frozen(state)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n3) pos[k] += dt * vel[k];
}

// ---- the thermostat's noise: a pure function of (key, step, draw, atom, component pair), stated in include/gotennet_hip.h
// 24 bits of a Philox word as a uniform in (0, 1] (exact in fp32): the logarithm below is finite
__device__ __forceinline__ float unit_interval(unsigned w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-08f; }
// two standard normals (Box-Muller) of one Philox evaluation: pair 0 -> components x, y; pair 1 -> z (and one unused)
__device__ __forceinline__ void md_normal_pair(const long long* __restrict__ key, unsigned atom, unsigned pair, unsigned draw,
                                               unsigned step, float& a, float& b) {
    const unsigned long long k = (unsigned long long)key[0], s = (unsigned long long)key[1];
    const uint4 w = philox4x32_10(atom, pair + 2u * draw, step, (unsigned)s, (unsigned)k, (unsigned)(k >> 32));
    const float r = sqrtf(-2.0f * logf(unit_interval(w.x)));
    const float t = 6.28318530717958648f * unit_interval(w.y);
    a = r * cosf(t);
    b = r * sinf(t);
}

// v = c1 v + c2 sqrt(1 / m[z]) xi, one thread per (atom, component pair), step = state[1]
__global__ void md_langevin_kernel(float* __restrict__ vel, const int* __restrict__ z, const float* __restrict__ mass,
                                   int n_mass, int N, float c1, float c2, const long long* __restrict__ key, unsigned draw,
                                   const int* __restrict__ state) {
    if (state[0] != 0) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2 * N) return;
    const int a = k >> 1, pair = k & 1;
    const float m = md_mass(z, mass, n_mass, a);
    if (!(m > 0.0f)) return;
    float xa, xb;
    md_normal_pair(key, (unsigned)a, (unsigned)pair, draw, (unsigned)state[1], xa, xb);
    const float g = c2 * sqrtf(1.0f / m);
    float* v = vel + 3 * a + 2 * pair;
    v[0] = c1 * v[0] + g * xa;
    if (pair == 0) v[1] = c1 * v[1] + g * xb;
}

// the same noise on its own: one thread per atom
__global__ __launch_bounds__(64) void md_noise_kernel(const long long* __restrict__ key, unsigned step, unsigned draw, int N,
                                                      float* __restrict__ out) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= N) return;
    float x, y, zz, unused;
    md_normal_pair(key, (unsigned)a, 0u, draw, step, x, y);
    md_normal_pair(key, (unsigned)a, 1u, draw, step, zz, unused);
    out[3 * a] = x; out[3 * a + 1] = y; out[3 * a + 2] = zz;
}

// ke[m] = (1/2) sum_{a in molecule m} mass[z_a] |v_a|^2 / force_scale.  One workgroup per molecule: per-thread sums over a
// stride of 256 atoms, wave_sum, then the four waves in order through LDS (gn_virial's scheme).
__global__ __launch_bounds__(256) void md_kinetic_kernel(const float* __restrict__ vel, const int* __restrict__ z,
                                                         const float* __restrict__ mass, int n_mass,
                                                         const int* __restrict__ mol_ptr, int N, float force_scale,
                                                         float* __restrict__ ke, const int* __restrict__ state) {
    __shared__ float part[4];
    if (md_frozen(state)) return;                      // (uniform over the launch)
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a0 = max(mol_ptr[m], 0), a1 = min(mol_ptr[m + 1], N);
    float s = 0.0f;
    for (int a = a0 + (int)threadIdx.x; a < a1; a += 256) {
        const float x = vel[3 * a], y = vel[3 * a + 1], w = vel[3 * a + 2];
        float v2 = x * x;
        v2 += y * y;
        v2 += w * w;
        s += md_mass(z, mass, n_mass, a) * v2;
    }
    const float t = wave_sum(s);
    if (lane == 0) part[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) ke[m] = 0.5f * (((part[0] + part[1]) + part[2]) + part[3]) / force_scale;
}

// end of a step, ONE workgroup: the step counter moves on, the step's forces / energies / stress become the kept ones (what the
// next kick reads; what the host reads, whatever a later stale replay leaves in the step's own buffers), and row
// (old counter mod log_len) of the log receives (potential, kinetic) per molecule.
__global__ __launch_bounds__(1024) void md_finish_kernel(int* __restrict__ state, const float* __restrict__ force,
                                                         float* __restrict__ force_keep, int n3,
                                                         const float* __restrict__ energy, const float* __restrict__ ke,
                                                         float* __restrict__ energy_keep, const float* __restrict__ stress,
                                                         float* __restrict__ stress_keep, float* __restrict__ log,
                                                         int log_len, int n_mol) {
    if (state[0] != 0) return;                         // (uniform: nobody writes state[0] here)
    const unsigned step = (unsigned)state[1];
    __syncthreads();                                   // every thread holds the counter before thread 0 moves it
    const int t = threadIdx.x;
    if (t == 0) state[1] = (int)(step + 1u);
    for (int k = t; k < n3; k += 1024) force_keep[k] = force[k];
    float* row = log_len > 0 ? log + (size_t)(step % (unsigned)log_len) * (size_t)n_mol * 2 : nullptr;
    for (int m = t; m < n_mol; m += 1024) {
        energy_keep[m] = energy[m];
        if (row != nullptr) {
            row[2 * m] = energy[m];
            row[2 * m + 1] = ke[m];
        }
    }
    if (stress != nullptr)
        for (int k = t; k < 9 * n_mol; k += 1024) stress_keep[k] = stress[k];
}

// ---- the barostat: isotropic stochastic cell rescaling in eps = ln V (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020),
// stated in include/gotennet_hip.h.  reason int32 [n_mol] holds WHY a box stopped the run (1: the cell outgrew the search
// parameters, 2: a volume move beyond max_step); state[0] is the one sticky word all kernels are predicated on.
// P_int = 2 K / (3 V) - tr(sigma) / 3 in fp64 from the fp32 inputs, rounded once
__device__ __forceinline__ float npt_pressure(float ke, const float* __restrict__ sg, float vol) {
    const double tr = ((double)sg[0] + (double)sg[4]) + (double)sg[8];
    return (float)(2.0 * (double)ke / (3.0 * (double)vol) - tr / 3.0);
}

// One thread per box: the kept pressure of the step that is ending and row (counter mod log_len) of the (V, P) ring.
// Runs BEFORE md_finish_kernel moves the counter.
__global__ void npt_pressure_kernel(const float* __restrict__ ke, const float* __restrict__ stress,
                                    const float* __restrict__ volume, int n_mol, float* __restrict__ pressure,
                                    float* __restrict__ log, int log_len, const int* __restrict__ state) {
    if (md_frozen(state)) return;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_mol) return;
    const float p = npt_pressure(ke[m], stress + 9 * (size_t)m, volume[m]);
    pressure[m] = p;
    if (log != nullptr && log_len > 0 && state != nullptr) {
        float* row = log + ((size_t)((unsigned)state[1] % (unsigned)log_len) * (size_t)n_mol + (size_t)m) * 2;
        row[0] = volume[m];
        row[1] = p;
    }
}

// d eps = -(beta / tau) (P0 - P) dt + sqrt(2 kT beta dt / (V tau)) xi.  (The volume equation of the paper carries a drift
// kT beta / tau per unit time as well; written in eps = ln V it cancels against the Ito term -(1/2) (2 kT beta / (V tau)) V / V,
// so the equation in eps has none.)  xi: the first normal of md_normal_pair(key, box, pair 0, draw 2, step); the key is not
// read when kT == 0.
__device__ __forceinline__ double npt_delta_eps(int m, const float* __restrict__ volume, const float* __restrict__ pressure,
                                                double p0, double beta, double tau, double dt, double kT,
                                                const long long* __restrict__ key, unsigned step) {
    double de = -(beta / tau) * (p0 - (double)pressure[m]) * dt;
    if (kT > 0.0) {
        float xa, xb;
        md_normal_pair(key, (unsigned)m, 0u, 2u, step, xa, xb);
        de += sqrt(2.0 * kT * beta * dt / ((double)volume[m] * tau)) * (double)xa;
    }
    return de;
}

// ONE workgroup, a thread per box (strided beyond 1024 boxes).  First every box's move is held against max_step: a move that
// is not finite or is larger stores reason 2 for its box and sets the sticky word, and then NO box is moved -- the cell array,
// s and inv_s stay as they are.  Otherwise s = exp(d eps / 3) and 1 / s are rounded once to fp32 and the nine cell entries
// are multiplied by s in fp32.
__global__ __launch_bounds__(1024) void npt_barostat_kernel(float* __restrict__ cell, const float* __restrict__ volume,
                                                            const float* __restrict__ pressure, int n_mol, double p0,
                                                            double beta, double tau, double dt, double kT, double max_step,
                                                            const long long* __restrict__ key, float* __restrict__ s_out,
                                                            float* __restrict__ inv_s_out, int* __restrict__ state,
                                                            int* __restrict__ reason) {
    if (state[0] != 0) return;                         // (uniform: the word is written behind the barrier below only)
    const unsigned step = (unsigned)state[1];
    int bad = 0;
    for (int m = threadIdx.x; m < n_mol; m += 1024) {
        const double de = npt_delta_eps(m, volume, pressure, p0, beta, tau, dt, kT, key, step);
        if (!(fabs(de) <= max_step)) {                 // (a NaN fails the comparison)
            reason[m] = 2;
            bad = 1;
        }
    }
    if (__syncthreads_or(bad)) {
        if (bad) state[0] = 1;
        return;
    }
    for (int m = threadIdx.x; m < n_mol; m += 1024) {
        const double sd = exp(npt_delta_eps(m, volume, pressure, p0, beta, tau, dt, kT, key, step) / 3.0);
        const float s = (float)sd;
        s_out[m] = s;
        inv_s_out[m] = (float)(1.0 / sd);
        float* c = cell + 9 * (size_t)m;
        for (int k = 0; k < 9; ++k) c[k] *= s;
    }
}

// pos *= s[box], vel *= 1 / s[box]: one thread per component (positions are scaled about the origin; a stored shift stays
// valid, pos[j] - pos[i] + shift @ cell scales as a whole)
__global__ void npt_rescale_kernel(float* __restrict__ pos, float* __restrict__ vel, const int64_t* __restrict__ batch,
                                   const float* __restrict__ s, const float* __restrict__ inv_s, int n3, int n_mol,
                                   const int* __restrict__ state) {
    if (md_frozen(state)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n3) return;
    const int64_t b = batch[k / 3];
    const int m = b < 0 ? 0 : (b >= n_mol ? n_mol - 1 : (int)b);        // (clamped as the searches clamp it)
    pos[k] *= s[m];
    vel[k] *= inv_s[m];
}

// The perpendicular widths of one cell in fp64 from its fp32 entries, the formulas of the host's check (graph.cell_widths):
// w[k] = V / |a_i x a_j|, V = |a . (b x c)| returned.  What the guard and the range kernel below both decide from.  A volume
// that is zero or not finite leaves w unset.
__device__ __forceinline__ double npt_cell_widths(const float* __restrict__ c, double w[3]) {
    const double a[3] = {c[0], c[1], c[2]}, b[3] = {c[3], c[4], c[5]}, d[3] = {c[6], c[7], c[8]};
    const double f[3][3] = {{b[1] * d[2] - b[2] * d[1], b[2] * d[0] - b[0] * d[2], b[0] * d[1] - b[1] * d[0]},       // b x c
                            {d[1] * a[2] - d[2] * a[1], d[2] * a[0] - d[0] * a[2], d[0] * a[1] - d[1] * a[0]},       // c x a
                            {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}};      // a x b
    const double vol = fabs((a[0] * f[0][0] + a[1] * f[0][1]) + a[2] * f[0][2]);
    if (!(isfinite(vol) && vol != 0.0)) return vol;
    for (int k = 0; k < 3; ++k) w[k] = vol / sqrt((f[k][0] * f[k][0] + f[k][1] * f[k][1]) + f[k][2] * f[k][2]);
    return vol;
}

// The image range a width asks for, floor(cutoff / w + 1/2 + 2^-6) (graph.image_ranges), as a double: the caller compares
__device__ __forceinline__ double npt_image_range(double cutoff, double w) { return floor(cutoff / w + 0.5 + 0.015625); }

// Does the moved cell still satisfy what the search parameters of this run assume?  One thread per box, fp64:
// minimum image (img_range == NULL): w_k >= 2 cutoff; else floor(cutoff / w_k + 1/2 + 2^-6) <= R_k.  A volume that is zero
// or not finite fails either way.
__global__ void npt_cell_guard_kernel(const float* __restrict__ cell, int n_mol, double cutoff,
                                      const int* __restrict__ img_range, int* __restrict__ state, int* __restrict__ reason) {
    if (state[0] != 0) return;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_mol) return;
    double w[3];
    const double vol = npt_cell_widths(cell + 9 * (size_t)m, w);
    bool ok = isfinite(vol) && vol != 0.0;
    for (int k = 0; k < 3 && ok; ++k) {
        if (img_range == nullptr) ok = w[k] >= 2.0 * cutoff;
        else ok = isfinite(w[k]) && w[k] > 0.0 && npt_image_range(cutoff, w[k]) <= (double)img_range[3 * m + k];
    }
    if (!ok) {
        reason[m] = 1;
        state[0] = 1;
    }
}

// The image ranges of the moved cell, for a search that is rebuilt inside the step: ONE workgroup, a thread per box (strided
// beyond 1024 boxes), the guard's arithmetic.  Every thread reads the sticky word before the barrier and nobody writes it
// before, so a launch that starts frozen writes nothing and a launch that starts clear treats every box alike, whatever
// another box of the same launch decides.  img_range[m, k] = floor(cutoff / w_k + 1/2 + 2^-6); a box whose volume is zero or
// not finite, or that asks for more than max_range images on some axis, keeps its row and stores reason 1 and the word.
__global__ __launch_bounds__(1024) void cell_image_ranges_kernel(const float* __restrict__ cell, int n_mol, double cutoff,
                                                                int max_range, int* __restrict__ img_range,
                                                                int* __restrict__ state, int* __restrict__ reason) {
    const int frozen = state[0];
    __syncthreads();
    if (frozen != 0) return;                           // (uniform: one word, read by all before anybody stores it)
    for (int m = threadIdx.x; m < n_mol; m += 1024) {
        double w[3];
        const double vol = npt_cell_widths(cell + 9 * (size_t)m, w);
        bool ok = isfinite(vol) && vol != 0.0;
        int r[3] = {0, 0, 0};
        for (int k = 0; k < 3 && ok; ++k) {
            const double rk = isfinite(w[k]) && w[k] > 0.0 ? npt_image_range(cutoff, w[k]) : -1.0;
            ok = rk >= 0.0 && rk <= (double)max_range;
            r[k] = ok ? (int)rk : 0;
        }
        if (ok) {
            for (int k = 0; k < 3; ++k) img_range[3 * (size_t)m + k] = r[k];
        } else {
            reason[m] = 1;
            state[0] = 1;
        }
    }
}

}  // namespace gn

static bool md_table_ok(const int* z, const float* mass, int n_mass, int N) { return N == 0 || (z && mass && n_mass > 0); }

extern "C" int gn_md_kick(float* vel, const float* force, const int* z, const float* mass, int n_mass, int N, float s,
                          const int* state, void* stream) {
    if (N < 0 || N > 0x7fffffff / 3 || !md_table_ok(z, mass, n_mass, N) || (N > 0 && (!vel || !force))) return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::md_kick_kernel, dim3((3 * N + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       vel, force, z, mass, n_mass, 3 * N, s, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_md_drift(float* pos, const float* vel, int N, float dt, const int* state, void* stream) {
    if (N < 0 || N > 0x7fffffff / 3 || (N > 0 && (!pos || !vel))) return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::md_drift_kernel, dim3((3 * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos, vel, 3 * N, dt,
                       state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_md_langevin(float* vel, const int* z, const float* mass, int n_mass, int N, float c1, float c2,
                              const long long* key, int draw, const int* state, void* stream) {
    if (N < 0 || N > 0x7fffffff / 3 || draw < 0 || !key || !state || !md_table_ok(z, mass, n_mass, N) || (N > 0 && !vel))
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::md_langevin_kernel, dim3((2 * N + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       vel, z, mass, n_mass, N, c1, c2, key, (unsigned)draw, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_md_noise(const long long* key, long step, int draw, int N, float* out, void* stream) {
    if (N < 0 || N > 0x7fffffff / 3 || draw < 0 || step < 0 || step > 0xffffffffL || !key || (N > 0 && !out))
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::md_noise_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, key, (unsigned)step,
                       (unsigned)draw, N, out);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_md_kinetic(const float* vel, const int* z, const float* mass, int n_mass, const int* mol_ptr, int N,
                             int n_mol, float force_scale, float* ke, const int* state, void* stream) {
    if (N < 0 || n_mol < 0 || !(force_scale > 0.0f) || !md_table_ok(z, mass, n_mass, N) || (N > 0 && !vel) ||
        (n_mol > 0 && (!mol_ptr || !ke)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::md_kinetic_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, vel, z, mass, n_mass, mol_ptr, N,
                       force_scale, ke, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_md_finish(int* state, const float* force, float* force_keep, int N, const float* energy, const float* ke,
                            float* energy_keep, const float* stress, float* stress_keep, float* log, int log_len, int n_mol,
                            void* stream) {
    if (!state || N < 0 || N > 0x7fffffff / 3 || n_mol < 0 || n_mol > 0x7fffffff / 9 || log_len < 0 ||
        (N > 0 && (!force || !force_keep)) || (n_mol > 0 && (!energy || !ke || !energy_keep)) ||
        (log_len > 0 && n_mol > 0 && !log) || (stress && !stress_keep))
        return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::md_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, state, force, force_keep, 3 * N,
                       energy, ke, energy_keep, stress, stress_keep, log, log_len, n_mol);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

static bool npt_count_ok(int n_mol) { return n_mol >= 0 && n_mol <= 0x7fffffff / 9; }

extern "C" int gn_npt_pressure(const float* ke, const float* stress, const float* volume, int n_mol, float* pressure,
                               float* log, int log_len, const int* state, void* stream) {
    if (!npt_count_ok(n_mol) || log_len < 0 || (n_mol > 0 && (!ke || !stress || !volume || !pressure))) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::npt_pressure_kernel, dim3((n_mol + 63) / 64), dim3(64), 0, (hipStream_t)stream, ke, stress, volume,
                       n_mol, pressure, log, log_len, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_npt_barostat(float* cell, const float* volume, const float* pressure, int n_mol, double p0, double beta,
                               double tau, double dt, double kT, double max_step, const long long* key, float* s,
                               float* inv_s, int* state, int* reason, void* stream) {
    if (!npt_count_ok(n_mol) || !state || !(beta > 0.0) || !(tau > 0.0) || !(dt > 0.0) || !(kT >= 0.0) || !(max_step > 0.0) ||
        (kT > 0.0 && !key) || (n_mol > 0 && (!cell || !volume || !pressure || !s || !inv_s || !reason)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::npt_barostat_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, cell, volume, pressure, n_mol, p0,
                       beta, tau, dt, kT, max_step, key, s, inv_s, state, reason);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_npt_rescale(float* pos, float* vel, const int64_t* batch, const float* s, const float* inv_s, int N,
                              int n_mol, const int* state, void* stream) {
    if (N < 0 || N > 0x7fffffff / 3 || n_mol < 0 || (N > 0 && (n_mol < 1 || !pos || !vel || !batch || !s || !inv_s)))
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::npt_rescale_kernel, dim3((3 * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos, vel, batch, s,
                       inv_s, 3 * N, n_mol, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_npt_cell_guard(const float* cell, int n_mol, double cutoff, const int* img_range, int* state, int* reason,
                                 void* stream) {
    if (!npt_count_ok(n_mol) || !state || !(cutoff > 0.0) || (n_mol > 0 && (!cell || !reason))) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::npt_cell_guard_kernel, dim3((n_mol + 63) / 64), dim3(64), 0, (hipStream_t)stream, cell, n_mol, cutoff,
                       img_range, state, reason);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_cell_image_ranges(const float* cell, int n_mol, double cutoff, int max_range, int* img_range, int* state,
                                   int* reason, void* stream) {
    if (!npt_count_ok(n_mol) || !state || !(cutoff > 0.0) || max_range < 0 || max_range > GN_PBC_MAX_IMAGE_RANGE ||
        (n_mol > 0 && (!cell || !img_range || !reason)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::cell_image_ranges_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, cell, n_mol, cutoff, max_range,
                       img_range, state, reason);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
