// gn_neb.hip -- nudged elastic band (gotennet_amd/neb.py) around the energy + force step: the one piece of arithmetic that
// couples neighbouring images -- tangent, projection, springs -- and the end-of-step bookkeeping whose freeze granularity is
// the band.  The images of a band are consecutive molecules of the batch: molecules b n_img .. (b + 1) n_img - 1 are band b,
// and atom a of image i pairs with the atom at the same offset from mol_ptr in images i - 1 and i + 1.  FIRE itself
// (gn_fire_plan, gn_fire_move of gn_fire.hip) then runs unchanged on the band forces g, with a band for a "molecule".
//
// The tangent is the improved tangent of Henkelman and Jonsson (J. Chem. Phys. 113, 9978; ASE's "improvedtangent").  With
// t+ = R_{i+1} - R_i, t- = R_i - R_{i-1} and the kept fp32 energies E- = E_{i-1}, E = E_i, E+ = E_{i+1}, compared as they are:
//     E+ > E > E-            t = t+
//     E+ < E < E-            t = t-
//     otherwise              dmax / dmin = the larger / smaller of |E+ - E| and |E- - E|;
//                            E+ > E-:  t = dmax t+ + dmin t-;   else (ties included):  t = dmin t+ + dmax t-
// so t = c+ t+ + c- t-, and from the five sums  t+.t+, t-.t-, t+.t-, f.t+, f.t-  over the free atoms
//     |t|^2 = c+^2 t+.t+ + 2 c+ c- t+.t- + c-^2 t-.t-        f.t = c+ f.t+ + c- f.t-
//     ordinary interior image   g = f - (f.t / |t|^2) t + k (|t+| - |t-|) t / |t|
//     climbing image            g = f - 2 (f.t / |t|^2) t                 (no spring)
// |t|^2 == 0 (coincident images): g = f.  One of the three energies not finite: g = NaN (gn_fire_plan then sets status 2).
// Rows of the two end images, of fixed atoms and of atoms without a partner in both neighbours: g = 0.
//
// The scheme is gn_fire.hip's: one workgroup of 256 threads per image, per-thread partial sums over a stride of 256, the
// wave, then the four waves in order through LDS; fp64 from the fp32 inputs, products included, every stored value rounded
// once.  Plain stores, nothing read back and added to, fixed order: identical inputs, identical bits.  state is gn_md.hip's
// pair; both kernels read state[0] first and do nothing when it is set.
#include "gn_common.h"

namespace gn {

__device__ __forceinline__ bool neb_free(const unsigned char* __restrict__ fixed, int a) { return fixed == nullptr || fixed[a] == 0; }

// the larger of two; a NaN wins and stays (gn_fire.hip's fire_max)
__device__ __forceinline__ float neb_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

__device__ __forceinline__ double neb_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void neb_range(const int* __restrict__ mol_ptr, int m, int N, int& a0, int& a1) {
    a0 = min(max(mol_ptr[m], 0), N);
    a1 = min(max(mol_ptr[m + 1], a0), N);
}

__global__ __launch_bounds__(256) void neb_forces_kernel(const float* __restrict__ pos, const float* __restrict__ force,
                                                         const float* __restrict__ energy, const unsigned char* __restrict__ fixed,
                                                         const int* __restrict__ mol_ptr, int N, int n_img, double k, int climb,
                                                         float* __restrict__ g, float* __restrict__ e_band,
                                                         int* __restrict__ climb_out, const int* __restrict__ state) {
    __shared__ double sums[4][5];
    if (state[0] != 0) return;                         // (uniform over the launch)
    const int m = blockIdx.x, b = m / n_img, i = m - b * n_img, first = m - i;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int a0, a1;
    neb_range(mol_ptr, m, N, a0, a1);
    // the band's climbing image: the interior image with the largest kept energy, the first of equal ones (every thread
    // walks the same n_img - 2 numbers)
    int ci = -1;
    if (climb != 0) {
        ci = 1;
        float best = energy[first + 1];
        for (int j = 2; j < n_img - 1; ++j) {
            const float e = energy[first + j];
            if (e > best) { best = e; ci = j; }
        }
    }
    if (i == 0 && threadIdx.x == 0) {
        float mx = energy[first];
        for (int j = 1; j < n_img; ++j) mx = neb_max(mx, energy[first + j]);
        e_band[b] = mx;
        climb_out[b] = ci;
    }
    if (i == 0 || i == n_img - 1) {                    // an end image never moves  (uniform over the workgroup)
        for (int q = 3 * a0 + (int)threadIdx.x; q < 3 * a1; q += 256) g[q] = 0.0f;
        return;
    }
    int p0, p1, q0, q1;
    neb_range(mol_ptr, m - 1, N, p0, p1);
    neb_range(mol_ptr, m + 1, N, q0, q1);
    const int n = min(a1 - a0, min(p1 - p0, q1 - q0)); // atoms with a partner in both neighbours (all of them on a sound band)
    const float Em = energy[m - 1], E0 = energy[m], Ep = energy[m + 1];
    const bool finite = isfinite(Em) && isfinite(E0) && isfinite(Ep);
    double cp, cm;
    if (Ep > E0 && E0 > Em) {
        cp = 1.0;
        cm = 0.0;
    } else if (Ep < E0 && E0 < Em) {
        cp = 0.0;
        cm = 1.0;
    } else {
        const double dp = fabs((double)Ep - (double)E0), dm = fabs((double)Em - (double)E0);
        const double dmax = dp > dm ? dp : dm, dmin = dp > dm ? dm : dp;
        cp = Ep > Em ? dmax : dmin;
        cm = Ep > Em ? dmin : dmax;
    }
    double pp = 0.0, mm = 0.0, pm = 0.0, fp = 0.0, fm = 0.0;
    for (int o = (int)threadIdx.x; o < n; o += 256) {
        if (!neb_free(fixed, a0 + o)) continue;
        for (int c = 0; c < 3; ++c) {
            const double x = (double)pos[3 * (a0 + o) + c], f = (double)force[3 * (a0 + o) + c];
            const double tp = (double)pos[3 * (q0 + o) + c] - x, tm = x - (double)pos[3 * (p0 + o) + c];
            pp += tp * tp;
            mm += tm * tm;
            pm += tp * tm;
            fp += f * tp;
            fm += f * tm;
        }
    }
    pp = neb_wave_sum(pp);
    mm = neb_wave_sum(mm);
    pm = neb_wave_sum(pm);
    fp = neb_wave_sum(fp);
    fm = neb_wave_sum(fm);
    if (lane == 0) { sums[wave][0] = pp; sums[wave][1] = mm; sums[wave][2] = pm; sums[wave][3] = fp; sums[wave][4] = fm; }
    __syncthreads();
    pp = ((sums[0][0] + sums[1][0]) + sums[2][0]) + sums[3][0];
    mm = ((sums[0][1] + sums[1][1]) + sums[2][1]) + sums[3][1];
    pm = ((sums[0][2] + sums[1][2]) + sums[2][2]) + sums[3][2];
    fp = ((sums[0][3] + sums[1][3]) + sums[2][3]) + sums[3][3];
    fm = ((sums[0][4] + sums[1][4]) + sums[2][4]) + sums[3][4];
    const double tt = ((cp * cp) * pp + (2.0 * (cp * cm)) * pm) + (cm * cm) * mm;
    const double ft = cp * fp + cm * fm;
    // g = f + s t:  the projection (twice it for the climbing image) and the spring along the unit tangent
    double s = 0.0;
    if (!finite) s = __longlong_as_double(0x7ff8000000000000ll);
    else if (tt == 0.0) s = 0.0;
    else if (i == ci) s = -2.0 * (ft / tt);
    else s = (k * (sqrt(pp) - sqrt(mm))) / sqrt(tt) - ft / tt;
    const bool plain = finite && tt == 0.0;            // coincident images: g = f, whatever the tangent's rows hold
    for (int o = (int)threadIdx.x; o < a1 - a0; o += 256) {
        const int a = a0 + o;
        float* row = g + 3 * (size_t)a;
        if (o >= n || !neb_free(fixed, a)) {
            row[0] = row[1] = row[2] = 0.0f;
            continue;
        }
        for (int c = 0; c < 3; ++c) {
            const double x = (double)pos[3 * a + c], f = (double)force[3 * a + c];
            const double tp = (double)pos[3 * (q0 + o) + c] - x, tm = x - (double)pos[3 * (p0 + o) + c];
            row[c] = plain ? force[3 * a + c] : (float)(f + s * (cp * tp + cm * tm));
        }
    }
}

// end of a step, ONE workgroup: gn_fire.hip's fire_finish_kernel with the status of image m read from its band,
// status[m / n_img] -- a frozen band keeps, for every one of its images, the values it was judged on
__global__ __launch_bounds__(1024) void neb_finish_kernel(int* __restrict__ state, const int* __restrict__ status,
                                                          const int64_t* __restrict__ batch, const float* __restrict__ force,
                                                          float* __restrict__ force_keep, int n3, const float* __restrict__ energy,
                                                          float* __restrict__ energy_keep, const float* __restrict__ stress,
                                                          float* __restrict__ stress_keep, int n_mol, int n_img) {
    if (state[0] != 0) return;                         // (uniform: nobody writes state[0] here)
    const int step = state[1];
    __syncthreads();                                   // every thread holds the counter before thread 0 moves it
    const int t = threadIdx.x;
    if (t == 0) state[1] = (int)((unsigned)step + 1u);
    for (int q = t; q < n3; q += 1024) {
        const int64_t bq = batch[q / 3];
        const int m = bq < 0 ? 0 : (bq >= n_mol ? n_mol - 1 : (int)bq);
        if (status[m / n_img] == 0) force_keep[q] = force[q];
    }
    for (int m = t; m < n_mol; m += 1024)
        if (status[m / n_img] == 0) energy_keep[m] = energy[m];
    if (stress != nullptr)
        for (int q = t; q < 9 * n_mol; q += 1024)
            if (status[(q / 9) / n_img] == 0) stress_keep[q] = stress[q];
}

}  // namespace gn

static bool neb_sizes_ok(int N, int n_mol, int n_img) {
    return N >= 0 && N <= 0x7fffffff / 3 && n_mol >= 0 && n_mol <= 0x7fffffff / 9 && n_img >= 3 && n_mol % n_img == 0;
}

extern "C" int gn_neb_forces(const float* pos, const float* force, const float* energy, const unsigned char* fixed,
                             const int* mol_ptr, int N, int n_mol, int n_img, double k, int climb, float* g_out,
                             float* e_band_out, int* climb_out, const int* state, void* stream) {
    if (!neb_sizes_ok(N, n_mol, n_img) || !state || !(k >= 0.0) || !(k <= 1.7976931348623157e308) ||
        (N > 0 && (!pos || !force || !g_out)) || (n_mol > 0 && (!energy || !mol_ptr || !e_band_out || !climb_out)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::neb_forces_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, pos, force, energy, fixed, mol_ptr, N,
                       n_img, k, climb, g_out, e_band_out, climb_out, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_neb_finish(int* state, const int* status, const int64_t* batch, const float* force, float* force_keep, int N,
                             const float* energy, float* energy_keep, const float* stress, float* stress_keep, int n_mol,
                             int n_img, void* stream) {
    if (!neb_sizes_ok(N, n_mol, n_img) || !state || (N > 0 && (n_mol < 1 || !batch || !force || !force_keep)) ||
        (n_mol > 0 && (!status || !energy || !energy_keep)) || (stress && !stress_keep))
        return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::neb_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, state, status, batch, force,
                       force_keep, 3 * N, energy, energy_keep, stress, stress_keep, n_mol, n_img);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
