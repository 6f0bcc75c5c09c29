// gn_cellrelax.hip -- variable-cell relaxation (gotennet_amd/relax.py, CellRelax): FIRE over the atoms AND the cell of every
// periodic box, in the formulation of ASE's UnitCellFilter written for row vectors.  Per box m: the reference cell C0 (the
// start), the deformation gradient F (the identity at the start), the reference coordinates x~ (the start positions);
//     pos = x~ F,   cell = C0 F,   degrees of freedom: the rows of x~ and the three "cell rows" U = w F  (w = cell_factor).
// The extended system of a box -- its atom rows, then its three cell rows -- is laid out so that gn_fire_plan and gn_fire_move
// run on it as on a molecule of n_m + 3 atoms: box m owns rows [mol_ptr[m] + 3 m, mol_ptr[m + 1] + 3 (m + 1)) of x_ext / g_ext.
//
// Generalised forces -dH/d(dof), H = E + pressure V, from the kept forces f and the kept stress sigma = (1/V) sum r (x) dE/dr:
//     atom rows   g_a = f_a F^T                       (dE/dx~_ai = sum_j dE/dpos_aj F_ij)
//     cell rows   G   = -(V / w) F^-T S,  S = (sigma + sigma^T) / 2 + pressure I
//                 (a change dF strains every vector by r -> r (I + F^-1 dF):  dE = V sigma : F^-1 dF,  dV = V tr(F^-1 dF))
// hydrostatic: S <- (tr S / 3) I;  then the components whose cell_mask entry is 0 are exactly 0.
//
// One workgroup of 256 threads per box; the 3 x 3 algebra is redone by every thread from the same inputs (it is a few dozen
// flops), the atoms go over a stride of 256.  Everything is fp64 from the fp32 inputs and every stored value is rounded once.
// Plain stores, no read-modify-write, fixed order: identical inputs, identical bits.  state is gn_md.hip's pair; both kernels
// read state[0] first and do nothing when it is set.
#include "gn_common.h"

namespace gn {

__device__ __forceinline__ void cellrelax_range(const int* __restrict__ mol_ptr, int m, int N, int& a0, int& a1) {
    a0 = min(max(mol_ptr[m], 0), N);
    a1 = min(max(mol_ptr[m + 1], a0), N);
}

// F = U / w from the three cell rows of box m, which follow its atom rows: extended rows a1 + 3 m .. a1 + 3 m + 2
__device__ __forceinline__ void cellrelax_deformation(const float* __restrict__ x_ext, int a1, int m, double w, double* F) {
    const float* u = x_ext + 3 * ((size_t)a1 + 3 * (size_t)m);
    for (int k = 0; k < 9; ++k) F[k] = (double)u[k] / w;
}

__device__ __forceinline__ double cellrelax_det(const double* a) {
    return a[0] * (a[4] * a[8] - a[5] * a[7]) + a[1] * (a[5] * a[6] - a[3] * a[8]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

__global__ __launch_bounds__(256) void cellrelax_forces_kernel(const float* __restrict__ force, const float* __restrict__ stress,
                                                               const float* __restrict__ cell, const float* __restrict__ x_ext,
                                                               const float* __restrict__ weight, double pressure, int hydrostatic,
                                                               const unsigned char* __restrict__ cell_mask,
                                                               const unsigned char* __restrict__ fixed,
                                                               const int* __restrict__ mol_ptr, int N, float* __restrict__ g_ext,
                                                               const int* __restrict__ state) {
    if (state[0] != 0) return;                         // (uniform over the launch)
    const int m = blockIdx.x;
    int a0, a1;
    cellrelax_range(mol_ptr, m, N, a0, a1);
    const double w = (double)weight[m];
    double F[9];
    cellrelax_deformation(x_ext, a1, m, w, F);
    const size_t shift = 3 * (size_t)m;                // atom a of this box is extended row a + 3 m
    if (threadIdx.x < 9) {
        const int i = threadIdx.x / 3, k = threadIdx.x % 3;
        double c[9], s[9], S[9];
        for (int q = 0; q < 9; ++q) {
            c[q] = (double)cell[9 * (size_t)m + q];
            s[q] = (double)stress[9 * (size_t)m + q];
        }
        const double V = fabs(cellrelax_det(c));
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) S[3 * r + q] = 0.5 * (s[3 * r + q] + s[3 * q + r]) + (r == q ? pressure : 0.0);
        if (hydrostatic) {
            const double t = ((S[0] + S[4]) + S[8]) / 3.0;
            for (int q = 0; q < 9; ++q) S[q] = (q % 4 == 0) ? t : 0.0;
        }
        // column i of F^-1 = row i of F^-T: cofactors of row i of F over det F
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        const double det = cellrelax_det(F);
        double t[3];
        for (int l = 0; l < 3; ++l) {
            const int l1 = (l + 1) % 3, l2 = (l + 2) % 3;
            t[l] = (F[3 * i1 + l1] * F[3 * i2 + l2] - F[3 * i1 + l2] * F[3 * i2 + l1]) / det;     // (F^-T)_il = cof(F)_il / det
        }
        const double G = -(V / w) * ((t[0] * S[k] + t[1] * S[3 + k]) + t[2] * S[6 + k]);
        const bool keep = cell_mask == nullptr || cell_mask[threadIdx.x] != 0;
        g_ext[3 * ((size_t)a1 + shift) + threadIdx.x] = keep ? (float)G : 0.0f;
    }
    for (int a = a0 + (int)threadIdx.x; a < a1; a += 256) {
        const bool free_atom = fixed == nullptr || fixed[a] == 0;
        const double fx = (double)force[3 * a], fy = (double)force[3 * a + 1], fz = (double)force[3 * a + 2];
        float* g = g_ext + 3 * ((size_t)a + shift);
        for (int i = 0; i < 3; ++i) g[i] = free_atom ? (float)((F[3 * i] * fx + F[3 * i + 1] * fy) + F[3 * i + 2] * fz) : 0.0f;
    }
}

// the boxes FIRE has just moved (coef[m][3] == 1): pos = x~ F for every atom, fixed ones included (they follow the cell
// affinely), and cell = C0 F, with F read from the moved cell rows
__global__ __launch_bounds__(256) void cellrelax_apply_kernel(const float* __restrict__ x_ext, const float* __restrict__ cell0,
                                                              const float* __restrict__ weight, const float* __restrict__ coef,
                                                              const int* __restrict__ mol_ptr, int N, float* __restrict__ pos,
                                                              float* __restrict__ cell, const int* __restrict__ state) {
    if (state[0] != 0) return;
    const int m = blockIdx.x;
    if (coef[4 * (size_t)m + 3] != 1.0f) return;       // (uniform over the workgroup)
    int a0, a1;
    cellrelax_range(mol_ptr, m, N, a0, a1);
    double F[9];
    cellrelax_deformation(x_ext, a1, m, (double)weight[m], F);
    if (threadIdx.x < 9) {
        const int i = threadIdx.x / 3, k = threadIdx.x % 3;
        const float* c = cell0 + 9 * (size_t)m + 3 * i;
        cell[9 * (size_t)m + threadIdx.x] = (float)(((double)c[0] * F[k] + (double)c[1] * F[3 + k]) + (double)c[2] * F[6 + k]);
    }
    const size_t shift = 3 * (size_t)m;
    for (int a = a0 + (int)threadIdx.x; a < a1; a += 256) {
        const float* x = x_ext + 3 * ((size_t)a + shift);
        const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
        for (int k = 0; k < 3; ++k) pos[3 * a + k] = (float)((x0 * F[k] + x1 * F[3 + k]) + x2 * F[6 + k]);
    }
}

}  // namespace gn

// N real atoms, n_mol boxes: the extended arrays have N + 3 n_mol rows of three
static bool cellrelax_sizes_ok(int N, int n_mol) {
    return N >= 0 && n_mol >= 0 && n_mol <= 0x7fffffff / 9 && (long long)N + 3ll * n_mol <= 0x7fffffff / 3;
}

extern "C" int gn_cellrelax_forces(const float* force, const float* stress, const float* cell, const float* x_ext,
                                   const float* weight, double pressure, int hydrostatic, const unsigned char* cell_mask,
                                   const unsigned char* fixed, const int* mol_ptr, int N, int n_mol, float* g_ext,
                                   const int* state, void* stream) {
    if (!cellrelax_sizes_ok(N, n_mol) || !state || !(pressure == pressure) || (N > 0 && !force) ||
        (n_mol > 0 && (!stress || !cell || !x_ext || !weight || !mol_ptr || !g_ext)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::cellrelax_forces_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, force, stress, cell, x_ext,
                       weight, pressure, hydrostatic, cell_mask, fixed, mol_ptr, N, g_ext, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_cellrelax_apply(const float* x_ext, const float* cell0, const float* weight, const float* coef,
                                  const int* mol_ptr, int N, int n_mol, float* pos, float* cell, const int* state,
                                  void* stream) {
    if (!cellrelax_sizes_ok(N, n_mol) || !state || (N > 0 && !pos) ||
        (n_mol > 0 && (!x_ext || !cell0 || !weight || !coef || !mol_ptr || !cell)))
        return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::cellrelax_apply_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream, x_ext, cell0, weight, coef,
                       mol_ptr, N, pos, cell, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
