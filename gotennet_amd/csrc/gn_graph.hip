// gn_graph.hip -- radius graph + edge vectors (reference Distance.forward, layers.py:1588-1604,
// over torch_cluster.radius_graph(pos, r, batch, loop=True, max_num_neighbors)).
//
// Molecules are small (tens to hundreds of atoms) and contiguous in `batch`, so each
// target atom scans its own molecule: O(atoms-per-molecule) per thread, no cell list.
// Output layout = radius_graph's: target-major, sources ascending, strict d^2 < r^2
// in fp32 (x,y,z accumulated in that order), at most max_nbr sources per target
// (the first max_nbr in source order), self-loop included.
#include "gn_common.h"

namespace gn {

__device__ __forceinline__ bool within(const float* __restrict__ pos, int i, int j, float r2) {
    const float dx = pos[3 * i] - pos[3 * j];
    const float dy = pos[3 * i + 1] - pos[3 * j + 1];
    const float dz = pos[3 * i + 2] - pos[3 * j + 2];
    float d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    return d < r2;
}

__device__ __forceinline__ int molecule_start(const int64_t* __restrict__ batch, int i) {
    const int64_t b = batch[i];
    int s = i;
    while (s > 0 && batch[s - 1] == b) --s;
    return s;
}

__global__ void radius_count_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch, int N,
                                    float r2, int max_nbr, int* __restrict__ deg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t b = batch[i];
    int c = 0;
    for (int j = molecule_start(batch, i); j < N && batch[j] == b && c < max_nbr; ++j) c += within(pos, i, j, r2) ? 1 : 0;
    deg[i] = c;
}

// rowptr = exclusive scan of deg (length N+1)
__global__ void radius_fill_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch, int N,
                                   float r2, int max_nbr, const int64_t* __restrict__ rowptr, int64_t E,
                                   int64_t* __restrict__ edge_index, float* __restrict__ edge_vec,
                                   float* __restrict__ edge_diff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t b = batch[i];
    int64_t e = rowptr[i];
    int c = 0;
    for (int j = molecule_start(batch, i); j < N && batch[j] == b && c < max_nbr; ++j) {
        if (!within(pos, i, j, r2)) continue;
        edge_index[e] = j;           // row 0: source
        edge_index[E + e] = i;       // row 1: target
        const float vx = pos[3 * j] - pos[3 * i], vy = pos[3 * j + 1] - pos[3 * i + 1], vz = pos[3 * j + 2] - pos[3 * i + 2];
        edge_vec[3 * e] = vx; edge_vec[3 * e + 1] = vy; edge_vec[3 * e + 2] = vz;
        edge_diff[e] = (j == i) ? 0.0f : sqrtf(vx * vx + vy * vy + vz * vz);
        ++e; ++c;
    }
}

// edge vectors of a FIXED edge list for new positions (same arithmetic as radius_fill_kernel)
__global__ void edge_vectors_kernel(const float* __restrict__ pos, const int* __restrict__ src, const int* __restrict__ dst,
                                    int E, float* __restrict__ edge_vec, float* __restrict__ edge_diff) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int j = src[e], i = dst[e];
    const float vx = pos[3 * j] - pos[3 * i], vy = pos[3 * j + 1] - pos[3 * i + 1], vz = pos[3 * j + 2] - pos[3 * i + 2];
    edge_vec[3 * e] = vx; edge_vec[3 * e + 1] = vy; edge_vec[3 * e + 2] = vz;
    edge_diff[e] = (j == i) ? 0.0f : sqrtf(vx * vx + vy * vy + vz * vz);
}

// ---- by-source (CSC) view of a target-major edge list, stable: perm lists the CSR edge ids of every source in increasing
// order (= what torch.sort(src, stable=True) gives), without a sort: count -> scan -> scatter (integer atomics: the ORDER
// inside a bucket is arbitrary at this point, its CONTENT is not) -> rank every bucket entry among its bucket's ids.
__global__ void csc_count_kernel(const int* __restrict__ src, int E, int* __restrict__ cnt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) atomicAdd(cnt + src[e], 1);
}
// one workgroup: colptr = exclusive scan of cnt (N + 1 entries), cursor = a copy of colptr[0..N) for the scatter.
// `cursor` MAY alias `cnt` (the launcher scans in place: a thread reads cnt[n] before it writes cursor[n], and no other
// thread touches entry n) -- neither pointer is __restrict__
__global__ __launch_bounds__(1024) void csc_scan_kernel(const int* cnt, int N, int* __restrict__ colptr, int* cursor) {
    __shared__ int part[16];
    __shared__ int carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < N; base += 1024) {
        const int n = base + t;
        const int v = n < N ? cnt[n] : 0;
        int incl = v;                                            // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += part[w];
        if (n < N) {
            colptr[n] = before + incl - v;
            cursor[n] = before + incl - v;
        }
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    if (t == 0) colptr[N] = carry;
}
__global__ void csc_scatter_kernel(const int* __restrict__ src, int E, int* __restrict__ cursor, int* __restrict__ tmp) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) tmp[atomicAdd(cursor + src[e], 1)] = e;
}
// one wave per source: entry j of the bucket goes to position #{k : id_k < id_j} (ids are distinct) = the order a stable
// sort by source gives.  O(d^2 / 64) comparisons per bucket: short buckets (a molecular neighbour list: d <= 64) compare against
// uniform global loads; longer ones (hub atoms of an uncapped dense graph) stage the bucket through a per-wave LDS
// window of 1024 ids, one coalesced pass per window, and count against LDS broadcasts -- the same ranks, ~10x fewer cycles at
// d = 4096
__global__ __launch_bounds__(256) void csc_rank_kernel(const int* __restrict__ colptr, const int* __restrict__ tmp,
                                                       const int* __restrict__ dst, int N, int* __restrict__ perm,
                                                       int* __restrict__ tgt_by_src) {
    constexpr int WIN = 1024;
    __shared__ int win[4][WIN];
    const int wv = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wv, lane = threadIdx.x & 63;
    if (s >= N) return;
    const int p0 = colptr[s], d = colptr[s + 1] - p0;
    if (d <= 64) {
        if (lane < d) {
            const int id = tmp[p0 + lane];
            int r = 0;
            for (int k = 0; k < d; ++k) r += tmp[p0 + k] < id ? 1 : 0;
            perm[p0 + r] = id;
            tgt_by_src[p0 + r] = dst[id];
        }
        return;
    }
    for (int j0 = 0; j0 < d; j0 += 64) {             // (every lane runs every trip: the window loads are wave-wide)
        const int j = j0 + lane;
        const int id = j < d ? tmp[p0 + j] : 0x7fffffff;
        int r = 0;
        for (int w0 = 0; w0 < d; w0 += WIN) {
            const int wn = d - w0 < WIN ? d - w0 : WIN;
            __builtin_amdgcn_wave_barrier();
            for (int k = lane; k < wn; k += 64) win[wv][k] = tmp[p0 + w0 + k];
            __builtin_amdgcn_wave_barrier();
            for (int k = 0; k < wn; ++k) r += win[wv][k] < id ? 1 : 0;
        }
        if (j < d) {
            perm[p0 + r] = id;
            tgt_by_src[p0 + r] = dst[id];
        }
    }
}

// offsets of the molecules in a SORTED batch vector: mol_ptr[m] = first atom with batch >= m  (m = 0 .. n_mol).
// Precondition: batch non-decreasing (molecules contiguous, what a PyG Batch gives).  For ANY input every entry 0 .. n_mol is
// written with a value in [0, N] (the sequence -1, batch[0], .., batch[N-1], n_mol crosses every m at least once; negative and
// too-large entries are clamped), so a bad batch vector gives wrong molecule sums, never an out-of-bounds access
__global__ void molecule_ptr_kernel(const int64_t* __restrict__ batch, int N, int n_mol, int* __restrict__ mol_ptr) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n > N) return;
    int64_t lo = n == 0 ? 0 : batch[n - 1] + 1;                  // molecules lo .. hi start at atom n
    if (lo < 0) lo = 0;
    const int64_t hi = n == N ? n_mol : batch[n];
    for (int64_t m = lo; m <= hi && m <= n_mol; ++m) mol_ptr[m] = n;
}


// ================================================================================ periodic boundary conditions
// Conventions (include/gotennet_hip.h): cell fp32 [n_mol, 3, 3], ROWS are the lattice vectors a, b, c, one cell per entry of
// `batch` (a "molecule" is a periodic box); edge_shift int32 [E, 3]; edge_vec[e] = pos[j] - pos[i] + edge_shift[e] @ cell.
// Minimum image (radius_pbc_kernel): the host sends it only cells whose perpendicular widths are at least 2 * cutoff, so
// each pair has at most one image inside the cutoff and that image has all fractional coordinates in (-1/2, 1/2): rounding
// the fractional difference finds it, for skewed cells too.  Narrower cells: radius_pbc_images_kernel below.
struct Image {
    float vx, vy, vz, d2;
    int sx, sy, sz;
};
// v = d + s @ cell and |v|^2: the ONLY place a shifted edge vector is computed (the fixed-list kernel calls it with the
// stored shift, count and fill through image_of below).  The shift always passes through int, so a recomputed and a
// stored one give the same bits; fmaf in the order a, b, c; d^2 accumulated x, y, z as in within().
__device__ __forceinline__ Image shifted(float dx, float dy, float dz, int sx, int sy, int sz, const float* __restrict__ c) {
    const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
    Image im;
    im.sx = sx; im.sy = sy; im.sz = sz;
    im.vx = fmaf(fz, c[6], fmaf(fy, c[3], fmaf(fx, c[0], dx)));
    im.vy = fmaf(fz, c[7], fmaf(fy, c[4], fmaf(fx, c[1], dy)));
    im.vz = fmaf(fz, c[8], fmaf(fy, c[5], fmaf(fx, c[2], dz)));
    float d = im.vx * im.vx;
    d += im.vy * im.vy;
    d += im.vz * im.vz;
    im.d2 = d;
    return im;
}
// the minimum image of the pair (j -> i): d = pos[j] - pos[i], n_k = rint(d . column k of inv_cell), shift = -n
__device__ __forceinline__ Image image_of(const float* __restrict__ pos, int i, int j, const float* __restrict__ c,
                                          const float* __restrict__ ic) {
    const float dx = pos[3 * j] - pos[3 * i], dy = pos[3 * j + 1] - pos[3 * i + 1], dz = pos[3 * j + 2] - pos[3 * i + 2];
    const int nx = (int)rintf(fmaf(dz, ic[6], fmaf(dy, ic[3], dx * ic[0])));
    const int ny = (int)rintf(fmaf(dz, ic[7], fmaf(dy, ic[4], dx * ic[1])));
    const int nz = (int)rintf(fmaf(dz, ic[8], fmaf(dy, ic[5], dx * ic[2])));
    return shifted(dx, dy, dz, -nx, -ny, -nz, c);
}

// one thread per box: inverse and |det| of its cell (on the device, so a recorded step follows a changing cell)
__global__ void cell_prepare_kernel(const float* __restrict__ cell, int n_mol, float* __restrict__ inv_cell,
                                    float* __restrict__ volume) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_mol) return;
    const float* c = cell + 9 * m;
    const float a0 = c[0], a1 = c[1], a2 = c[2], b0 = c[3], b1 = c[4], b2 = c[5], c0 = c[6], c1 = c[7], c2 = c[8];
    const float k00 = b1 * c2 - b2 * c1, k01 = b2 * c0 - b0 * c2, k02 = b0 * c1 - b1 * c0;      // b x c
    const float det = a0 * k00 + a1 * k01 + a2 * k02;
    const float r = 1.0f / det;
    float* o = inv_cell + 9 * m;                       // inverse = adjugate / det (row-major)
    o[0] = k00 * r; o[1] = (a2 * c1 - a1 * c2) * r; o[2] = (a1 * b2 - a2 * b1) * r;
    o[3] = k01 * r; o[4] = (a0 * c2 - a2 * c0) * r; o[5] = (a2 * b0 - a0 * b2) * r;
    o[6] = k02 * r; o[7] = (a1 * c0 - a0 * c1) * r; o[8] = (a0 * b1 - a1 * b0) * r;
    volume[m] = fabsf(det);
}

// The box of target i: its atom range from mol_ptr (never a backward scan of `batch`: a box holds hundreds to thousands of
// atoms).  A batch entry outside [0, n_mol) is clamped and gn_molecule_ptr keeps every offset in [0, N]: a bad batch vector
// gives a wrong list, never an out-of-bounds access.
__device__ __forceinline__ int box_of(const int64_t* __restrict__ batch, int i, int n_mol) {
    const int64_t b = batch[i];
    return b < 0 ? 0 : (b >= n_mol ? n_mol - 1 : (int)b);
}

// One wave64 per target atom.  The lanes stride over the box's atoms, 64 per trip; a ballot plus the popcount of the lower
// lanes gives each hit its slot in source order, and the wave-uniform running count `c` carries the cap across trips: the
// first max_nbr sources in source order, deterministic, no atomics.  FILL = false counts (deg), FILL = true writes the list
// -- ONE body, so the two cannot disagree about which pair is a hit (a count and a fill that disagree write out of bounds;
// the fill checks its slot against E all the same).
template <bool FILL>
__global__ __launch_bounds__(256) void radius_pbc_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch,
                                                         const int* __restrict__ mol_ptr, const float* __restrict__ cell,
                                                         const float* __restrict__ inv_cell, int N, int n_mol, float r2,
                                                         int max_nbr, int* __restrict__ deg,
                                                         const int64_t* __restrict__ rowptr, int64_t E,
                                                         int64_t* __restrict__ edge_index, int* __restrict__ edge_shift,
                                                         float* __restrict__ edge_vec, float* __restrict__ edge_diff) {
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                // (wave-uniform)
    const int m = box_of(batch, i, n_mol);
    const int j0 = mol_ptr[m], j1 = mol_ptr[m + 1];
    const float* c = cell + 9 * m;
    const float* ic = inv_cell + 9 * m;
    const int64_t e0 = FILL ? rowptr[i] : 0;
    int cnt = 0;
    for (int base = j0; base < j1 && cnt < max_nbr; base += 64) {
        const int j = base + lane;
        Image im;
        bool hit = false;
        if (j < j1) {
            im = image_of(pos, i, j, c, ic);
            hit = im.d2 < r2;
        }
        const unsigned long long mask = __ballot(hit);
        if (FILL && hit) {
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            const int64_t e = e0 + slot;
            if (slot < max_nbr && e < E) {
                edge_index[e] = j;                     // row 0: source
                edge_index[E + e] = i;                 // row 1: target
                edge_shift[3 * e] = im.sx; edge_shift[3 * e + 1] = im.sy; edge_shift[3 * e + 2] = im.sz;
                edge_vec[3 * e] = im.vx; edge_vec[3 * e + 1] = im.vy; edge_vec[3 * e + 2] = im.vz;
                edge_diff[e] = (j == i) ? 0.0f : sqrtf(im.d2);
            }
        }
        cnt += __popcll(mask);
    }
    if (!FILL && lane == 0) deg[i] = cnt < max_nbr ? cnt : max_nbr;
}

// ---- several images per pair: cells narrower than 2 * cutoff (down to cutoff / 3).
// The self-loop of such a list is the edge with j == i AND shift 0; an atom's own periodic image (j == i, shift != 0) is a
// real neighbour at distance |s @ cell| > 0.
__device__ __forceinline__ bool is_self_loop(int j, int i, const Image& im) { return j == i && (im.sx | im.sy | im.sz) == 0; }

// One wave64 per target atom, as radius_pbc_kernel, over the candidates (source j, image t) of its box: the flattened index
// q = (j - j0) * n_img + t_flat, t_flat = (tx * ny + ty) * nz + tz (tx slowest), candidate shift s = -rint(f) + (t - R) with
// f the fractional difference of image_of (the same expression, so R = 0 IS the minimum-image kernel, bit for bit) and
// R = img_range[box] the host's per-axis bound (gn_radius_count_pbc_images in the header: every image inside the cutoff has
// |s_k + rint(f_k)| <= R_k).  Ascending q is: sources ascending, then shifts ascending lexicographically in (sx, sy, sz).
// Ballot + popcount of the lower lanes + the running wave-uniform count place each hit and carry the cap across trips: the
// first max_nbr hits in that order, no atomics.  (jb, tb) = candidate of lane 0 as (source offset, image index): 32-bit
// throughout, no product of the box size and n_img is ever formed.  FILL as above: one body for count and fill.
template <bool FILL>
__global__ __launch_bounds__(256) void radius_pbc_images_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch,
                                                                const int* __restrict__ mol_ptr, const float* __restrict__ cell,
                                                                const float* __restrict__ inv_cell,
                                                                const int* __restrict__ img_range, int N, int n_mol, float r2,
                                                                int max_nbr, int* __restrict__ deg,
                                                                const int64_t* __restrict__ rowptr, int64_t E,
                                                                int64_t* __restrict__ edge_index, int* __restrict__ edge_shift,
                                                                float* __restrict__ edge_vec, float* __restrict__ edge_diff) {
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                // (wave-uniform)
    const int m = box_of(batch, i, n_mol);
    const int j0 = mol_ptr[m], nj = mol_ptr[m + 1] - j0;
    const float* c = cell + 9 * m;
    const float* ic = inv_cell + 9 * m;
    // (the host refuses R > GN_PBC_MAX_IMAGE_RANGE; clamped all the same: a bad array costs images, never a long loop)
    const int Rx = min(max(img_range[3 * m], 0), GN_PBC_MAX_IMAGE_RANGE);
    const int Ry = min(max(img_range[3 * m + 1], 0), GN_PBC_MAX_IMAGE_RANGE);
    const int Rz = min(max(img_range[3 * m + 2], 0), GN_PBC_MAX_IMAGE_RANGE);
    const int ny = 2 * Ry + 1, nz = 2 * Rz + 1, nyz = ny * nz, n_img = (2 * Rx + 1) * nyz;      // <= 343
    const float pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
    const int64_t e0 = FILL ? rowptr[i] : 0;
    int cnt = 0, jb = 0, tb = 0;
    while (jb < nj && cnt < max_nbr) {
        int t = tb + lane;                             // < n_img + 64
        const int dj = t / n_img;
        t -= dj * n_img;
        const int j = j0 + jb + dj;
        Image im;
        bool hit = false;
        if (jb + dj < nj) {
            const int tx = t / nyz, r = t - tx * nyz, ty = r / nz, tz = r - ty * nz;
            const float dx = pos[3 * j] - pix, dy = pos[3 * j + 1] - piy, dz = pos[3 * j + 2] - piz;
            const int nx_ = (int)rintf(fmaf(dz, ic[6], fmaf(dy, ic[3], dx * ic[0])));
            const int ny_ = (int)rintf(fmaf(dz, ic[7], fmaf(dy, ic[4], dx * ic[1])));
            const int nz_ = (int)rintf(fmaf(dz, ic[8], fmaf(dy, ic[5], dx * ic[2])));
            im = shifted(dx, dy, dz, tx - Rx - nx_, ty - Ry - ny_, tz - Rz - nz_, c);
            hit = im.d2 < r2;                          // (the self-loop: 0 < r2)
        }
        const unsigned long long mask = __ballot(hit);
        if (FILL && hit) {
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            const int64_t e = e0 + slot;
            if (slot < max_nbr && e < E) {
                edge_index[e] = j;                     // row 0: source
                edge_index[E + e] = i;                 // row 1: target
                edge_shift[3 * e] = im.sx; edge_shift[3 * e + 1] = im.sy; edge_shift[3 * e + 2] = im.sz;
                edge_vec[3 * e] = im.vx; edge_vec[3 * e + 1] = im.vy; edge_vec[3 * e + 2] = im.vz;
                edge_diff[e] = is_self_loop(j, i, im) ? 0.0f : sqrtf(im.d2);
            }
        }
        cnt += __popcll(mask);
        tb += 64;                                      // the next 64 candidates
        jb += tb / n_img;
        tb %= n_img;
    }
    if (!FILL && lane == 0) deg[i] = cnt < max_nbr ? cnt : max_nbr;
}

// edge vectors of a FIXED periodic edge list for new positions / a new cell: the stored shift, no image search
__global__ void edge_vectors_pbc_kernel(const float* __restrict__ pos, const int* __restrict__ src, const int* __restrict__ dst,
                                        const int* __restrict__ shift, const float* __restrict__ cell,
                                        const int64_t* __restrict__ batch, int E, int n_mol, float* __restrict__ edge_vec,
                                        float* __restrict__ edge_diff) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int j = src[e], i = dst[e];
    const float dx = pos[3 * j] - pos[3 * i], dy = pos[3 * j + 1] - pos[3 * i + 1], dz = pos[3 * j + 2] - pos[3 * i + 2];
    const Image im = shifted(dx, dy, dz, shift[3 * e], shift[3 * e + 1], shift[3 * e + 2], cell + 9 * box_of(batch, i, n_mol));
    edge_vec[3 * e] = im.vx; edge_vec[3 * e + 1] = im.vy; edge_vec[3 * e + 2] = im.vz;
    edge_diff[e] = is_self_loop(j, i, im) ? 0.0f : sqrtf(im.d2);     // (an atom's own image, shift != 0, is a real edge)
}

// ================================================================================ is a stored list still the radius graph?
// gn_radius_verify*: every target walks the candidates of its search in the search's order and asks the search's own
// predicate (within(), image_of(), shifted()): hit number k must be stored entry k of the target's CSR row (source, and
// shift for a periodic list), up to the cap, and the number of kept hits must be the row's degree.  Nothing is written but
// a per-target flag and the sticky word: a row that differs sets state[0] = 1 (plain stores of the same value from every
// such row; nobody clears it on the device).  Same thread mapping as the searches.
__device__ __forceinline__ void report_row(bool differs, int i, int* __restrict__ row_flag, int* __restrict__ state) {
    row_flag[i] = differs ? 1 : 0;
    if (differs) state[0] = 1;
}
// is hit number `slot` of a target something else than entry `slot` of its stored row [e0, e0 + d)?  (shift == nullptr: a
// list without shifts.  The slot is held to [0, E) all the same: a bad rowptr reads nothing out of bounds.)
__device__ __forceinline__ bool entry_differs(const int* __restrict__ src, const int* __restrict__ shift, int slot, int d,
                                              int e0, int E, int j, int sx, int sy, int sz) {
    const int e = e0 + slot;
    if (slot >= d || e < 0 || e >= E) return true;
    if (src[e] != j) return true;
    return shift != nullptr && (shift[3 * e] != sx || shift[3 * e + 1] != sy || shift[3 * e + 2] != sz);
}

// one thread per target: radius_count_kernel's loop
__global__ void radius_verify_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch, int N, float r2,
                                     int max_nbr, const int* __restrict__ rowptr, const int* __restrict__ src, int E,
                                     int* __restrict__ row_flag, int* __restrict__ state) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t b = batch[i];
    const int e0 = rowptr[i], d = rowptr[i + 1] - e0;
    int c = 0;
    bool differs = false;
    for (int j = molecule_start(batch, i); j < N && batch[j] == b && c < max_nbr; ++j) {
        if (!within(pos, i, j, r2)) continue;
        differs |= entry_differs(src, nullptr, c, d, e0, E, j, 0, 0, 0);
        ++c;
    }
    report_row(differs || c != d, i, row_flag, state);
}

// one wave64 per target: radius_pbc_kernel's loop
__global__ __launch_bounds__(256) void radius_verify_pbc_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch,
                                                                const int* __restrict__ mol_ptr, const float* __restrict__ cell,
                                                                const float* __restrict__ inv_cell, int N, int n_mol, float r2,
                                                                int max_nbr, const int* __restrict__ rowptr,
                                                                const int* __restrict__ src, const int* __restrict__ shift, int E,
                                                                int* __restrict__ row_flag, int* __restrict__ state) {
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                // (wave-uniform)
    const int m = box_of(batch, i, n_mol);
    const int j0 = mol_ptr[m], j1 = mol_ptr[m + 1];
    const float* c = cell + 9 * m;
    const float* ic = inv_cell + 9 * m;
    const int e0 = rowptr[i], d = rowptr[i + 1] - e0;
    int cnt = 0;
    bool differs = false;
    for (int base = j0; base < j1 && cnt < max_nbr; base += 64) {
        const int j = base + lane;
        Image im;
        bool hit = false;
        if (j < j1) {
            im = image_of(pos, i, j, c, ic);
            hit = im.d2 < r2;
        }
        const unsigned long long mask = __ballot(hit);
        if (hit) {
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < max_nbr) differs |= entry_differs(src, shift, slot, d, e0, E, j, im.sx, im.sy, im.sz);
        }
        cnt += __popcll(mask);
    }
    const bool any = __ballot(differs) != 0ull || (cnt < max_nbr ? cnt : max_nbr) != d;
    if (lane == 0) report_row(any, i, row_flag, state);
}

// one wave64 per target: radius_pbc_images_kernel's loop over the flattened (source, image) candidates
__global__ __launch_bounds__(256) void radius_verify_pbc_images_kernel(
    const float* __restrict__ pos, const int64_t* __restrict__ batch, const int* __restrict__ mol_ptr,
    const float* __restrict__ cell, const float* __restrict__ inv_cell, const int* __restrict__ img_range, int N, int n_mol,
    float r2, int max_nbr, const int* __restrict__ rowptr, const int* __restrict__ src, const int* __restrict__ shift, int E,
    int* __restrict__ row_flag, int* __restrict__ state) {
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                // (wave-uniform)
    const int m = box_of(batch, i, n_mol);
    const int j0 = mol_ptr[m], nj = mol_ptr[m + 1] - j0;
    const float* c = cell + 9 * m;
    const float* ic = inv_cell + 9 * m;
    const int Rx = min(max(img_range[3 * m], 0), GN_PBC_MAX_IMAGE_RANGE);
    const int Ry = min(max(img_range[3 * m + 1], 0), GN_PBC_MAX_IMAGE_RANGE);
    const int Rz = min(max(img_range[3 * m + 2], 0), GN_PBC_MAX_IMAGE_RANGE);
    const int ny = 2 * Ry + 1, nz = 2 * Rz + 1, nyz = ny * nz, n_img = (2 * Rx + 1) * nyz;
    const float pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
    const int e0 = rowptr[i], d = rowptr[i + 1] - e0;
    int cnt = 0, jb = 0, tb = 0;
    bool differs = false;
    while (jb < nj && cnt < max_nbr) {
        int t = tb + lane;
        const int dj = t / n_img;
        t -= dj * n_img;
        const int j = j0 + jb + dj;
        Image im;
        bool hit = false;
        if (jb + dj < nj) {
            const int tx = t / nyz, r = t - tx * nyz, ty = r / nz, tz = r - ty * nz;
            const float dx = pos[3 * j] - pix, dy = pos[3 * j + 1] - piy, dz = pos[3 * j + 2] - piz;
            const int nx_ = (int)rintf(fmaf(dz, ic[6], fmaf(dy, ic[3], dx * ic[0])));
            const int ny_ = (int)rintf(fmaf(dz, ic[7], fmaf(dy, ic[4], dx * ic[1])));
            const int nz_ = (int)rintf(fmaf(dz, ic[8], fmaf(dy, ic[5], dx * ic[2])));
            im = shifted(dx, dy, dz, tx - Rx - nx_, ty - Ry - ny_, tz - Rz - nz_, c);
            hit = im.d2 < r2;
        }
        const unsigned long long mask = __ballot(hit);
        if (hit) {
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < max_nbr) differs |= entry_differs(src, shift, slot, d, e0, E, j, im.sx, im.sy, im.sz);
        }
        cnt += __popcll(mask);
        tb += 64;
        jb += tb / n_img;
        tb %= n_img;
    }
    const bool any = __ballot(differs) != 0ull || (cnt < max_nbr ? cnt : max_nbr) != d;
    if (lane == 0) report_row(any, i, row_flag, state);
}

// changed[m] = the number of flagged targets of molecule m.  One wave64 per molecule over its atom range, ballot +
// popcount per trip: an integer count in a fixed order.
__global__ __launch_bounds__(256) void rows_changed_kernel(const int* __restrict__ row_flag, const int* __restrict__ mol_ptr,
                                                           int N, int n_mol, int* __restrict__ changed) {
    const int m = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n_mol) return;                            // (wave-uniform)
    const int j0 = max(mol_ptr[m], 0), j1 = min(mol_ptr[m + 1], N);
    int c = 0;
    for (int base = j0; base < j1; base += 64) {
        const int j = base + lane;
        c += __popcll(__ballot(j < j1 && row_flag[j] != 0));
    }
    if (lane == 0) changed[m] = c;
}

// out[m] = (1 / volume[m]) sum_{e in box m} r_e (x) dE/dr_e,  dE/dr_e = g_vec + g_diff r / |r| (gn_pos_scatter's expression).
// One workgroup per box over its contiguous edge range; nine sums, wave_sum, then the waves in order through LDS: no
// atomics, identical inputs give identical bits.  An empty box gives zeros.
__global__ __launch_bounds__(256) void virial_kernel(const float* __restrict__ g_vec, const float* __restrict__ g_diff,
                                                     const float* __restrict__ vec, const int* __restrict__ rowptr,
                                                     const int* __restrict__ mol_ptr, const float* __restrict__ volume,
                                                     float* __restrict__ out) {
    __shared__ float part[4][9];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e0 = rowptr[mol_ptr[m]], e1 = rowptr[mol_ptr[m + 1]];
    float s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.f;
    for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
        const float x = vec[3 * e], y = vec[3 * e + 1], z = vec[3 * e + 2];
        const float gd = g_diff[e];
        float rx = g_vec[3 * e], ry = g_vec[3 * e + 1], rz = g_vec[3 * e + 2];
        if (gd != 0.f) {
            const float q = gd / sqrtf(x * x + y * y + z * z);
            rx += q * x; ry += q * y; rz += q * z;
        }
        s[0] += x * rx; s[1] += x * ry; s[2] += x * rz;
        s[3] += y * rx; s[4] += y * ry; s[5] += y * rz;
        s[6] += z * rx; s[7] += z * ry; s[8] += z * rz;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float t = wave_sum(s[k]);
        if (lane == 0) part[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        const float t = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
        out[9 * m + k] = t / volume[m];
    }
}

}  // namespace gn

extern "C" int gn_build_csc(const int* src, const int* dst, int E, int N, int* colptr, int* perm, int* tgt_by_src,
                            int* work, void* stream) {
    if (E < 0 || N < 0 || !colptr || (E > 0 && (!src || !dst || !perm || !tgt_by_src || !work))) return GN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    int* cnt = work;                                             // [N] counts, then the scatter cursor
    int* tmp = work + N;                                         // [E] bucket contents before ranking
    if (N > 0 && hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)N, st) != hipSuccess) return (int)hipGetLastError();
    if (E > 0) hipLaunchKernelGGL(gn::csc_count_kernel, dim3((E + 255) / 256), dim3(256), 0, st, src, E, cnt);
    hipLaunchKernelGGL(gn::csc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, N, colptr, cnt);
    if (E > 0) {
        hipLaunchKernelGGL(gn::csc_scatter_kernel, dim3((E + 255) / 256), dim3(256), 0, st, src, E, cnt, tmp);
        hipLaunchKernelGGL(gn::csc_rank_kernel, dim3((N + 3) / 4), dim3(256), 0, st, colptr, tmp, dst, N, perm, tgt_by_src);
    }
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_molecule_ptr(const int64_t* batch, int N, int n_mol, int* mol_ptr, void* stream) {
    if (N < 0 || n_mol < 0 || !mol_ptr || (N > 0 && !batch)) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::molecule_ptr_kernel, dim3((N + 256) / 256), dim3(256), 0, (hipStream_t)stream, batch, N, n_mol, mol_ptr);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_edge_vectors(const float* pos, const int* src, const int* dst, int E, float* edge_vec,
                               float* edge_diff, void* stream) {
    if (E < 0) return GN_ERR_BAD_ARG;
    if (E == 0) return GN_OK;
    hipLaunchKernelGGL(gn::edge_vectors_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       pos, src, dst, E, edge_vec, edge_diff);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_count(const float* pos, const int64_t* batch, int N, float cutoff, int max_nbr,
                               int* deg, void* stream) {
    if (N < 0 || max_nbr <= 0) return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::radius_count_kernel, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream,
                       pos, batch, N, cutoff * cutoff, max_nbr, deg);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_fill(const float* pos, const int64_t* batch, int N, float cutoff, int max_nbr,
                              const int64_t* rowptr, int64_t E, int64_t* edge_index, float* edge_vec,
                              float* edge_diff, void* stream) {
    if (N < 0 || max_nbr <= 0 || E < 0) return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::radius_fill_kernel, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream,
                       pos, batch, N, cutoff * cutoff, max_nbr, rowptr, E, edge_index, edge_vec, edge_diff);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

/* ---- periodic boundary conditions ---------------------------------------------------------------------------- */
extern "C" int gn_cell_prepare(const float* cell, int n_mol, float* inv_cell, float* volume, void* stream) {
    if (n_mol < 0 || (n_mol > 0 && (!cell || !inv_cell || !volume))) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::cell_prepare_kernel, dim3((n_mol + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       cell, n_mol, inv_cell, volume);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_count_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                   const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, int* deg,
                                   void* stream) {
    if (N < 0 || max_nbr <= 0 || n_mol < 0 || (N > 0 && (n_mol < 1 || !pos || !batch || !mol_ptr || !cell || !inv_cell || !deg)))
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::radius_pbc_kernel<false>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       pos, batch, mol_ptr, cell, inv_cell, N, n_mol, cutoff * cutoff, max_nbr, deg,
                       (const int64_t*)nullptr, (int64_t)0, (int64_t*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_fill_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                  const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr,
                                  const int64_t* rowptr, int64_t E, int64_t* edge_index, int* edge_shift,
                                  float* edge_vec, float* edge_diff, void* stream) {
    if (N < 0 || max_nbr <= 0 || E < 0 || n_mol < 0 || (N > 0 && (n_mol < 1 || !pos || !batch || !mol_ptr || !cell || !inv_cell || !rowptr)))
        return GN_ERR_BAD_ARG;
    if (E > 0 && (!edge_index || !edge_shift || !edge_vec || !edge_diff)) return GN_ERR_BAD_ARG;
    if (N == 0 || E == 0) return GN_OK;
    hipLaunchKernelGGL(gn::radius_pbc_kernel<true>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       pos, batch, mol_ptr, cell, inv_cell, N, n_mol, cutoff * cutoff, max_nbr, (int*)nullptr,
                       rowptr, E, edge_index, edge_shift, edge_vec, edge_diff);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

static bool radius_pbc_args_ok(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                               const float* inv_cell, const int* img_range, int N, int n_mol, int max_nbr) {
    if (N < 0 || max_nbr <= 0 || n_mol < 0) return false;
    return N == 0 || (n_mol >= 1 && pos && batch && mol_ptr && cell && inv_cell && img_range);
}

extern "C" int gn_radius_count_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                          const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff,
                                          int max_nbr, int* deg, void* stream) {
    if (!radius_pbc_args_ok(pos, batch, mol_ptr, cell, inv_cell, img_range, N, n_mol, max_nbr) || (N > 0 && !deg))
        return GN_ERR_BAD_ARG;
    if (N == 0) return GN_OK;
    hipLaunchKernelGGL(gn::radius_pbc_images_kernel<false>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       pos, batch, mol_ptr, cell, inv_cell, img_range, N, n_mol, cutoff * cutoff, max_nbr, deg,
                       (const int64_t*)nullptr, (int64_t)0, (int64_t*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_fill_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                         const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff,
                                         int max_nbr, const int64_t* rowptr, int64_t E, int64_t* edge_index,
                                         int* edge_shift, float* edge_vec, float* edge_diff, void* stream) {
    if (!radius_pbc_args_ok(pos, batch, mol_ptr, cell, inv_cell, img_range, N, n_mol, max_nbr) || E < 0 || (N > 0 && !rowptr))
        return GN_ERR_BAD_ARG;
    if (E > 0 && (!edge_index || !edge_shift || !edge_vec || !edge_diff)) return GN_ERR_BAD_ARG;
    if (N == 0 || E == 0) return GN_OK;
    hipLaunchKernelGGL(gn::radius_pbc_images_kernel<true>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       pos, batch, mol_ptr, cell, inv_cell, img_range, N, n_mol, cutoff * cutoff, max_nbr, (int*)nullptr,
                       rowptr, E, edge_index, edge_shift, edge_vec, edge_diff);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_edge_vectors_pbc(const float* pos, const int* src, const int* dst, const int* shift, const float* cell,
                                   const int64_t* batch, int E, int n_mol, float* edge_vec, float* edge_diff, void* stream) {
    if (E < 0 || n_mol < 0) return GN_ERR_BAD_ARG;
    if (E == 0) return GN_OK;
    if (n_mol < 1 || !pos || !src || !dst || !shift || !cell || !batch || !edge_vec || !edge_diff) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::edge_vectors_pbc_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       pos, src, dst, shift, cell, batch, E, n_mol, edge_vec, edge_diff);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_virial(const float* g_vec, const float* g_diff, const float* edge_vec, const int* rowptr,
                         const int* mol_ptr, int n_mol, const float* volume, float* out, void* stream) {
    if (n_mol < 0) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    if (!rowptr || !mol_ptr || !volume || !out) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::virial_kernel, dim3(n_mol), dim3(256), 0, (hipStream_t)stream,
                       g_vec, g_diff, edge_vec, rowptr, mol_ptr, volume, out);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

/* ---- is a stored list still the radius graph of these positions? ----------------------------------------------- */
static bool radius_verify_args_ok(const float* pos, const int64_t* batch, const int* mol_ptr, int N, int n_mol, int max_nbr,
                                  const int* rowptr, const int* src, int E, const int* row_flag, const int* changed,
                                  const int* state) {
    if (N < 0 || n_mol < 0 || max_nbr <= 0 || E < 0 || !state || (n_mol > 0 && (!changed || !mol_ptr))) return false;
    return N == 0 || (n_mol >= 1 && pos && batch && rowptr && row_flag && (E == 0 || src));
}
static int rows_changed(const int* row_flag, const int* mol_ptr, int N, int n_mol, int* changed, hipStream_t st) {
    if (n_mol > 0)
        hipLaunchKernelGGL(gn::rows_changed_kernel, dim3((n_mol + 3) / 4), dim3(256), 0, st, row_flag, mol_ptr, N, n_mol, changed);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_verify(const float* pos, const int64_t* batch, const int* mol_ptr, int N, int n_mol, float cutoff,
                                int max_nbr, const int* rowptr, const int* src, int E, int* row_flag, int* changed,
                                int* state, void* stream) {
    if (!radius_verify_args_ok(pos, batch, mol_ptr, N, n_mol, max_nbr, rowptr, src, E, row_flag, changed, state))
        return GN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (N > 0)
        hipLaunchKernelGGL(gn::radius_verify_kernel, dim3((N + 127) / 128), dim3(128), 0, st, pos, batch, N, cutoff * cutoff,
                           max_nbr, rowptr, src, E, row_flag, state);
    return rows_changed(row_flag, mol_ptr, N, n_mol, changed, st);
}

extern "C" int gn_radius_verify_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                    const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, const int* rowptr,
                                    const int* src, const int* shift, int E, int* row_flag, int* changed, int* state,
                                    void* stream) {
    if (!radius_verify_args_ok(pos, batch, mol_ptr, N, n_mol, max_nbr, rowptr, src, E, row_flag, changed, state) ||
        (N > 0 && (!cell || !inv_cell)) || (E > 0 && !shift))
        return GN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (N > 0)
        hipLaunchKernelGGL(gn::radius_verify_pbc_kernel, dim3((N + 3) / 4), dim3(256), 0, st, pos, batch, mol_ptr, cell,
                           inv_cell, N, n_mol, cutoff * cutoff, max_nbr, rowptr, src, shift, E, row_flag, state);
    return rows_changed(row_flag, mol_ptr, N, n_mol, changed, st);
}

extern "C" int gn_radius_verify_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                           const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff,
                                           int max_nbr, const int* rowptr, const int* src, const int* shift, int E,
                                           int* row_flag, int* changed, int* state, void* stream) {
    if (!radius_verify_args_ok(pos, batch, mol_ptr, N, n_mol, max_nbr, rowptr, src, E, row_flag, changed, state) ||
        (N > 0 && (!cell || !inv_cell || !img_range)) || (E > 0 && !shift))
        return GN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (N > 0)
        hipLaunchKernelGGL(gn::radius_verify_pbc_images_kernel, dim3((N + 3) / 4), dim3(256), 0, st, pos, batch, mol_ptr,
                           cell, inv_cell, img_range, N, n_mol, cutoff * cutoff, max_nbr, rowptr, src, shift, E, row_flag,
                           state);
    return rows_changed(row_flag, mol_ptr, N, n_mol, changed, st);
}
