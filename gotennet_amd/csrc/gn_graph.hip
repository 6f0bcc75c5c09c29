// gn_graph.hip -- radius graph + edge vectors (reference Distance.forward, layers.py:1588-1604,
// over torch_cluster.radius_graph(pos, r, batch, loop=True, max_num_neighbors)).
//
// Molecules are small (tens to hundreds of atoms) and contiguous in `batch`, so each
// target atom scans its own molecule: O(atoms-per-molecule) per thread, no cell list.
// Output layout = radius_graph's: target-major, sources ascending, strict d^2 < r^2
// in fp32 (x,y,z accumulated in that order), at most max_nbr sources per target
// (the first max_nbr in source order), self-loop included.
//
// Three searches (isolated molecules, periodic minimum image, periodic multi-image), each asked three questions (how many
// neighbours, which, is a stored list still the answer).  A search is a WALK: it enumerates a target's candidates in the
// list's order, decides which are hits and numbers the hits kept under the cap.  A question is a SINK: a small struct,
// passed to the kernel by value, that the walk hands every kept hit.  Two walks (one thread per target for the open search,
// one wave per target for the periodic ones) times three sinks: count, fill and verify of one search run the SAME loop and
// the SAME predicate, so they cannot disagree about which pair is a hit or where it goes (a count and a fill that disagree
// write out of bounds; a verify that disagrees with the search at the threshold bit breaks an MD trajectory).
#include "gn_common.h"

namespace gn {

// A candidate of target i: source j under the lattice shift s.  v = pos[j] - pos[i] + s @ cell, d2 = |v|^2.
struct Image {
    float vx, vy, vz, d2;
    int sx, sy, sz;
};
// |v|^2 accumulated x, y, z: the order of every hit test and every stored distance in this file
__device__ __forceinline__ float norm2(float x, float y, float z) {
    float d = x * x;
    d += y * y;
    d += z * z;
    return d;
}
// the candidate of an open search: no cell, shift 0
__device__ __forceinline__ Image unshifted(float dx, float dy, float dz) {
    return Image{dx, dy, dz, norm2(dx, dy, dz), 0, 0, 0};
}
// v = d + s @ cell and |v|^2: the ONLY place a shifted edge vector is computed (the fixed-list kernel calls it with the
// stored shift, the periodic walk with the candidate's).  The shift always passes through int, so a recomputed and a
// stored one give the same bits; fmaf in the order a, b, c.
__device__ __forceinline__ Image shifted(float dx, float dy, float dz, int sx, int sy, int sz, const float* __restrict__ c) {
    const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
    Image im;
    im.sx = sx; im.sy = sy; im.sz = sz;
    im.vx = fmaf(fz, c[6], fmaf(fy, c[3], fmaf(fx, c[0], dx)));
    im.vy = fmaf(fz, c[7], fmaf(fy, c[4], fmaf(fx, c[1], dy)));
    im.vz = fmaf(fz, c[8], fmaf(fy, c[5], fmaf(fx, c[2], dz)));
    im.d2 = norm2(im.vx, im.vy, im.vz);
    return im;
}
// The self-loop is the edge with j == i AND shift 0; an atom's own periodic image (j == i, shift != 0: cells narrower than
// 2 * cutoff) is a real neighbour at distance |s @ cell| > 0.  (Open and minimum-image lists: j == i implies shift 0.)
__device__ __forceinline__ bool is_self_loop(int j, int i, const Image& im) { return j == i && (im.sx | im.sy | im.sz) == 0; }

// The ONLY place an edge is written: slot e of a list of E edges (the caller has checked e < E).  INDEX = false: the list is
// already stored (the fixed-list kernels); SHIFTS = false: a list without shifts, or with stored ones.  Compile-time both: the
// fill's loop carries no test of a pointer.
template <bool INDEX, bool SHIFTS>
__device__ __forceinline__ void store_edge(int64_t e, int64_t E, int j, int i, const Image& im, int64_t* __restrict__ edge_index,
                                           int* __restrict__ edge_shift, float* __restrict__ edge_vec,
                                           float* __restrict__ edge_diff) {
    if (INDEX) {
        edge_index[e] = j;                             // row 0: source
        edge_index[E + e] = i;                         // row 1: target
    }
    if (SHIFTS) {
        edge_shift[3 * e] = im.sx; edge_shift[3 * e + 1] = im.sy; edge_shift[3 * e + 2] = im.sz;
    }
    edge_vec[3 * e] = im.vx; edge_vec[3 * e + 1] = im.vy; edge_vec[3 * e + 2] = im.vz;
    edge_diff[e] = is_self_loop(j, i, im) ? 0.0f : sqrtf(im.d2);
}

// ================================================================================ the three sinks
// What a walk asks of a sink, per thread: begin(i) before the first candidate of target i; hit(i, j, slot, im) for hit number
// `slot` < max_nbr of the target, in the list's order; flag() = this thread saw something to report; finish(i, kept, any) once
// per target with kept = min(hits, max_nbr) and any = the OR of flag() over the threads that walked the target.

// deg[i] = the number of neighbours kept
struct CountSink {
    int* __restrict__ deg;
    __device__ __forceinline__ void begin(int) {}
    __device__ __forceinline__ void hit(int, int, int, const Image&) {}
    __device__ __forceinline__ bool flag() const { return false; }
    __device__ __forceinline__ void finish(int i, int kept, bool) const { deg[i] = kept; }
};

// the list itself: rowptr = exclusive scan of deg (length N + 1), E = rowptr[N].  The slot is checked against E all the same.
// SHIFTS = false: the open search, whose list has no shift array (decided when the kernel is compiled, not per hit).
template <bool SHIFTS>
struct FillSink {
    const int64_t* __restrict__ rowptr;
    int64_t E;
    int64_t* __restrict__ edge_index;
    int* __restrict__ edge_shift;                      // (unused without SHIFTS)
    float* __restrict__ edge_vec;
    float* __restrict__ edge_diff;
    int64_t e0 = 0;
    __device__ __forceinline__ void begin(int i) { e0 = rowptr[i]; }
    __device__ __forceinline__ void hit(int i, int j, int slot, const Image& im) const {
        const int64_t e = e0 + slot;
        if (e < E) store_edge<true, SHIFTS>(e, E, j, i, im, edge_index, edge_shift, edge_vec, edge_diff);
    }
    __device__ __forceinline__ bool flag() const { return false; }
    __device__ __forceinline__ void finish(int, int, bool) const {}
};

// Is a stored list still the radius graph?  Hit number k must be stored entry k of the target's CSR row (source, and shift for
// a periodic list), up to the cap, and the number of kept hits must be the row's degree.  Nothing is written but a per-target
// flag and the sticky word: a row that differs sets state[0] = 1 (plain stores of the same value from every such row; nobody
// clears it on the device).
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
struct VerifySink {
    const int* __restrict__ rowptr;                    // int32 [N + 1]: the stored list in CSR form
    const int* __restrict__ src;
    const int* __restrict__ shift;                     // nullptr: the open search
    int E;
    int* __restrict__ row_flag;
    int* __restrict__ state;
    int e0 = 0, d = 0;
    bool differs = false;
    __device__ __forceinline__ void begin(int i) { e0 = rowptr[i]; d = rowptr[i + 1] - e0; }
    __device__ __forceinline__ void hit(int, int j, int slot, const Image& im) {
        differs |= entry_differs(src, shift, slot, d, e0, E, j, im.sx, im.sy, im.sz);
    }
    __device__ __forceinline__ bool flag() const { return differs; }
    __device__ __forceinline__ void finish(int i, int kept, bool any) const { report_row(any || kept != d, i, row_flag, state); }
};

// ================================================================================ isolated molecules: one thread per target
__device__ __forceinline__ int molecule_start(const int64_t* __restrict__ batch, int i) {
    const int64_t b = batch[i];
    int s = i;
    while (s > 0 && batch[s - 1] == b) --s;
    return s;
}

// The open walk (gn_radius_count / _fill / _verify): the target's own molecule, sources ascending, until the cap is reached.
template <class Sink>
__global__ void radius_thread_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch, int N, float r2,
                                     int max_nbr, Sink sink) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t b = batch[i];
    sink.begin(i);
    int cnt = 0;
    for (int j = molecule_start(batch, i); j < N && batch[j] == b && cnt < max_nbr; ++j) {
        const Image im = unshifted(pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]);
        if (!(im.d2 < r2)) continue;
        sink.hit(i, j, cnt, im);
        ++cnt;
    }
    sink.finish(i, cnt, sink.flag());
}

// edge vectors of a FIXED edge list for new positions (the open search's arithmetic)
__global__ void edge_vectors_kernel(const float* __restrict__ pos, const int* __restrict__ src, const int* __restrict__ dst,
                                    int E, float* __restrict__ edge_vec, float* __restrict__ edge_diff) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int j = src[e], i = dst[e];
    const Image im = unshifted(pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]);
    store_edge<false, false>(e, E, j, i, im, nullptr, nullptr, edge_vec, edge_diff);
}

// ---- by-source (CSC) view of a target-major edge list, stable: perm lists the CSR edge ids of every source in increasing
// order (= what torch.sort(src, stable=True) gives), without a sort: count -> scan -> scatter (integer atomics: the ORDER
// inside a bucket is arbitrary at this point, its CONTENT is not) -> rank every bucket entry among its bucket's ids.
__global__ void csc_count_kernel(const int* __restrict__ src, int E, int* __restrict__ cnt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) atomicAdd(cnt + src[e], 1);
}
// One workgroup of 1024 threads: the exclusive scan of v[0 .. N), handed to write(n, sum of v[0 .. n)) by the thread that read
// v[n]; returns the total (to every thread).  Inclusive scan inside each wave, the waves' sums through LDS, a carry across
// trips of 1024 entries.  A thread reads v[n] before it calls write(n, .) and no other thread touches entry n: `write` may
// store over v itself.  The one scan of this file: csc_scan_kernel and degree_scan_kernel are its two callers.
template <class Write>
__device__ __forceinline__ int block_exclusive_scan(const int* v_in, int N, Write write) {
    __shared__ int part[16];
    __shared__ int carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < N; base += 1024) {
        const int n = base + t;
        const int v = n < N ? v_in[n] : 0;
        int incl = v;                                            // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += part[w];
        if (n < N) write(n, before + incl - v);
        __syncthreads();
        if (t == 1023) carry = before + incl;
        __syncthreads();
    }
    return carry;
}
// one workgroup: colptr = exclusive scan of cnt (N + 1 entries), cursor = a copy of colptr[0..N) for the scatter.
// `cursor` MAY alias `cnt` (the launcher scans in place) -- neither pointer is __restrict__
__global__ __launch_bounds__(1024) void csc_scan_kernel(const int* cnt, int N, int* __restrict__ colptr, int* cursor) {
    const int total = block_exclusive_scan(cnt, N, [=](int n, int s) {
        colptr[n] = s;
        cursor[n] = s;
    });
    if (threadIdx.x == 0) colptr[N] = total;
}
// gn_degree_scan: rowptr64 = the exclusive scan of the searches' deg (N + 1 entries, int64: what FillSink reads), the total
// also into the device word n_edges -- what torch.cumsum and a host read of its last entry give graph.distance*
__global__ __launch_bounds__(1024) void degree_scan_kernel(const int* __restrict__ deg, int N, int64_t* __restrict__ rowptr64,
                                                           int* __restrict__ n_edges) {
    const int total = block_exclusive_scan(deg, N, [=](int n, int s) { rowptr64[n] = s; });
    if (threadIdx.x == 0) {
        rowptr64[N] = total;
        n_edges[0] = total;
    }
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

// gn_graph_refresh's first launch: what gn_build_csr writes (csr_split_edge: the same body), and the zeroes that
// gn_build_csc's memset and gn_out_degree's caller supply -- in a kernel, so a recorded chain holds kernel nodes only.
// Grid over max(E, N + 1).
__global__ void refresh_split_kernel(const int64_t* __restrict__ ei, int E, int N, int* __restrict__ src, int* __restrict__ dst,
                                     int* __restrict__ rowptr, int* __restrict__ cnt, int* __restrict__ outdeg) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) {
        cnt[t] = 0;
        if (outdeg != nullptr) outdeg[t] = 0;
    }
    if (E == 0) {
        if (t <= N) rowptr[t] = 0;
        return;
    }
    if (t < E) csr_split_edge(ei, t, E, N, src, dst, rowptr);
}

// gn_padded_tail: the slots [E_real, capacity) of a [2, capacity] list, E_real = rowptr64[N] read HERE, as self-loops of the
// dummy atoms N .. N + n_pad - 1 (shift, vector and distance 0), dealt in the balanced contiguous partition of
// graph.PaddedLayout.tail_degrees: P = capacity - E_real slots, the first P % n_pad dummies get P / n_pad + 1, the others
// P / n_pad.  One thread per tail slot t = slot - E_real; its dummy is closed-form: with q = P / n_pad, r = P % n_pad the
// first r (q + 1) slots belong to t / (q + 1), the rest to r + (t - r (q + 1)) / q  (q >= 1 because P >= n_pad).
// E_real outside [N, capacity - n_pad] -- a count the layout's bound excludes -- writes nothing and sets the sticky word.
template <bool SHIFTS>
__global__ void padded_tail_kernel(const int64_t* __restrict__ rowptr64, int N, int n_pad, int64_t capacity,
                                   int64_t* __restrict__ edge_index, int* __restrict__ edge_shift, float* __restrict__ edge_vec,
                                   float* __restrict__ edge_diff, int* __restrict__ state) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t E_real = rowptr64[N];
    if (E_real < N || E_real > capacity - n_pad) {
        if (t == 0) state[0] = 1;
        return;
    }
    const int64_t P = capacity - E_real;
    if (t >= P) return;
    const int64_t q = P / n_pad, r = P % n_pad, head = r * (q + 1);
    const int k = N + (int)(t < head ? t / (q + 1) : r + (t - head) / q);
    store_edge<true, SHIFTS>(E_real + t, capacity, k, k, Image{0.f, 0.f, 0.f, 0.f, 0, 0, 0}, edge_index, edge_shift, edge_vec,
                             edge_diff);
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

// The periodic walk (gn_radius_{count,fill,verify}_pbc and their _images forms): one wave64 per target atom over the
// candidates (source j, image t) of its box.
//   Candidates.  The flattened index q = (j - j0) * n_img + t_flat, t_flat = (tx * ny + ty) * nz + tz (tx slowest); candidate
// shift s = -rint(f) + (t - R), f the fractional difference d @ inv_cell of the pair -- formed HERE and nowhere else -- and
// R = img_range[box] the host's per-axis bound (gn_radius_count_pbc_images in the header: every image inside the cutoff has
// |s_k + rint(f_k)| <= R_k).  Ascending q is: sources ascending, then shifts ascending lexicographically in (sx, sy, sz).
//   IMAGES = false is the minimum-image search: R = 0 at compile time, so n_img = 1, every division below folds away and
// the candidate of a pair is its rounded image, the one inside the cutoff when the cell is at least 2 * cutoff wide (the
// host sends no other: that image has all fractional coordinates in (-1/2, 1/2), for skewed cells too).  The multi-image
// search at R = 0 is therefore the minimum-image search bit for bit: it is the same code.
//   Placement.  The lanes take 64 consecutive candidates per trip; a ballot plus the popcount of the lower lanes gives each
// hit its slot in candidate order, and the wave-uniform running count carries the cap across trips: the first max_nbr hits
// in that order, deterministic, no atomics.  (jb, tb) = candidate of lane 0 as (source offset, image index): 32-bit
// throughout, no product of the box size and n_img is ever formed.
template <bool IMAGES, class Sink>
__global__ __launch_bounds__(256) void radius_wave_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch,
                                                          const int* __restrict__ mol_ptr, const float* __restrict__ cell,
                                                          const float* __restrict__ inv_cell,
                                                          const int* __restrict__ img_range, int N, int n_mol, float r2,
                                                          int max_nbr, Sink sink) {
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                // (wave-uniform)
    const int m = box_of(batch, i, n_mol);
    const int j0 = mol_ptr[m], nj = mol_ptr[m + 1] - j0;
    const float* c = cell + 9 * m;
    const float* ic = inv_cell + 9 * m;
    // (the host refuses R > GN_PBC_MAX_IMAGE_RANGE; clamped all the same: a bad array costs images, never a long loop)
    const int Rx = IMAGES ? min(max(img_range[3 * m], 0), GN_PBC_MAX_IMAGE_RANGE) : 0;
    const int Ry = IMAGES ? min(max(img_range[3 * m + 1], 0), GN_PBC_MAX_IMAGE_RANGE) : 0;
    const int Rz = IMAGES ? min(max(img_range[3 * m + 2], 0), GN_PBC_MAX_IMAGE_RANGE) : 0;
    const int ny = 2 * Ry + 1, nz = 2 * Rz + 1, nyz = ny * nz, n_img = (2 * Rx + 1) * nyz;      // <= 343
    const float pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
    sink.begin(i);
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
            const int fx = (int)rintf(fmaf(dz, ic[6], fmaf(dy, ic[3], dx * ic[0])));
            const int fy = (int)rintf(fmaf(dz, ic[7], fmaf(dy, ic[4], dx * ic[1])));
            const int fz = (int)rintf(fmaf(dz, ic[8], fmaf(dy, ic[5], dx * ic[2])));
            im = shifted(dx, dy, dz, tx - Rx - fx, ty - Ry - fy, tz - Rz - fz, c);
            hit = im.d2 < r2;                          // (the self-loop: 0 < r2)
        }
        const unsigned long long mask = __ballot(hit);
        const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && slot < max_nbr) sink.hit(i, j, slot, im);
        cnt += __popcll(mask);
        tb += 64;                                      // the next 64 candidates
        jb += tb / n_img;
        tb %= n_img;
    }
    const bool any = __ballot(sink.flag()) != 0ull;
    if (lane == 0) sink.finish(i, cnt < max_nbr ? cnt : max_nbr, any);
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
    store_edge<false, false>(e, E, j, i, im, nullptr, nullptr, edge_vec, edge_diff);     // (an atom's own image, shift != 0, is a real edge)
}

// ================================================================================ which molecules hold a changed row?
// gn_radius_verify*: the verify sink above leaves one flag per target (same thread mapping as the searches).
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

/* ---- a neighbour list rebuilt inside a recorded step: kernel launches only, no memset, no copy, no host read ----------- */
extern "C" int gn_degree_scan(const int* deg, int N, int64_t* rowptr64, int* n_edges, void* stream) {
    if (N < 0 || !rowptr64 || !n_edges || (N > 0 && !deg)) return GN_ERR_BAD_ARG;
    hipLaunchKernelGGL(gn::degree_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, deg, N, rowptr64, n_edges);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_padded_tail(const int64_t* rowptr64, int N, int n_pad, int64_t capacity, int64_t* edge_index,
                              int* edge_shift, float* edge_vec, float* edge_diff, int* state, void* stream) {
    if (N < 0 || n_pad < 1 || capacity < (int64_t)N + n_pad || capacity > 0x7fffffff) return GN_ERR_BAD_ARG;
    if (!rowptr64 || !edge_index || !edge_vec || !edge_diff || !state) return GN_ERR_BAD_ARG;
    const dim3 grid((unsigned)((capacity - N + 255) / 256)), block(256);          // the longest tail: self-loops only
    if (edge_shift)
        hipLaunchKernelGGL(gn::padded_tail_kernel<true>, grid, block, 0, (hipStream_t)stream, rowptr64, N, n_pad, capacity,
                           edge_index, edge_shift, edge_vec, edge_diff, state);
    else
        hipLaunchKernelGGL(gn::padded_tail_kernel<false>, grid, block, 0, (hipStream_t)stream, rowptr64, N, n_pad, capacity,
                           edge_index, edge_shift, edge_vec, edge_diff, state);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_graph_refresh(const int64_t* edge_index, int E, int N, int* src, int* dst, int* rowptr, int* outdeg,
                                int* colptr, int* perm, int* tgt_by_src, int* work, void* stream) {
    if (E < 0 || N < 0 || !rowptr || !colptr || (N > 0 && !work)) return GN_ERR_BAD_ARG;
    if (E > 0 && (!edge_index || !src || !dst || !perm || !tgt_by_src || !work)) return GN_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    int* cnt = work;                                             // gn_build_csc's layout: [N] counts, then [E] bucket contents
    int* tmp = work + N;
    const int items = E > N + 1 ? E : N + 1;
    const dim3 edges((E + 255) / 256), block(256);
    hipLaunchKernelGGL(gn::refresh_split_kernel, dim3((items + 255) / 256), block, 0, st, edge_index, E, N, src, dst, rowptr,
                       cnt, outdeg);
    if (E > 0) {
        hipLaunchKernelGGL(gn::csc_count_kernel, edges, block, 0, st, src, E, cnt);
        if (outdeg) hipLaunchKernelGGL(gn::csc_count_kernel, edges, block, 0, st, src, E, outdeg);   // (gn_out_degree's count)
    }
    hipLaunchKernelGGL(gn::csc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, N, colptr, cnt);
    if (E > 0) {
        hipLaunchKernelGGL(gn::csc_scatter_kernel, edges, block, 0, st, src, E, cnt, tmp);
        hipLaunchKernelGGL(gn::csc_rank_kernel, dim3((N + 3) / 4), block, 0, st, colptr, tmp, dst, N, perm, tgt_by_src);
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

/* ---- periodic boundary conditions ---------------------------------------------------------------------------- */
extern "C" int gn_cell_prepare(const float* cell, int n_mol, float* inv_cell, float* volume, void* stream) {
    if (n_mol < 0 || (n_mol > 0 && (!cell || !inv_cell || !volume))) return GN_ERR_BAD_ARG;
    if (n_mol == 0) return GN_OK;
    hipLaunchKernelGGL(gn::cell_prepare_kernel, dim3((n_mol + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       cell, n_mol, inv_cell, volume);
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

/* ---- the radius searches: nine entry points = three searches x three sinks ------------------------------------------ */
// What an entry point says about its search.  The open entry points take no mol_ptr / n_mol for the search itself (the
// verify one passes both for the per-molecule counts) and have always taken their pointers on trust.
struct Search {
    const float* pos;
    const int64_t* batch;
    int N;
    float cutoff;
    int max_nbr;
    bool periodic = false, images = false;
    const int* mol_ptr = nullptr;
    int n_mol = 0;
    const float* cell = nullptr;
    const float* inv_cell = nullptr;
    const int* img_range = nullptr;
};
static Search periodic_search(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                              const float* inv_cell, const int* img_range, bool images, int N, int n_mol, float cutoff,
                              int max_nbr) {
    return Search{pos, batch, N, cutoff, max_nbr, true, images, mol_ptr, n_mol, cell, inv_cell, img_range};
}
static bool search_ok(const Search& s) {
    if (s.N < 0 || s.max_nbr <= 0) return false;
    if (!s.periodic) return true;
    if (s.n_mol < 0) return false;
    return s.N == 0 || (s.n_mol >= 1 && s.pos && s.batch && s.mol_ptr && s.cell && s.inv_cell && (!s.images || s.img_range));
}
// one launch helper per walk: each kernel template is launched from here and nowhere else
template <class Sink>
static int launch_thread_walk(const Search& s, const Sink& sink, void* stream) {
    hipLaunchKernelGGL((gn::radius_thread_kernel<Sink>), dim3((s.N + 127) / 128), dim3(128), 0, (hipStream_t)stream, s.pos, s.batch,
                       s.N, s.cutoff * s.cutoff, s.max_nbr, sink);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
template <class Sink>
static int launch_wave_walk(const Search& s, const Sink& sink, void* stream) {
    const dim3 grid((s.N + 3) / 4), block(256);
    const float r2 = s.cutoff * s.cutoff;
    if (s.images)
        hipLaunchKernelGGL((gn::radius_wave_kernel<true, Sink>), grid, block, 0, (hipStream_t)stream, s.pos, s.batch, s.mol_ptr,
                           s.cell, s.inv_cell, s.img_range, s.N, s.n_mol, r2, s.max_nbr, sink);
    else
        hipLaunchKernelGGL((gn::radius_wave_kernel<false, Sink>), grid, block, 0, (hipStream_t)stream, s.pos, s.batch, s.mol_ptr,
                           s.cell, s.inv_cell, s.img_range, s.N, s.n_mol, r2, s.max_nbr, sink);
    GN_LAUNCH_CHECK();
    return GN_OK;
}
template <class Sink>
static int launch_walk(const Search& s, const Sink& sink, void* stream) {
    return s.periodic ? launch_wave_walk(s, sink, stream) : launch_thread_walk(s, sink, stream);
}

static int search_count(const Search& s, int* deg, void* stream) {
    if (!search_ok(s) || (s.periodic && s.N > 0 && !deg)) return GN_ERR_BAD_ARG;
    if (s.N == 0) return GN_OK;
    return launch_walk(s, gn::CountSink{deg}, stream);
}
template <bool SHIFTS>
static int search_fill(const Search& s, const gn::FillSink<SHIFTS>& f, void* stream) {
    if (!search_ok(s) || f.E < 0) return GN_ERR_BAD_ARG;
    if (s.periodic && ((s.N > 0 && !f.rowptr) || (f.E > 0 && (!f.edge_index || !f.edge_shift || !f.edge_vec || !f.edge_diff))))
        return GN_ERR_BAD_ARG;
    if (s.N == 0 || (s.periodic && f.E == 0)) return GN_OK;
    if constexpr (SHIFTS) return launch_wave_walk(s, f, stream);           // (a list with shifts is a periodic one)
    else return launch_thread_walk(s, f, stream);
}
// the walk leaves row_flag; then changed[m] = the flagged targets of molecule m
static int search_verify(const Search& s, const gn::VerifySink& v, int* changed, void* stream) {
    if (!search_ok(s) || s.n_mol < 0 || v.E < 0 || !v.state || (s.n_mol > 0 && (!changed || !s.mol_ptr))) return GN_ERR_BAD_ARG;
    if (s.N > 0 && !(s.n_mol >= 1 && s.pos && s.batch && v.rowptr && v.row_flag && (v.E == 0 || v.src))) return GN_ERR_BAD_ARG;
    if (s.periodic && v.E > 0 && !v.shift) return GN_ERR_BAD_ARG;
    if (s.N > 0) {
        const int rc = launch_walk(s, v, stream);
        if (rc != GN_OK) return rc;
    }
    if (s.n_mol > 0)
        hipLaunchKernelGGL(gn::rows_changed_kernel, dim3((s.n_mol + 3) / 4), dim3(256), 0, (hipStream_t)stream, v.row_flag,
                           s.mol_ptr, s.N, s.n_mol, changed);
    GN_LAUNCH_CHECK();
    return GN_OK;
}

extern "C" int gn_radius_count(const float* pos, const int64_t* batch, int N, float cutoff, int max_nbr,
                               int* deg, void* stream) {
    return search_count(Search{pos, batch, N, cutoff, max_nbr}, deg, stream);
}

extern "C" int gn_radius_fill(const float* pos, const int64_t* batch, int N, float cutoff, int max_nbr,
                              const int64_t* rowptr, int64_t E, int64_t* edge_index, float* edge_vec,
                              float* edge_diff, void* stream) {
    return search_fill(Search{pos, batch, N, cutoff, max_nbr}, gn::FillSink<false>{rowptr, E, edge_index, nullptr, edge_vec, edge_diff},
                       stream);
}

extern "C" int gn_radius_verify(const float* pos, const int64_t* batch, const int* mol_ptr, int N, int n_mol, float cutoff,
                                int max_nbr, const int* rowptr, const int* src, int E, int* row_flag, int* changed,
                                int* state, void* stream) {
    Search s{pos, batch, N, cutoff, max_nbr};
    s.mol_ptr = mol_ptr;
    s.n_mol = n_mol;
    return search_verify(s, gn::VerifySink{rowptr, src, nullptr, E, row_flag, state}, changed, stream);
}

extern "C" int gn_radius_count_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                   const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, int* deg,
                                   void* stream) {
    return search_count(periodic_search(pos, batch, mol_ptr, cell, inv_cell, nullptr, false, N, n_mol, cutoff, max_nbr), deg, stream);
}

extern "C" int gn_radius_fill_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                  const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr,
                                  const int64_t* rowptr, int64_t E, int64_t* edge_index, int* edge_shift,
                                  float* edge_vec, float* edge_diff, void* stream) {
    return search_fill(periodic_search(pos, batch, mol_ptr, cell, inv_cell, nullptr, false, N, n_mol, cutoff, max_nbr),
                       gn::FillSink<true>{rowptr, E, edge_index, edge_shift, edge_vec, edge_diff}, stream);
}

extern "C" int gn_radius_verify_pbc(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                    const float* inv_cell, int N, int n_mol, float cutoff, int max_nbr, const int* rowptr,
                                    const int* src, const int* shift, int E, int* row_flag, int* changed, int* state,
                                    void* stream) {
    return search_verify(periodic_search(pos, batch, mol_ptr, cell, inv_cell, nullptr, false, N, n_mol, cutoff, max_nbr),
                         gn::VerifySink{rowptr, src, shift, E, row_flag, state}, changed, stream);
}

extern "C" int gn_radius_count_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                          const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff,
                                          int max_nbr, int* deg, void* stream) {
    return search_count(periodic_search(pos, batch, mol_ptr, cell, inv_cell, img_range, true, N, n_mol, cutoff, max_nbr), deg, stream);
}

extern "C" int gn_radius_fill_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                         const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff,
                                         int max_nbr, const int64_t* rowptr, int64_t E, int64_t* edge_index,
                                         int* edge_shift, float* edge_vec, float* edge_diff, void* stream) {
    return search_fill(periodic_search(pos, batch, mol_ptr, cell, inv_cell, img_range, true, N, n_mol, cutoff, max_nbr),
                       gn::FillSink<true>{rowptr, E, edge_index, edge_shift, edge_vec, edge_diff}, stream);
}

extern "C" int gn_radius_verify_pbc_images(const float* pos, const int64_t* batch, const int* mol_ptr, const float* cell,
                                           const float* inv_cell, const int* img_range, int N, int n_mol, float cutoff,
                                           int max_nbr, const int* rowptr, const int* src, const int* shift, int E,
                                           int* row_flag, int* changed, int* state, void* stream) {
    return search_verify(periodic_search(pos, batch, mol_ptr, cell, inv_cell, img_range, true, N, n_mol, cutoff, max_nbr),
                         gn::VerifySink{rowptr, src, shift, E, row_flag, state}, changed, stream);
}
