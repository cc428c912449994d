// spc_label.hip - connected components of a uint8 include array (scipy.ndimage.label on cube.get_mask_array(),
// spectral_cube.py:552, which users of the reference run on the host), the size and bounding box of every component
// (np.bincount, scipy.ndimage.find_objects) and the gather of a keep table through the labels.
//
// Rules (include/spcube_hip.h).  Two True voxels are neighbours when their offset is a True entry of the 3x3x3 structure;
// the structure is centrosymmetric and its centre is ignored, so the connectivity is 13 bits, one per pair of opposite
// offsets: bit t = entry t of the structure in C order, t < 13, the offsets that point BACK in raster order.  A component's
// label is 1 + the number of components whose first voxel (smallest linear index) comes before its own: scipy's numbering.
//
// Algorithm: union-find on the label array itself.  word[i] is the parent of voxel i, LB_BG for a False voxel, with the
// invariant 0 <= word[i] <= i for every True voxel at every moment of the merge.  A fixed sequence of six launches (five
// when the structure joins nothing and the merge is left out),
// whatever the shape of the components - nothing is swept until it settles and nothing is read back between them:
//   lb_init     word[i] = the first voxel of i's run of True voxels along x inside its wave's 64 voxels (i itself when
//               the x pair is not in the structure), from one ballot: runs along x are joined without an atomic.
//   lb_merge    every True voxel unites itself with each True backward neighbour the structure allows.  A union finds
//               both roots and hangs the larger under the smaller with atomicMin; the smallest index of a component
//               can only ever point at itself, so at the end each component is one tree rooted at its first voxel.
//   lb_flatten  word[i] = ~root for every voxel that is not a root (negative, so roots stay recognisable: word[r] == r),
//               and the number of roots of every block's contiguous chunk of the array.
//   lb_scan     exclusive prefix sum of the chunk counts (one block); the total is the number of labels.
//   lb_number   roots, in raster order: word[r] = 1 + the number of roots before r.
//   lb_relabel  word[i] = word[~word[i]] for the rest, 0 for the background.
//
// Termination.  No workgroup waits for another: there is no spin, ticket or look-back, only loops that make progress of
// their own.  A find walks word[j] < j strictly downward and ends at a root (at most i steps).  A union retries only when
// its atomicMin met a word another thread had lowered in between; every lowering decreases the sum of all words, which
// is a non-negative integer, so the retries of all threads together are finite.
// An atomicMin(word + a, b) that finds word[a] = old != a (a was no longer a root) may replace the link a -> old by
// a -> b; the same thread then unites old with b, which restores it.  The shortcut a find leaves behind (word[i] = the
// root it reached) replaces a link by one to an ancestor of its target.  So every value a word ever holds is a voxel of
// the same component with a smaller or equal index, and when the launch ends every pair the structure joins is in one tree.
//
// Visibility.  The 8 XCDs have private L2s and every CU a private L1.  In lb_merge and lb_flatten EVERY access to a word
// is an agent-scope relaxed atomic (a load that bypasses L1, an atomicMin, an atomic store): no plain load sees the
// array while other workgroups write it.  The other kernels read what an earlier launch wrote (kernel boundary) or words
// only their own thread writes: lb_relabel reads root words, which that launch does not change.
//
// Bytes per voxel and pass: init 1 B read + 4 B written, merge 4 B read + its neighbours' words (L2) + the atomics,
// flatten 4 + 4, number 4 B read, relabel 4 + 4: about 25 B against the 5 B (1 read, 4 written) the result needs.
#include "spc_common.h"

namespace {

constexpr int LB_BLOCK = 256;
constexpr int64_t LB_MAX_BLOCKS = 1 << 16;                            // of every grid; the most chunks lb_scan adds up
constexpr int32_t LB_BG = INT32_MIN;                                  // a False voxel until lb_relabel
constexpr int64_t LB_MAX_VOXELS = INT32_MAX;
constexpr int LB_SCAN_THREADS = 256;
constexpr int LB_OBJ_CHUNKS = 16;                                     // 64-voxel chunks a wave of lb_objects walks through
constexpr int64_t LB_OBJ_SPAN = (int64_t)LB_BLOCK * LB_OBJ_CHUNKS;    // voxels per block and round
constexpr int64_t LB_OBJ_MAX_BLOCKS = 2048;                            // of lb_objects: one add to the background's size each
constexpr int LB_KEEP_LDS = 32768;                                    // keep-table bytes lb_select stages in LDS
static_assert(LB_BLOCK % 64 == 0, "a wave's 64 voxels start at a multiple of 64");

__device__ __forceinline__ int32_t lb_ld(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_st(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t lb_min(int32_t* p, int32_t v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- init ---------------------------------------------------------------------------------------------------------------
struct LbInit {
    const uint8_t* src;                  // (nz, ny, nx) bytes, strides rs / ps
    int64_t rs, ps;
    int32_t* L;
    int64_t n;
    uint32_t ny, nx;
    int xlink;                           // the (0, 0, +-1) pair is in the structure
};

__global__ __launch_bounds__(LB_BLOCK) void lb_init_kernel(const LbInit A) {
    const int lane = threadIdx.x & 63;
    // bound: i0 grows by a positive stride up to n (uniform over the block: the ballots below see whole waves)
    for (int64_t i0 = (int64_t)blockIdx.x * LB_BLOCK; i0 < A.n; i0 += (int64_t)gridDim.x * LB_BLOCK) {
        const int64_t i = i0 + threadIdx.x;
        const bool valid = i < A.n;
        uint32_t x = 0;
        bool fg = false;
        if (valid) {
            const uint32_t row = (uint32_t)i / A.nx, z = row / A.ny, y = row - z * A.ny;
            x = (uint32_t)i - row * A.nx;
            fg = A.src[(int64_t)z * A.ps + (int64_t)y * A.rs + x] != 0;
        }
        const uint64_t F = __ballot(fg), R = __ballot(valid && x == 0);
        // a run starts after a False lane, at the head of a row and at lane 0: the highest such lane at or below this one
        const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
        const int start = 63 - __clzll((long long)((((~F) << 1) | R | 1ull) & upto));
        if (valid) A.L[i] = fg ? (int32_t)(i - (A.xlink ? lane - start : 0)) : LB_BG;
    }
}

// ---- merge --------------------------------------------------------------------------------------------------------------
// the root of i's tree (every load an agent-scope atomic); a walk of two links or more leaves a shortcut behind
__device__ __forceinline__ int32_t lb_find(int32_t* L, int32_t i) {
    int32_t j = i, v = lb_ld(L + j);
    int steps = 0;
    while (v != j) {                                                  // bound: word[j] < j here, j falls strictly and is >= 0
        j = v;
        v = lb_ld(L + j);
        ++steps;
    }
    if (steps >= 2) lb_min(L + i, j);
    return j;
}

// unite the trees of a and b; the root of the result as this thread saw it
__device__ __forceinline__ int32_t lb_union(int32_t* L, int32_t a, int32_t b) {
    for (;;) {          // bound: a pass is repeated only after an atomicMin met a word ANOTHER thread had lowered (file header)
        a = lb_find(L, a);
        b = lb_find(L, b);
        if (a == b) return a;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = lb_min(L + a, b);                         // b < a: word[a] <= a stays true
        if (old == a) return b;                                       // a was a root and now hangs under b
        a = old;                                                      // a had a parent already: that tree and b's, then
    }
}

struct LbMerge {
    int32_t* L;
    int64_t n;
    uint32_t nz, ny, nx;
    uint32_t bits;                       // bit t: entry t of the structure in C order, t < 13
};

__global__ __launch_bounds__(LB_BLOCK) void lb_merge_kernel(const LbMerge A) {
    const bool xlink = (A.bits >> 12) & 1u;
    // bound: i grows by a positive stride up to n
    for (int64_t i = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * LB_BLOCK) {
        if (lb_ld(A.L + i) < 0) continue;
        const uint32_t row = (uint32_t)i / A.nx, z = row / A.ny, y = row - z * A.ny, x = (uint32_t)i - row * A.nx;
        const bool prev = x > 0 && lb_ld(A.L + i - 1) >= 0;
        int32_t a = (int32_t)i;
        // lb_init joined the runs inside a wave's 64 voxels: only its first lane still has to look back along x
        if (xlink && prev && (i & 63) == 0) a = lb_union(A.L, a, (int32_t)(i - 1));
#pragma unroll
        for (int t = 0; t < 12; ++t) {                                // bound: the 12 backward offsets besides (0, 0, -1)
            if (!((A.bits >> t) & 1u)) continue;
            const int dz = t / 9 - 1, dy = (t / 3) % 3 - 1, dx = t % 3 - 1;
            const int64_t zz = (int64_t)z + dz, yy = (int64_t)y + dy, xx = (int64_t)x + dx;
            if (zz < 0 || yy < 0 || yy >= A.ny || xx < 0 || xx >= A.nx) continue;     // (dz <= 0: zz < nz)
            const int64_t j = (zz * A.ny + yy) * A.nx + xx;           // < i
            if (lb_ld(A.L + j) < 0) continue;
            // the pair one voxel back along x has the same offset: voxel i - 1 unites it (or passes it on in the same
            // way), and i ~ i - 1, j ~ j - 1 along x
            if (xlink && prev && xx >= 1 && lb_ld(A.L + j - 1) >= 0) continue;
            a = lb_union(A.L, a, (int32_t)j);
        }
    }
}

// ---- flatten, count, scan, number, relabel --------------------------------------------------------------------------------
// block b owns the voxels [b * per, (b + 1) * per), per = LB_BLOCK * rounds: the chunks follow each other in raster order
struct LbChunks {
    int32_t* L;
    int64_t n;
    int rounds;
    int32_t* counts;                     // one per block: roots in its chunk, then (lb_scan) roots before its chunk
    int64_t* total;
};

__device__ __forceinline__ int lb_block_sum(int v, int* lds) {       // lds: LB_BLOCK / 64 ints
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);          // bound: 6 halvings of the wave
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < LB_BLOCK / 64; ++w) s += lds[w];              // bound: the block's 4 waves
    return s;
}

__global__ __launch_bounds__(LB_BLOCK) void lb_flatten_kernel(const LbChunks A) {
    __shared__ int wsum[LB_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * LB_BLOCK * A.rounds;
    int roots = 0;
    for (int k = 0; k < A.rounds; ++k) {                              // bound: rounds
        const int64_t i = base + (int64_t)k * LB_BLOCK + threadIdx.x;
        if (i >= A.n) break;
        const int32_t v = lb_ld(A.L + i);
        if (v < 0) continue;
        if (v == (int32_t)i) { ++roots; continue; }
        int32_t j = v;
        for (;;) {                                                    // bound: j falls strictly until a root or a flattened word
            const int32_t w = lb_ld(A.L + j);
            if (w < 0) { j = ~w; break; }                             // j's own thread has written ~root already
            if (w == j) break;
            j = w;
        }
        lb_st(A.L + i, ~j);
    }
    const int s = lb_block_sum(roots, wsum);
    if (threadIdx.x == 0) A.counts[blockIdx.x] = s;
}

__global__ __launch_bounds__(LB_SCAN_THREADS) void lb_scan_kernel(int32_t* counts, int nblocks, int64_t* total) {
    __shared__ int sums[LB_SCAN_THREADS];
    const int per = (nblocks + LB_SCAN_THREADS - 1) / LB_SCAN_THREADS;
    const int lo = threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
    int s = 0;
    for (int b = lo; b < hi; ++b) s += counts[b];                     // bound: per <= LB_MAX_BLOCKS / LB_SCAN_THREADS
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < LB_SCAN_THREADS; o <<= 1) {                   // bound: log2(LB_SCAN_THREADS) steps
        const int add = threadIdx.x >= o ? sums[threadIdx.x - o] : 0;
        __syncthreads();
        sums[threadIdx.x] += add;
        __syncthreads();
    }
    int run = sums[threadIdx.x] - s;                                  // roots before this thread's chunks
    for (int b = lo; b < hi; ++b) {                                   // bound: per, as above
        const int c = counts[b];
        counts[b] = run;
        run += c;
    }
    if (threadIdx.x == LB_SCAN_THREADS - 1) *total = sums[LB_SCAN_THREADS - 1];
}

__global__ __launch_bounds__(LB_BLOCK) void lb_number_kernel(const LbChunks A) {
    __shared__ int wsum[LB_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * LB_BLOCK * A.rounds;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before = A.counts[blockIdx.x];
    for (int k = 0; k < A.rounds; ++k) {                              // bound: rounds (uniform: barriers inside)
        const int64_t i = base + (int64_t)k * LB_BLOCK + threadIdx.x;
        const bool root = i < A.n && A.L[i] == (int32_t)i;
        const uint64_t B = __ballot(root);
        __syncthreads();                                              // wsum of the round before has been read
        if (lane == 0) wsum[wave] = __popcll(B);
        __syncthreads();
        int off = 0, all = 0;
        for (int w = 0; w < LB_BLOCK / 64; ++w) {                     // bound: the block's 4 waves
            if (w < wave) off += wsum[w];
            all += wsum[w];
        }
        if (root) A.L[i] = before + off + __popcll(B & ((1ull << lane) - 1ull)) + 1;
        before += all;
    }
}

__global__ __launch_bounds__(LB_BLOCK) void lb_relabel_kernel(int32_t* L, int64_t n) {
    // bound: i grows by a positive stride up to n
    for (int64_t i = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LB_BLOCK) {
        const int32_t v = L[i];
        if (v == LB_BG) L[i] = 0;
        else if (v < 0) L[i] = L[~v];                                 // a root's word: lb_number wrote it, nobody writes it here
    }
}

// ---- sizes and bounding boxes -------------------------------------------------------------------------------------------
struct LbObjects {
    const int32_t* L;
    int64_t n, nlabels;
    uint32_t ny, nx;
    unsigned long long* sizes;           // nlabels + 1
    int32_t* bbox;                       // (nlabels + 1) x 6: zlo, zhi, ylo, yhi, xlo, xhi
    uint32_t* bad;
};

__global__ __launch_bounds__(LB_BLOCK) void lb_objects_init_kernel(const LbObjects A) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.bad = 0u;
    // bound: k grows by a positive stride up to nlabels
    for (int64_t k = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x; k <= A.nlabels; k += (int64_t)gridDim.x * LB_BLOCK) {
        A.sizes[k] = 0ull;
        int32_t* b = A.bbox + 6 * k;
        b[0] = b[2] = b[4] = INT32_MAX;
        b[1] = b[3] = b[5] = 0;
    }
}

// the bounds only ever move one way and start from the launch before: a stale read can only cost an atomic it did not need
__device__ __forceinline__ void lb_lower(int32_t* p, int32_t v) {
    if (v < *p) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_raise(int32_t* p, int32_t v) {
    if (v > *p) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_count(unsigned long long* sizes, int32_t k, long long c) {
    if (k >= 0 && c > 0) __hip_atomic_fetch_add(sizes + k, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wave walks through LB_OBJ_CHUNKS x 64 consecutive voxels a round.  Lanes run along x and mostly share a label: the
// voxels of one label that follow each other are one run, found with a shuffle and a ballot, and cost one atomic add - a
// run that goes on into the next 64 voxels, or into the wave's next round, is carried there, so a component that fills
// the array costs one add per wave.  The background is the one label every field has plenty of: it is counted apart,
// a popcount per 64 voxels, summed over the block in LDS, one add per block (atomics on ONE address run one after the
// other: the grid is kept small).  A run inside one row gives its label's box one candidate per bound, and the atomic
// is issued only where it would move it.
__global__ __launch_bounds__(LB_BLOCK) void lb_objects_kernel(const LbObjects A) {
    __shared__ unsigned long long bg_sum[LB_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad = false;
    long long bg = 0;                                                 // voxels of label 0 this wave met (uniform)
    int32_t open = -1;                                                // the run that reached the end of the chunk before
    long long open_n = 0;
    // bound: b0 grows by a positive stride up to n
    for (int64_t b0 = (int64_t)blockIdx.x * LB_OBJ_SPAN; b0 < A.n; b0 += (int64_t)gridDim.x * LB_OBJ_SPAN) {
        const int64_t w0 = b0 + (int64_t)wave * 64 * LB_OBJ_CHUNKS;
        for (int c = 0; c < LB_OBJ_CHUNKS; ++c) {                     // bound: LB_OBJ_CHUNKS (uniform over the wave)
            const int64_t c0 = w0 + (int64_t)c * 64;
            if (c0 >= A.n) break;
            const int64_t i = c0 + lane;
            int32_t k = -1;
            uint32_t row = ~0u, x = 0;
            if (i < A.n) {
                k = A.L[i];
                if (k < 0 || (int64_t)k > A.nlabels) { bad = true; k = -1; }
                row = (uint32_t)i / A.nx;
                x = (uint32_t)i - row * A.nx;
            }
            const int32_t kp = __shfl_up(k, 1);
            const uint32_t rowp = __shfl_up(row, 1);
            const bool head_k = lane == 0 || k != kp, head_r = head_k || row != rowp;
            const uint64_t HK = __ballot(head_k), HR = __ballot(head_r);
            bg += __popcll(__ballot(k == 0));
            if (head_r && k >= 0) {                                   // one run of a label inside a row
                const uint64_t above = lane == 63 ? 0ull : HR >> (lane + 1);
                const int len = above ? 1 + __builtin_ctzll(above) : 64 - lane;
                const uint32_t z = row / A.ny, y = row - z * A.ny;
                int32_t* b = A.bbox + 6 * (int64_t)k;
                lb_lower(b + 0, (int32_t)z); lb_raise(b + 1, (int32_t)z + 1);
                lb_lower(b + 2, (int32_t)y); lb_raise(b + 3, (int32_t)y + 1);
                lb_lower(b + 4, (int32_t)x); lb_raise(b + 5, (int32_t)x + len);
            }
            // the sizes of the labels above 0: lb_count passes over a run of -1, which a run of the background is here
            const int32_t ks = k == 0 ? -1 : k;
            const int last = 63 - __clzll((long long)HK);             // the head of the chunk's last run (bit 0 is set)
            const int first_n = (HK >> 1) ? 1 + __builtin_ctzll(HK >> 1) : 64;
            const int32_t kf = __shfl(ks, 0), kl = __shfl(ks, last);
            if (kf == open) open_n += first_n;
            else {
                if (lane == 0) lb_count(A.sizes, open, open_n);
                open = kf;
                open_n = first_n;
            }
            if (last != 0) {                                          // more runs than one: the first is complete,
                if (lane == 0) lb_count(A.sizes, open, open_n);
                if (head_k && lane != 0 && lane != last) {            // so are those in the middle, the last stays open
                    const uint64_t above = HK >> (lane + 1);          // (lane < last <= 63)
                    lb_count(A.sizes, ks, 1 + __builtin_ctzll(above));
                }
                open = kl;
                open_n = 64 - last;
            }
        }
    }
    if (lane == 0) {
        lb_count(A.sizes, open, open_n);
        bg_sum[wave] = (unsigned long long)bg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < LB_BLOCK / 64; ++w) s += bg_sum[w];       // bound: the block's 4 waves
        lb_count(A.sizes, 0, (long long)s);
    }
    if (__ballot(bad) != 0ull && lane == 0) __hip_atomic_fetch_or(A.bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- select ---------------------------------------------------------------------------------------------------------------
struct LbSelect {
    const int32_t* L;
    const uint8_t* keep;                 // nlabels + 1
    uint8_t* out;
    int64_t n, nlabels;
    int vec;                             // L is 16-byte and out 4-byte aligned
};

template <bool LDS>
__device__ __forceinline__ uint32_t lb_kept(const LbSelect& A, const uint8_t* tab, int32_t k) {
    if (k < 0 || (int64_t)k > A.nlabels) return 0u;                   // never past the table
    return (LDS ? tab[k] : A.keep[k]) != 0 ? 1u : 0u;
}

template <bool LDS>
__device__ __forceinline__ void lb_select_body(const LbSelect& A, const uint8_t* tab) {
    const int64_t groups = (A.n + 3) / 4;
    // bound: g grows by a positive stride up to groups
    for (int64_t g = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x; g < groups; g += (int64_t)gridDim.x * LB_BLOCK) {
        const int64_t i = 4 * g;
        if (A.vec && i + 4 <= A.n) {
            const int4 k = *reinterpret_cast<const int4*>(A.L + i);
            *reinterpret_cast<uint32_t*>(A.out + i) = lb_kept<LDS>(A, tab, k.x) | (lb_kept<LDS>(A, tab, k.y) << 8) |
                                                      (lb_kept<LDS>(A, tab, k.z) << 16) | (lb_kept<LDS>(A, tab, k.w) << 24);
        } else {
            // bound: the group's 4 voxels
            for (int64_t t = i; t < i + 4 && t < A.n; ++t) A.out[t] = (uint8_t)lb_kept<LDS>(A, tab, A.L[t]);
        }
    }
}

// LDS: the table fits LB_KEEP_LDS and is staged there; otherwise it is read through L2, by a kernel that holds no LDS
template <bool LDS>
__global__ __launch_bounds__(LB_BLOCK) void lb_select_kernel(const LbSelect A) {
    if constexpr (LDS) {
        __shared__ uint8_t tab[LB_KEEP_LDS];
        for (int t = threadIdx.x; t <= (int)A.nlabels; t += LB_BLOCK) tab[t] = A.keep[t];      // bound: nlabels < LB_KEEP_LDS
        __syncthreads();
        lb_select_body<true>(A, tab);
    } else {
        lb_select_body<false>(A, nullptr);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// the number of voxels, or -1 for a shape that is not positive; saturates at INT64_MAX / 4
int64_t lb_voxels(int64_t nz, int64_t ny, int64_t nx) {
    if (nz <= 0 || ny <= 0 || nx <= 0) return -1;
    const int64_t cap = INT64_MAX / 4;
    if (ny > cap / nz) return cap;
    const int64_t a = nz * ny;
    return nx > cap / a ? cap : a * nx;
}

unsigned lb_grid(int64_t n, int64_t per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b < LB_MAX_BLOCKS ? b : LB_MAX_BLOCKS));
}

bool lb_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

int lb_shape(int64_t nz, int64_t ny, int64_t nx, int64_t* n) {
    *n = lb_voxels(nz, ny, nx);
    SPC_REQUIRE(*n > 0, "label shape must be positive (got %lld,%lld,%lld)", (long long)nz, (long long)ny, (long long)nx);
    if (*n > LB_MAX_VOXELS) {
        spc_set_error("%lld x %lld x %lld voxels: linear indices are int32, at most 2^31 - 1 voxels are labelled", (long long)nz,
                      (long long)ny, (long long)nx);
        return SPC_ERR_UNSUPPORTED;
    }
    return SPC_OK;
}

size_t lb_counts_bytes(int64_t n) {
    const int64_t chunks = (n + LB_BLOCK - 1) / LB_BLOCK;
    return spc_ws_round(sizeof(int32_t) * (size_t)(chunks < LB_MAX_BLOCKS ? chunks : LB_MAX_BLOCKS));
}

}  // namespace

extern "C" {

size_t spc_label_workspace_bytes(int64_t nz, int64_t ny, int64_t nx) {
    const int64_t n = lb_voxels(nz, ny, nx);
    if (n <= 0) return 0;
    // the chunk counts, the total, the flag of spc_label_objects_i32; a slice may start up to 255 bytes into the workspace
    return lb_counts_bytes(n) + 2 * spc_ws_round(sizeof(int64_t)) + 256;
}

int spc_label_u8(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const uint8_t* d_in, int64_t in_row_stride,
                 int64_t in_plane_stride, const uint8_t* h_structure, int32_t* d_labels, void* d_workspace, size_t workspace_bytes,
                 int64_t* h_nlabels) {
    int64_t n = 0;
    const int rc = lb_shape(nz, ny, nx, &n);
    if (rc) return rc;
    SPC_REQUIRE(d_in != nullptr, "d_in is NULL");
    SPC_REQUIRE(d_labels != nullptr, "d_labels is NULL");
    SPC_REQUIRE(h_structure != nullptr, "h_structure is NULL");
    SPC_REQUIRE(h_nlabels != nullptr, "h_nlabels is NULL");
    int64_t rs = in_row_stride ? in_row_stride : nx, ps = in_plane_stride ? in_plane_stride : ny * rs;
    SPC_REQUIRE(rs >= nx && ps >= nx, "d_in: row / plane stride smaller than nx");
    SPC_REQUIRE(ps >= rs * (ny - 1) + nx || rs >= ps * (nz - 1) + nx, "d_in: overlapping rows and planes");
    const int64_t iext = (nz - 1) * ps + (ny - 1) * rs + nx;
    uint32_t bits = 0;
    for (int t = 0; t < 13; ++t) {
        SPC_REQUIRE((h_structure[t] != 0) == (h_structure[26 - t] != 0),
                    "the structure is not centrosymmetric (entry %d and entry %d differ)", t, 26 - t);
        if (h_structure[t]) bits |= 1u << t;
    }
    SPC_REQUIRE(!lb_overlap(d_labels, 4 * n, d_in, iext), "d_labels overlaps d_in");
    SPC_REQUIRE(d_workspace != nullptr && workspace_bytes >= spc_label_workspace_bytes(nz, ny, nx),
                "d_workspace too small: this call needs the %zu bytes spc_label_workspace_bytes returns", spc_label_workspace_bytes(nz, ny, nx));
    SpcWorkspace ws(d_workspace, workspace_bytes);
    const int rounds = (int)((n + LB_BLOCK * LB_MAX_BLOCKS - 1) / (LB_BLOCK * LB_MAX_BLOCKS));
    const int64_t per = (int64_t)LB_BLOCK * rounds;
    const int nchunks = (int)((n + per - 1) / per);                   // <= LB_MAX_BLOCKS
    SPC_WS_TAKE(d_counts, ws, int32_t, lb_counts_bytes(n) / sizeof(int32_t));
    SPC_WS_TAKE(d_total, ws, int64_t, 1);
    SPC_REQUIRE(!lb_overlap(d_workspace, (int64_t)ws.used, d_labels, 4 * n) && !lb_overlap(d_workspace, (int64_t)ws.used, d_in, iext),
                "d_workspace overlaps d_in or d_labels");

    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const unsigned gv = lb_grid(n, LB_BLOCK);

    LbInit I{};
    I.src = d_in; I.rs = rs; I.ps = ps; I.L = d_labels; I.n = n;
    I.ny = (uint32_t)ny; I.nx = (uint32_t)nx; I.xlink = (int)((bits >> 12) & 1u);
    hipLaunchKernelGGL(lb_init_kernel, dim3(gv), dim3(LB_BLOCK), 0, st, I);
    SPC_LAUNCH_CHECK();
    if (bits != 0u) {                                                 // no pair at all: every True voxel is its own root
        LbMerge M{};
        M.L = d_labels; M.n = n; M.nz = (uint32_t)nz; M.ny = (uint32_t)ny; M.nx = (uint32_t)nx; M.bits = bits;
        hipLaunchKernelGGL(lb_merge_kernel, dim3(gv), dim3(LB_BLOCK), 0, st, M);
        SPC_LAUNCH_CHECK();
    }
    LbChunks K{};
    K.L = d_labels; K.n = n; K.rounds = rounds; K.counts = d_counts; K.total = d_total;
    hipLaunchKernelGGL(lb_flatten_kernel, dim3((unsigned)nchunks), dim3(LB_BLOCK), 0, st, K);
    SPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(lb_scan_kernel, dim3(1), dim3(LB_SCAN_THREADS), 0, st, d_counts, nchunks, d_total);
    SPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(lb_number_kernel, dim3((unsigned)nchunks), dim3(LB_BLOCK), 0, st, K);
    SPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(lb_relabel_kernel, dim3(gv), dim3(LB_BLOCK), 0, st, d_labels, n);
    SPC_LAUNCH_CHECK();
    SPC_HIP(hipMemcpyAsync(h_nlabels, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SPC_HIP(hipStreamSynchronize(st));                                // the 8 bytes that reach the host
    return SPC_OK;
}

int spc_label_objects_i32(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const int32_t* d_labels, int64_t nlabels,
                          int64_t* d_sizes, int32_t* d_bbox, void* d_workspace, size_t workspace_bytes) {
    int64_t n = 0;
    const int rc = lb_shape(nz, ny, nx, &n);
    if (rc) return rc;
    SPC_REQUIRE(d_labels != nullptr, "d_labels is NULL");
    SPC_REQUIRE(d_sizes != nullptr, "d_sizes is NULL");
    SPC_REQUIRE(d_bbox != nullptr, "d_bbox is NULL");
    SPC_REQUIRE(nlabels >= 0 && nlabels <= LB_MAX_VOXELS, "nlabels must be 0 to 2^31 - 1 (got %lld)", (long long)nlabels);
    const int64_t nt = nlabels + 1;
    SPC_REQUIRE(!lb_overlap(d_sizes, 8 * nt, d_labels, 4 * n) && !lb_overlap(d_bbox, 24 * nt, d_labels, 4 * n) &&
                    !lb_overlap(d_sizes, 8 * nt, d_bbox, 24 * nt), "d_sizes, d_bbox and d_labels overlap");
    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(d_bad, ws, uint32_t, 1);
    SPC_REQUIRE(!lb_overlap(d_workspace, (int64_t)ws.used, d_labels, 4 * n) && !lb_overlap(d_workspace, (int64_t)ws.used, d_sizes, 8 * nt) &&
                    !lb_overlap(d_workspace, (int64_t)ws.used, d_bbox, 24 * nt), "d_workspace overlaps d_labels or a table");

    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    LbObjects O{};
    O.L = d_labels; O.n = n; O.nlabels = nlabels; O.ny = (uint32_t)ny; O.nx = (uint32_t)nx;
    O.sizes = reinterpret_cast<unsigned long long*>(d_sizes); O.bbox = d_bbox; O.bad = d_bad;
    hipLaunchKernelGGL(lb_objects_init_kernel, dim3(lb_grid(nt, LB_BLOCK)), dim3(LB_BLOCK), 0, st, O);
    SPC_LAUNCH_CHECK();
    const unsigned go = lb_grid(n, LB_OBJ_SPAN);
    hipLaunchKernelGGL(lb_objects_kernel, dim3(go < LB_OBJ_MAX_BLOCKS ? go : (unsigned)LB_OBJ_MAX_BLOCKS), dim3(LB_BLOCK), 0, st, O);
    SPC_LAUNCH_CHECK();
    uint32_t bad = 0;
    SPC_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    SPC_HIP(hipStreamSynchronize(st));
    SPC_REQUIRE(bad == 0u, "d_labels holds a label outside 0 ... %lld: those voxels were skipped", (long long)nlabels);
    return SPC_OK;
}

int spc_label_select_i32(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const int32_t* d_labels, int64_t nlabels,
                         const uint8_t* d_keep, uint8_t* d_out) {
    int64_t n = 0;
    const int rc = lb_shape(nz, ny, nx, &n);
    if (rc) return rc;
    SPC_REQUIRE(d_labels != nullptr, "d_labels is NULL");
    SPC_REQUIRE(d_keep != nullptr, "d_keep is NULL");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(nlabels >= 0 && nlabels <= LB_MAX_VOXELS, "nlabels must be 0 to 2^31 - 1 (got %lld)", (long long)nlabels);
    SPC_REQUIRE(!lb_overlap(d_out, n, d_labels, 4 * n), "d_out overlaps d_labels");
    SPC_REQUIRE(!lb_overlap(d_out, n, d_keep, nlabels + 1), "d_out overlaps d_keep");

    SPC_DEVICE(device);
    LbSelect S{};
    S.L = d_labels; S.keep = d_keep; S.out = d_out; S.n = n; S.nlabels = nlabels;
    S.vec = spc_aligned(d_labels, 16) && spc_aligned(d_out, 4);
    // (blocks that each stage the table: enough voxels per block to pay for it)
    const dim3 grid(lb_grid((n + 3) / 4, (int64_t)LB_BLOCK * 16));
    if (nlabels + 1 <= LB_KEEP_LDS) hipLaunchKernelGGL(lb_select_kernel<true>, grid, dim3(LB_BLOCK), 0, (hipStream_t)stream, S);
    else hipLaunchKernelGGL(lb_select_kernel<false>, grid, dim3(LB_BLOCK), 0, (hipStream_t)stream, S);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // extern "C"
