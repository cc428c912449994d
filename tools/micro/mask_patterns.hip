// build + run: hipcc --offload-arch=gfx950 -O3 -o tools/micro/mask_patterns tools/micro/mask_patterns.hip && gpurun -- tools/micro/mask_patterns
// Microbenchmark: the moment kernel's two streams (float32 cube + uint8 mask), read-only, no arithmetic.
//   A<ZW,U>    : the kernel's pattern - a wave reads 1 KiB of data + 256 B of mask per plane, ZW waves on interleaved planes
//   B<ZW,U,K>  : a wave reads K consecutive KiB of data + K x 256 B of mask per plane (lane l owns columns 4l + 256k .. + 3)
//   C<ZW,U>    : ZW waves side by side on ONE plane (ZW KiB of data + ZW x 256 B of mask contiguous per block and plane)
//   P<ZW,U,F>  : pattern A with the mask read first and the 16 data bytes of a lane only loaded where its mask dword is not zero
//                (F 0: masks and data in the same iteration, 1: masks one batch of U planes ahead, 2: decided per group of 8 lanes =
//                per 128-byte line).  `mask_patterns pred TILE1024 TILE256 [reps]` runs A and the three P forms on a mask made of the
//                (nz, 16, 2048) uint8 tile of each file repeated along y (tools/needed_lines.py --tile writes the bench mask's tile)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#include <functional>
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ long xcd_group(long b, long nb) { const long q = nb >> 3, r = nb & 7, k = b & 7; return k * q + (k < r ? k : r) + (b >> 3); }

template <int ZW, int U, int K, bool SIDE>
__global__ __launch_bounds__(64 * ZW) void rd(const float* __restrict__ in, const uint8_t* __restrict__ mk, float* sink, long nz, long ncols,
                                             int remap) {
    long b = blockIdx.x;
    if (remap) b = xcd_group(b, gridDim.x);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    // SIDE: the ZW waves of a block sit side by side on one plane; otherwise they take interleaved planes
    const long col0 = SIDE ? ((b * ZW + w) * 64 * K + threadIdx.x) * 4 : (b * 64 * K + threadIdx.x) * 4;
    if (col0 >= ncols) return;
    const long zstep = SIDE ? 1 : ZW;
    f4 acc{};
    unsigned macc = 0;
    for (long z = SIDE ? 0 : w; z + (long)(U - 1) * zstep < nz; z += (long)U * zstep) {
        f4 v[U][K];
        unsigned m[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                v[u][k] = __builtin_nontemporal_load((const f4*)(in + (z + u * zstep) * ncols + col0 + k * 256));
                m[u][k] = __builtin_nontemporal_load((const unsigned*)(mk + (z + u * zstep) * ncols + col0 + k * 256));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < K; ++k) { acc += v[u][k]; macc += m[u][k]; }
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.f || macc == 0x12345u) sink[0] = 1;
}

// W<ZW,U>: the data as in A (16 bytes per lane and plane); the mask in 16-byte requests - lane l of a quad of lanes reads the quad's
// 16 mask bytes of plane (u & ~3) + (l & 3): U / 4 mask requests per lane for U planes instead of U (the moment kernel would then
// hand the four dwords around inside the quad)
template <int ZW, int U>
__global__ __launch_bounds__(64 * ZW) void rdw(const float* __restrict__ in, const uint8_t* __restrict__ mk, float* sink, long nz, long ncols, int remap) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    long b = blockIdx.x;
    if (remap) b = xcd_group(b, gridDim.x);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const long col0 = (b * 64 + threadIdx.x) * 4, colq = (b * 64 + (threadIdx.x & ~3)) * 4;
    if (col0 >= ncols) return;
    const long zstep = ZW;
    f4 acc{};
    u4 macc{};
    for (long z = w; z + (long)(U - 1) * zstep < nz; z += (long)U * zstep) {
        f4 v[U];
        u4 m[U / 4];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load((const f4*)(in + (z + u * zstep) * ncols + col0));
#pragma unroll
        for (int u = 0; u < U / 4; ++u) m[u] = __builtin_nontemporal_load((const u4*)(mk + (z + (4 * u + (threadIdx.x & 3)) * zstep) * ncols + colq));
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u];
#pragma unroll
        for (int u = 0; u < U / 4; ++u) macc += m[u];
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.f || (macc.x ^ macc.y ^ macc.z ^ macc.w) == 0x12345u) sink[0] = 1;
}

// P<ZW,U,FORM>: pattern A, mask first; a lane's data load is issued only where need(mask dword) holds, the others keep 0
template <int FORM>
__device__ __forceinline__ bool need(unsigned m) {
    if (FORM != 2) return m != 0;
    const unsigned long long b = __ballot(m != 0);             // FORM 2: the 8 lanes of one 128-byte line decide together
    return ((b >> (threadIdx.x & 56)) & 0xffull) != 0;
}
template <int ZW, int U, int FORM>
__global__ __launch_bounds__(64 * ZW) void rdp(const float* __restrict__ in, const uint8_t* __restrict__ mk, float* sink, long nz, long ncols, int remap) {
    long b = blockIdx.x;
    if (remap) b = xcd_group(b, gridDim.x);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const long col0 = (b * 64 + threadIdx.x) * 4;
    if (col0 >= ncols) return;
    const long step = (long)U * ZW;
    f4 acc{};
    unsigned macc = 0;
    long z = w;
    unsigned mn[U];
    if (FORM == 1 && z + (long)(U - 1) * ZW < nz) {
#pragma unroll
        for (int u = 0; u < U; ++u) mn[u] = __builtin_nontemporal_load((const unsigned*)(mk + (z + u * ZW) * ncols + col0));
    }
    for (; z + (long)(U - 1) * ZW < nz; z += step) {
        f4 v[U];
        unsigned m[U];
        if (FORM == 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) m[u] = mn[u];
            if (z + step + (long)(U - 1) * ZW < nz) {            // wave-uniform: the next batch's masks go out before this batch's data
#pragma unroll
                for (int u = 0; u < U; ++u) mn[u] = __builtin_nontemporal_load((const unsigned*)(mk + (z + step + u * ZW) * ncols + col0));
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) m[u] = __builtin_nontemporal_load((const unsigned*)(mk + (z + u * ZW) * ncols + col0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = f4{};
            if (need<FORM>(m[u])) v[u] = __builtin_nontemporal_load((const f4*)(in + (z + u * ZW) * ncols + col0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { acc += v[u]; macc += m[u]; }
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.f || macc == 0x12345u) sink[0] = 1;
}

static hipEvent_t e0, e1;
template <typename F>
static void timeit(const char* name, double bytes, F f) {
    float best = 1e9, ms = 0, sum = 0;
    for (int rep = 0; rep < 5; ++rep) {
        hipEventRecord(e0);
        f();
        hipEventRecord(e1); hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep) { sum += ms; if (ms < best) best = ms; }
    }
    printf("%-72s best %.3f ms  mean %.3f ms  %.2f TB/s\n", name, best, sum / 4, bytes / best / 1e9);
    fflush(stdout);
}
template <int ZW, int U, int K, bool SIDE>
static void run(const float* in, const uint8_t* mk, float* sink, long nz, long ncols) {
    for (int remap : {0, 1}) {
        char name[160];
        snprintf(name, 160, "%s ZW %d, U %d, %d KiB + %d B per wave and plane, xcd grouping %d", SIDE ? "side by side" : "interleaved ", ZW, U, K, 256 * K, remap);
        dim3 grid((unsigned)(ncols / 4 / 64 / K / (SIDE ? ZW : 1))), block(64, ZW);
        timeit(name, (double)nz * ncols * 5, [&] { rd<ZW, U, K, SIDE><<<grid, block>>>(in, mk, sink, nz, ncols, remap); });
    }
}
// ---- `pred`: A against the mask-first forms on the benchmark's own mask pattern
static std::vector<float> times(int reps, const std::function<void()>& f) {
    std::vector<float> t;
    for (int rep = 0; rep <= reps; ++rep) {
        float ms = 0;
        hipEventRecord(e0);
        f();
        hipEventRecord(e1); hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep) t.push_back(ms);                                 // the first launch warms up
    }
    std::sort(t.begin(), t.end());
    return t;
}
static int run_pred(int argc, char** argv) {
    const int reps = argc > 4 ? atoi(argv[4]) : 10;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (long shape = 0; shape < 2; ++shape) {
        const long nz = shape ? 256 : 1024, ncols = shape ? 4096L * 1024 : 1024 * 1024, tile = 16 * 2048;
        std::vector<uint8_t> t((size_t)nz * tile), host((size_t)nz * ncols);
        FILE* fh = fopen(argv[2 + shape], "rb");
        if (!fh || fread(t.data(), 1, t.size(), fh) != t.size()) { fprintf(stderr, "%s: not a (%ld, 16, 2048) uint8 tile\n", argv[2 + shape], nz); return 1; }
        fclose(fh);
        for (long z = 0; z < nz; ++z)
            for (long c = 0; c < ncols; c += tile) memcpy(&host[z * ncols + c], &t[z * tile], tile);
        // what a predicated form has to fetch: the share of the tile's aligned segments that hold an included voxel (the buffer repeats the tile)
        size_t valid = 0;
        for (uint8_t x : t) valid += x != 0;
        printf("# %ld planes of %ld columns, mask tile %s: valid %.4f; cube segments with an included voxel:", nz, ncols, argv[2 + shape], (double)valid / t.size());
        for (size_t vox : {4, 16, 32, 64, 256}) {                 // 16 B (one lane) .. 1 KiB (one wave) of the float32 cube
            size_t hit = 0;
            for (size_t i = 0; i < t.size(); i += vox) {
                bool any = false;
                for (size_t k = 0; k < vox; ++k) any |= t[i + k] != 0;
                hit += any;
            }
            printf("  %zu B %.4f", 4 * vox, (double)hit / (t.size() / vox));
        }
        printf("\n");
        float *in, *sink; uint8_t* mk;
        hipMalloc(&in, nz * ncols * 4); hipMalloc(&mk, nz * ncols); hipMalloc(&sink, 64);
        hipMemset(in, 0, nz * ncols * 4);
        hipMemcpy(mk, host.data(), host.size(), hipMemcpyHostToDevice);
        const dim3 grid((unsigned)(ncols / 4 / 64)), block(64, 4);
        struct V { const char* name; std::function<void()> f; };
        const V vs[] = {
            {"A  unpredicated        (rd<4,8,1>)", [&] { rd<4, 8, 1, false><<<grid, block>>>(in, mk, sink, nz, ncols, 0); }},
            {"P0 same iteration      (rdp<4,8,0>)", [&] { rdp<4, 8, 0><<<grid, block>>>(in, mk, sink, nz, ncols, 0); }},
            {"P1 masks a batch ahead (rdp<4,8,1>)", [&] { rdp<4, 8, 1><<<grid, block>>>(in, mk, sink, nz, ncols, 0); }},
            {"P2 per 8 lanes (128 B) (rdp<4,8,2>)", [&] { rdp<4, 8, 2><<<grid, block>>>(in, mk, sink, nz, ncols, 0); }},
        };
        for (int round = 0; round < 3; ++round)                   // three rounds, the forms alternating: A's own spread is rounds 0..2 of A
            for (const V& v : vs) {
                const std::vector<float> ts = times(reps, v.f);
                printf("round %d  %-38s min %.3f  median %.3f  max %.3f ms  (%d launches)  %.2f TB/s of the algorithmic 5 B/voxel\n", round, v.name,
                       ts.front(), ts[ts.size() / 2], ts.back(), (int)ts.size(), (double)nz * ncols * 5 / ts[ts.size() / 2] / 1e9);
                fflush(stdout);
            }
        hipFree(in); hipFree(mk); hipFree(sink);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "pred")) return run_pred(argc, argv);
    for (long shape = 0; shape < 2; ++shape) {
        const long nz = shape ? 256 : 1024, ncols = shape ? 4096L * 1024 : 1024 * 1024;
        printf("# %ld planes of %ld columns\n", nz, ncols);
        float *in, *sink; uint8_t* mk;
        hipMalloc(&in, nz * ncols * 4); hipMalloc(&mk, nz * ncols); hipMalloc(&sink, 64);
        hipMemset(in, 0, nz * ncols * 4); hipMemset(mk, 1, nz * ncols);
        hipEventCreate(&e0); hipEventCreate(&e1);
        run<4, 8, 1, false>(in, mk, sink, nz, ncols);
        for (int remap : {0, 1}) {
            char name[160];
            snprintf(name, 160, "16-byte mask requests ZW 4, U 8, 1 KiB + 4 x 1 KiB / 4 planes per wave, xcd grouping %d", remap);
            timeit(name, (double)nz * ncols * 5, [&] { rdw<4, 8><<<dim3((unsigned)(ncols / 4 / 64)), dim3(64, 4)>>>(in, mk, sink, nz, ncols, remap); });
            snprintf(name, 160, "16-byte mask requests ZW 8, U 8, xcd grouping %d", remap);
            timeit(name, (double)nz * ncols * 5, [&] { rdw<8, 8><<<dim3((unsigned)(ncols / 4 / 64)), dim3(64, 8)>>>(in, mk, sink, nz, ncols, remap); });
        }
        run<8, 8, 1, false>(in, mk, sink, nz, ncols);
        run<4, 4, 1, false>(in, mk, sink, nz, ncols);
        run<4, 4, 2, false>(in, mk, sink, nz, ncols);
        run<4, 2, 4, false>(in, mk, sink, nz, ncols);
        run<4, 4, 4, false>(in, mk, sink, nz, ncols);
        run<2, 4, 4, false>(in, mk, sink, nz, ncols);
        run<1, 4, 4, false>(in, mk, sink, nz, ncols);
        run<8, 2, 4, false>(in, mk, sink, nz, ncols);
        run<4, 8, 1, true>(in, mk, sink, nz, ncols);
        run<4, 4, 1, true>(in, mk, sink, nz, ncols);
        run<4, 4, 2, true>(in, mk, sink, nz, ncols);
        run<4, 2, 4, true>(in, mk, sink, nz, ncols);
        hipFree(in); hipFree(mk); hipFree(sink);
    }
    return 0;
}
