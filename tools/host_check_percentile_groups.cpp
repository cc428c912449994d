// Stand-alone host check of spc_percentile_groups_f32 (csrc/spc_select_groups.hip) for a CPU build under sanitizers: the
// argument checks, the piece arithmetic and the workspace carving - everything up to the device switch.  Every call names
// device 2^20, which no machine has, so no kernel is ever launched and no pointer is dereferenced (the buffers are host
// memory); the pass loop itself needs a device and is covered by tests/test_gpu_plane_order_stats.py.  From the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_select_groups.hip -o groups.o
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/host_check_percentile_groups.cpp -o main.o
//   /opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined main.o groups.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o host_check && ./host_check
//
// (its own main: nothing is preloaded, nothing is loaded into an interpreter)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/spcube_hip.h"
static char g_err[512];
void spc_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
static int fails = 0;
static const int NO_DEVICE = 1 << 20;      // a device no machine has: the call stops at the device switch
#define EXPECT(rc, want, what) do { int r_ = (rc); if (r_ != (want)) { printf("FAIL %s: rc %d want %d (%s)\n", what, r_, want, g_err); ++fails; } else printf("ok   %-44s rc %d  %s\n", what, r_, r_ ? g_err : ""); g_err[0] = 0; } while (0)
int main() {
    std::vector<float> data(4 * 5 * 6, 1.f), out(64, 0.f), cen(64, 0.f);
    std::vector<unsigned char> marr(4 * 5 * 6, 1);
    spc_cube_f32 c; memset(&c, 0, sizeof c);
    c.d_data = data.data(); c.nz = 4; c.ny = 5; c.nx = 6; c.row_stride = 6; c.plane_stride = 30;
    size_t prev = 0;
    for (long long n : {0LL, 1LL, 2LL, 3LL, 700LL, 65536LL, 1LL << 20, 1LL << 32, -5LL}) {
        size_t b = spc_percentile_groups_workspace_bytes(n);
        printf("workspace_bytes(%lld) = %zu\n", n, b);
        if (n >= 0 && (b == 0 || b < prev)) { printf("FAIL size not monotone\n"); ++fails; }
        if (n >= 0) prev = b;
    }
    size_t need = spc_percentile_groups_workspace_bytes(5);
    std::vector<char> ws(need + 512);
    void* w = (void*)(((uintptr_t)ws.data() + 255) & ~(uintptr_t)255);
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, nullptr, nullptr, 0, 50.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "NULL cube");
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, nullptr, 2, 50.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "keep_axis 2");
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, nullptr, -1, 50.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "keep_axis -1");
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, nullptr, 0, 101.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "q 101");
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, nullptr, 0, 0.0 / 0.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "q NaN");
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, nullptr, 0, 50.0, nullptr, 1.f, nullptr, w, need), SPC_ERR_INVALID, "NULL d_out");
    spc_mask m; memset(&m, 0, sizeof m);
    m.flags = SPC_MASK_ARRAY;
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, &m, 0, 50.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "MASK_ARRAY without an array");
    m.flags = 64;
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, &m, 0, 50.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "unknown mask flag");
    m.flags = SPC_MASK_ARRAY | SPC_MASK_FINITE; m.d_array = marr.data(); m.row_stride = 6; m.plane_stride = 30;
    for (int keep = 0; keep < 2; ++keep) {
        size_t nd = spc_percentile_groups_workspace_bytes(keep ? c.ny : c.nz);
        EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, &m, keep, 50.0, cen.data(), 1.f, out.data(), nullptr, 0), SPC_ERR_INVALID, "no workspace");
        EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, &m, keep, 50.0, cen.data(), 1.f, out.data(), w, nd - 600), SPC_ERR_INVALID, "workspace 600 bytes short");
        // enough scratch: everything up to the device switch runs; without a device the call stops there
        EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &c, &m, keep, 50.0, cen.data(), 1.f, out.data(), w, nd), SPC_ERR_HIP, "valid call, no device");
    }
    // strided views and extreme extents through the segment arithmetic (no memory is touched before the device switch)
    spc_cube_f32 big = c;
    big.nz = 1LL << 20; big.ny = 1LL << 20; big.nx = 1LL << 20; big.row_stride = (1LL << 20) + 3; big.plane_stride = big.row_stride * big.ny;
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &big, nullptr, 0, 50.0, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "2^60 samples, scratch too small");
    big.nz = 3; big.ny = 1; big.nx = 70001; big.row_stride = 70001; big.plane_stride = 70001;
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &big, nullptr, 1, 37.5, nullptr, 1.f, out.data(), w, need), SPC_ERR_HIP, "one group of long rows, no device");
    big.row_stride = 10; 
    EXPECT(spc_percentile_groups_f32(NO_DEVICE, nullptr, &big, nullptr, 1, 37.5, nullptr, 1.f, out.data(), w, need), SPC_ERR_INVALID, "row_stride < nx");
    printf("%s\n", fails ? "FAILED" : "all host checks passed");
    return fails != 0;
}
