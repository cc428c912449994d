// Stand-alone host check of spc_label_measure_f32 / _f64 (csrc/spc_label_measure.hip) for a CPU build under sanitizers: the
// argument checks, the list of buffers that must not overlap and the workspace carving - everything up to the device
// switch.  Every call names device 2^20, which no machine has, so no kernel is ever launched and no pointer is dereferenced
// (the buffers are host memory); the kernels need a device and are covered by tests/test_gpu_measurements.py.  The case that
// matters most is the fullest one: all four groups, a mask array and an origin table together put 13 buffers on the list.
// From the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_label_measure.hip -o measure.o
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/host_check_label_measure.cpp -o main.o
//   /opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined main.o measure.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o host_check && ./host_check
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
#define EXPECT(rc, want, what) do { int r_ = (rc); if (r_ != (want)) { printf("FAIL %s: rc %d want %d (%s)\n", what, r_, want, g_err); ++fails; } else printf("ok   %-52s rc %d  %s\n", what, r_, r_ ? g_err : ""); g_err[0] = 0; } while (0)

int main() {
    const int64_t nz = 3, ny = 4, nx = 40, n = nz * ny * nx, nl = 7, nt = nl + 1;
    std::vector<double> data(n, 1.0), origin(4 * nt, 0.0), sums(2 * nt), first(4 * nt), second(6 * nt), vmin(nt), vmax(nt);
    std::vector<int32_t> labels(n, 1);
    std::vector<int64_t> count(nt), pmin(nt), pmax(nt);
    std::vector<unsigned char> marr(n, 1);
    spc_label_measure_outputs o;
    o.d_count = count.data(); o.d_sums = sums.data(); o.d_min = vmin.data(); o.d_max = vmax.data();
    o.d_min_pos = pmin.data(); o.d_max_pos = pmax.data(); o.d_first = first.data(); o.d_second = second.data();
    for (int wide = 0; wide < 2; ++wide) {
        spc_cube_f32 c32; memset(&c32, 0, sizeof c32);
        c32.d_data = (const float*)data.data(); c32.nz = nz; c32.ny = ny; c32.nx = nx; c32.row_stride = nx; c32.plane_stride = ny * nx;
        spc_cube_f64 c64; memset(&c64, 0, sizeof c64);
        c64.d_data = data.data(); c64.nz = nz; c64.ny = ny; c64.nx = nx; c64.row_stride = nx; c64.plane_stride = ny * nx;
        spc_mask m32; memset(&m32, 0, sizeof m32);
        spc_mask_f64 m64; memset(&m64, 0, sizeof m64);
        auto run = [&](bool with_mask, const double* org, uint32_t want, void* w, size_t wn) {
            m32.flags = m64.flags = with_mask ? (SPC_MASK_ARRAY | SPC_MASK_GT) : 0;
            m32.d_array = m64.d_array = with_mask ? marr.data() : nullptr;
            return wide ? spc_label_measure_f64(NO_DEVICE, nullptr, &c64, &m64, labels.data(), nl, org, want, &o, w, wn)
                        : spc_label_measure_f32(NO_DEVICE, nullptr, &c32, &m32, labels.data(), nl, org, want, &o, w, wn);
        };
        for (uint32_t want = 1; want < 16; ++want) {
            const size_t need = spc_label_measure_workspace_bytes(nl, want);
            std::vector<char> ws(need + 512);
            void* w = (void*)(((uintptr_t)ws.data() + 255) & ~(uintptr_t)255);
            char what[96];
            // enough of everything: all checks run, then the call stops for want of a device
            for (int form = 0; form < 4; ++form) {
                snprintf(what, sizeof what, "%s want %2u%s%s: valid, no device", wide ? "f64" : "f32", want, (form & 1) ? " + mask array" : "",
                         (form & 2) ? " + origin" : "");
                EXPECT(run(form & 1, (form & 2) ? origin.data() : nullptr, want, w, need), SPC_ERR_HIP, what);
            }
            snprintf(what, sizeof what, "%s want %2u: workspace one byte short", wide ? "f64" : "f32", want);
            EXPECT(run(true, origin.data(), want, w, need - 1), SPC_ERR_INVALID, what);
        }
        const size_t need = spc_label_measure_workspace_bytes(nl, 15);
        std::vector<char> ws(need + 512);
        void* w = (void*)(((uintptr_t)ws.data() + 255) & ~(uintptr_t)255);
        // the last entries of the fullest list are looked at too: the origins against a table, the mask array against one
        o.d_second = origin.data();
        EXPECT(run(true, origin.data(), 15, w, need), SPC_ERR_INVALID, "fullest list: d_second is d_origin");
        o.d_second = (double*)marr.data();
        EXPECT(run(true, origin.data(), 15, w, need), SPC_ERR_INVALID, "fullest list: d_second is the mask array");
        o.d_second = second.data();
    }
    printf(fails ? "%d host checks FAILED\n" : "all host checks passed\n", fails);
    return fails ? 1 : 0;
}
