// Stand-alone host check of spc_baseline_fit_f32 / _f64 and spc_baseline_apply_f32 / _f64 (csrc/spc_baseline.hip) for a CPU
// build under sanitizers: the argument checks, the list of buffers held against each other, the segment rule and the
// workspace carving - everything up to the device switch.  Every call names device 2^20, which no machine has, so no kernel
// is ever launched and no pointer is dereferenced (the buffers are host memory); the kernels need a device and are covered
// by tests/test_gpu_baseline.py.  From the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_baseline.hip -o baseline.o
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/host_check_baseline.cpp -o main.o
//   /opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined main.o baseline.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o host_check && ./host_check
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
#define EXPECT(rc, want, what) do { int r_ = (rc); if (r_ != (want)) { printf("FAIL %s: rc %d want %d (%s)\n", what, r_, want, g_err); ++fails; } else printf("ok   %-58s rc %d  %s\n", what, r_, r_ ? g_err : ""); g_err[0] = 0; } while (0)

int main() {
    // two shapes: one the rule leaves whole, one it cuts into three segments of 67, 67 and 66 list entries
    const int64_t shapes[2][3] = {{40, 4, 9}, {200, 2, 3}};
    for (int sh = 0; sh < 2; ++sh) {
        const int64_t nz = shapes[sh][0], ny = shapes[sh][1], nx = shapes[sh][2], n = nz * ny * nx, nsp = ny * nx;
        const int64_t nseg = spc_baseline_segments(nz, ny, nx, nz);
        printf("shape %lld x %lld x %lld: %lld segment(s)\n", (long long)nz, (long long)ny, (long long)nx, (long long)nseg);
        if (nseg != (sh ? 3 : 1)) { printf("FAIL segment rule\n"); ++fails; }
        std::vector<double> data(n, 1.0), out(n), basis(nz * 6, 1.0), coef(6 * nsp);
        std::vector<int32_t> npts(nsp), chan(nz);
        for (int64_t k = 0; k < nz; ++k) chan[k] = (int32_t)k;
        std::vector<unsigned char> marr(n, 1);
        for (int wide = 0; wide < 2; ++wide) {
            spc_cube_f32 c32; memset(&c32, 0, sizeof c32);
            c32.d_data = (const float*)data.data(); c32.nz = nz; c32.ny = ny; c32.nx = nx; c32.row_stride = nx; c32.plane_stride = ny * nx;
            spc_cube_f64 c64; memset(&c64, 0, sizeof c64);
            c64.d_data = data.data(); c64.nz = nz; c64.ny = ny; c64.nx = nx; c64.row_stride = nx; c64.plane_stride = ny * nx;
            spc_mask m32; memset(&m32, 0, sizeof m32);
            spc_mask_f64 m64; memset(&m64, 0, sizeof m64);
            auto fit = [&](bool with_mask, int order, const int32_t* ch, int64_t nfit, double* cf, int32_t* np, void* w, size_t wn) {
                m32.flags = m64.flags = with_mask ? (SPC_MASK_ARRAY | SPC_MASK_GT) : 0;
                m32.d_array = m64.d_array = with_mask ? marr.data() : nullptr;
                return wide ? spc_baseline_fit_f64(NO_DEVICE, nullptr, &c64, &m64, order, ch, nfit, basis.data(), cf, np, w, wn)
                            : spc_baseline_fit_f32(NO_DEVICE, nullptr, &c32, &m32, order, ch, nfit, basis.data(), cf, np, w, wn);
            };
            auto apply = [&](int order, int mode, void* o, int64_t ors, int64_t ops) {
                return wide ? spc_baseline_apply_f64(NO_DEVICE, nullptr, &c64, order, basis.data(), coef.data(), mode, (double*)o, ors, ops)
                            : spc_baseline_apply_f32(NO_DEVICE, nullptr, &c32, order, basis.data(), coef.data(), mode, (float*)o, ors, ops);
            };
            char what[112];
            const char* ty = wide ? "f64" : "f32";
            for (int order = 0; order <= SPC_BASELINE_MAX_ORDER; ++order) {
                const size_t need = spc_baseline_workspace_bytes(nz, ny, nx, nz, order);
                if ((need != 0) != (nseg > 1)) { printf("FAIL workspace size %zu with %lld segments\n", need, (long long)nseg); ++fails; }
                std::vector<char> ws(need + 512);
                void* w = (void*)(((uintptr_t)ws.data() + 255) & ~(uintptr_t)255);
                // enough of everything: all checks run, then the call stops for want of a device
                for (int form = 0; form < 8; ++form) {
                    snprintf(what, sizeof what, "%s fit order %d%s%s%s: valid, no device", ty, order, (form & 1) ? " + mask array" : "",
                             (form & 2) ? " + list" : "", (form & 4) ? ", no npts" : "");
                    EXPECT(fit(form & 1, order, (form & 2) ? chan.data() : nullptr, nz, coef.data(), (form & 4) ? nullptr : npts.data(), w, need),
                           SPC_ERR_HIP, what);
                }
                if (need) {
                    snprintf(what, sizeof what, "%s fit order %d: workspace one byte short", ty, order);
                    EXPECT(fit(true, order, chan.data(), nz, coef.data(), npts.data(), w, need - 1), SPC_ERR_INVALID, what);
                    snprintf(what, sizeof what, "%s fit order %d: workspace is d_coef", ty, order);
                    EXPECT(fit(true, order, chan.data(), nz, (double*)w, npts.data(), w, need), SPC_ERR_INVALID, what);
                }
                for (int mode = 0; mode < 2; ++mode) {
                    snprintf(what, sizeof what, "%s apply order %d mode %d: valid, no device", ty, order, mode);
                    EXPECT(apply(order, mode, out.data(), 0, 0), SPC_ERR_HIP, what);
                }
            }
            const size_t need = spc_baseline_workspace_bytes(nz, ny, nx, nz, 5);
            std::vector<char> ws(need + 512);
            void* w = (void*)(((uintptr_t)ws.data() + 255) & ~(uintptr_t)255);
            snprintf(what, sizeof what, "%s fit: order 6", ty);
            EXPECT(fit(false, 6, nullptr, nz, coef.data(), npts.data(), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s fit: order -1", ty);
            EXPECT(fit(false, -1, nullptr, nz, coef.data(), npts.data(), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s fit: no list and nfit != nz", ty);
            EXPECT(fit(false, 1, nullptr, nz - 1, coef.data(), npts.data(), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s fit: d_coef NULL", ty);
            EXPECT(fit(false, 1, nullptr, nz, nullptr, npts.data(), w, need), SPC_ERR_INVALID, what);
            // the last entries of the list are looked at too
            snprintf(what, sizeof what, "%s fit: d_coef is the cube", ty);
            EXPECT(fit(true, 1, chan.data(), nz, data.data(), npts.data(), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s fit: d_npts is the channel list", ty);
            EXPECT(fit(true, 1, chan.data(), nz, coef.data(), chan.data(), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s fit: d_npts is the mask array", ty);
            EXPECT(fit(true, 1, chan.data(), nz, coef.data(), (int32_t*)marr.data(), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s fit: d_npts inside d_coef", ty);
            EXPECT(fit(true, 1, chan.data(), nz, coef.data(), (int32_t*)(coef.data() + 1), w, need), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s apply: in place", ty);
            EXPECT(apply(1, 0, data.data(), 0, 0), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s apply: d_out is d_coef", ty);
            EXPECT(apply(1, 1, coef.data(), 0, 0), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s apply: mode 2", ty);
            EXPECT(apply(1, 2, out.data(), 0, 0), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s apply: out_row_stride below nx", ty);
            EXPECT(apply(1, 0, out.data(), nx - 1, 0), SPC_ERR_INVALID, what);
            snprintf(what, sizeof what, "%s apply: order 6", ty);
            EXPECT(apply(6, 0, out.data(), 0, 0), SPC_ERR_INVALID, what);
        }
    }
    printf(fails ? "%d host checks FAILED\n" : "all host checks passed\n", fails);
    return fails ? 1 : 0;
}
