// Stand-alone host check of spc_moments_vlist_count_f32 / _fill_f32 and spc_moments_vlist_f32 (csrc/spc_moments.hip,
// csrc/spc_moments_forms.hip) for a CPU build under sanitizers: the argument and bounds checks of the three entries and the size arithmetic held against
// them - the long-axis and the empty cases among them - everything up to the device switch.  Every call that would launch
// names device 2^20, which no machine has, so no kernel is ever launched and no pointer is dereferenced (the buffers are
// host memory); the kernels need a device and are covered by tests/test_gpu_moments_vlist.py.  From the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_moments.hip -o moments.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_moments_forms.hip -o forms.o
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/host_check_moments_vlist.cpp -o main.o
//   /opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined main.o moments.o forms.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o host_check && ./host_check
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
#define EXPECT(rc, want, what) do { int r_ = (rc); if (r_ != (want)) { printf("FAIL %s: rc %d want %d (%s)\n", what, r_, want, g_err); ++fails; } else printf("ok   %-66s rc %d  %s\n", what, r_, r_ ? g_err : ""); g_err[0] = 0; } while (0)
#define CHECK(cond, what) do { if (!(cond)) { printf("FAIL %s\n", what); ++fails; } else printf("ok   %s\n", what); } while (0)

int main() {
    unsetenv("SPC_MOMENTS_ZW"); unsetenv("SPC_MOMENTS_NSPLIT"); unsetenv("SPC_MOMENTS_VEC"); unsetenv("SPC_MOMENTS_MASK_FIRST");
    unsetenv("SPC_MOMENTS_MASK_BITS"); unsetenv("SPC_MOMENTS_LIST"); unsetenv("SPC_MOMENTS_LIST_U");
    unsetenv("SPC_MOMENTS_VLIST"); unsetenv("SPC_MOMENTS_VLIST_U");
    CHECK(sizeof(spc_moments_list_desc) == 32 && sizeof(spc_moments_list) == 96 && sizeof(spc_moments_vlist) == 80,
          "struct sizes: desc 32, list 96 (unchanged), voxel list 80");
    // addresses that are never read: 256-byte aligned host blocks
    std::vector<char> block(1 << 16);
    char* base = (char*)(((uintptr_t)block.data() + 255) & ~(uintptr_t)255);
    double dummy[8];
    spc_moment_outputs out; memset(&out, 0, sizeof out);
    out.d_m0 = out.d_m1 = out.d_m2 = dummy;
    spc_mask mask; memset(&mask, 0, sizeof mask);
    mask.flags = SPC_MASK_ARRAY; mask.d_array = (const uint8_t*)base;

    struct Case { int64_t nz, ny, nx; const char* what; };
    const Case cases[] = {
        {4096, 2048, 2048, "the headline cube"},
        {1024, 1024, 1024, "1024^3"},
        {66000, 2, 8, "more than 65535 planes"},
        {9, 4, 16, "fewer than 16 planes"},
        {37, 6, 40, "60 lane groups: dead lanes"},
        {300, 4, 64, "a z split"},
    };
    for (const Case& k : cases) {
        spc_cube_f32 c; memset(&c, 0, sizeof c);
        c.d_data = (const float*)base; c.nz = k.nz; c.ny = k.ny; c.nx = k.nx; c.row_stride = k.nx; c.plane_stride = k.ny * k.nx;
        const size_t wsn = spc_moments_workspace_bytes(k.nz, k.ny, k.nx);
        void* ws = wsn ? base : nullptr;
        spc_moments_list_desc d; memset(&d, 0xff, sizeof d);
        char what[200];
        snprintf(what, sizeof what, "plan: %s", k.what);
        EXPECT(spc_moments_list_plan_f32(&c, &mask, &out, ws, wsn, &d), SPC_OK, what);
        const size_t bits = spc_mask_bits_bytes(k.nz, k.ny, k.nx);
        const size_t n = (size_t)(d.nblocks * d.nsub);
        uint32_t* len = (uint32_t*)(base + 1024);
        uint32_t* vlen = (uint32_t*)(base + 2048);
        // rows = 0 is the empty list: no samples, no meta, no entries, still valid calls
        for (uint64_t rows : {(uint64_t)0, (uint64_t)1, (uint64_t)n * 3}) {
            spc_moments_list l; memset(&l, 0, sizeof l);
            l.desc = d; l.rows = rows; l.nsublists = n;
            l.d_off = (const uint64_t*)(base + 4096); l.d_len = len;
            l.d_samples = rows ? base + 8192 : nullptr; l.samples_bytes = (size_t)rows * 1024;
            l.d_meta = rows ? base + 8192 + 512 : nullptr; l.meta_bytes = (size_t)rows * 256;
            // count
            snprintf(what, sizeof what, "count: %s, %llu rows: valid, no device", k.what, (unsigned long long)rows);
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &l, vlen, n), SPC_ERR_HIP, what);
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &l, vlen, n - 1), SPC_ERR_INVALID, "count: d_vlen one sublist short");
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &l, nullptr, n), SPC_ERR_INVALID, "count: d_vlen NULL");
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &l, (uint32_t*)(base + 2050), n), SPC_ERR_INVALID, "count: d_vlen not 4-byte aligned");
            spc_moments_list s = l; s.nsublists = n - 1;
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_INVALID, "count: the list one sublist short");
            s = l; s.d_off = nullptr;
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_INVALID, "count: the list's d_off NULL");
            s = l; s.desc.nsub += 1;
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n + (size_t)d.nblocks), SPC_ERR_INVALID, "count: nsub is not nsplit * zw");
            s = l; s.desc.zw = 2; s.desc.nsub = 2 * s.desc.nsplit;
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_INVALID, "count: zw 2");
            s = l; s.desc.nblocks = 0;
            EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_INVALID, "count: no blocks");
            if (rows) {
                s = l; s.meta_bytes -= 1;
                EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_INVALID, "count: meta one byte short");
                s = l; s.d_meta = nullptr;
                EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_INVALID, "count: meta NULL with rows");
                s = l; s.d_samples = nullptr; s.samples_bytes = 0;
                EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, &s, vlen, n), SPC_ERR_HIP, "count: reads only the metas: no samples, no device");
            }
            // fill and the launch: sizes from a row count of the voxel list
            for (uint64_t vrows : {(uint64_t)0, rows, rows * 4}) {
                spc_moments_vlist v; memset(&v, 0, sizeof v);
                v.desc = d; v.rows = vrows; v.nsublists = n;
                v.d_off = (const uint64_t*)(base + 6144); v.d_len = vlen;
                v.d_entries = base + 16384; v.entries_bytes = (size_t)(vrows ? vrows : 1) * 512;
                snprintf(what, sizeof what, "fill: %s, %llu -> %llu rows: valid, no device", k.what, (unsigned long long)rows, (unsigned long long)vrows);
                EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &v), SPC_ERR_HIP, what);
                snprintf(what, sizeof what, "moments with the voxel list: %s, %llu rows: valid, no device", k.what, (unsigned long long)vrows);
                EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, ws, wsn, base, bits, &l, &v), SPC_ERR_HIP, what);
                spc_moments_vlist t = v;
                if (vrows) {
                    t.entries_bytes = (size_t)vrows * 512 - 1;
                    EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &t), SPC_ERR_INVALID, "fill: entries one byte short");
                    t = v; t.d_entries = nullptr;
                    EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &t), SPC_ERR_INVALID, "fill: entries NULL with rows");
                }
                t = v; t.d_entries = base + 16384 + 4;
                EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &t), SPC_ERR_INVALID, "fill: entries not 8-byte aligned");
                t = v; t.nsublists = n - 1;
                EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &t), SPC_ERR_INVALID, "fill: one sublist short");
                t = v; t.d_len = nullptr;
                EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &t), SPC_ERR_INVALID, "fill: d_len NULL");
                t = v; t.desc.zchunk += 1;
                EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, &t), SPC_ERR_INVALID, "fill: the voxel list's desc is not the list's");
                if (rows) {
                    s = l; s.samples_bytes -= 1;
                    EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &s, &v), SPC_ERR_INVALID, "fill: the list's samples one byte short");
                    s = l; s.d_samples = base + 8192 + 4;
                    EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &s, &v), SPC_ERR_INVALID, "fill: the list's samples not 16-byte aligned");
                }
            }
            spc_moments_vlist v; memset(&v, 0, sizeof v);
            EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, &l, nullptr), SPC_ERR_INVALID, "fill: vlist NULL");
            EXPECT(spc_moments_vlist_fill_f32(NO_DEVICE, nullptr, nullptr, &v), SPC_ERR_INVALID, "fill: list NULL");
            // a voxel list the launch does not read is no error: the call is spc_moments_list_f32
            v.desc = d; v.desc.zw = d.zw == 4 ? 8 : 4; v.rows = 1;
            EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, ws, wsn, base, bits, &l, &v), SPC_ERR_HIP,
                   "moments: a voxel list of another plan, no arrays: the list form, no device");
            EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, ws, wsn, base, bits, &l, nullptr), SPC_ERR_HIP,
                   "moments: no voxel list: spc_moments_list_f32, no device");
        }
        EXPECT(spc_moments_vlist_count_f32(NO_DEVICE, nullptr, nullptr, vlen, n), SPC_ERR_INVALID, "count: list NULL");
    }
    // the checks of spc_moments_f32 come first, as they always did
    spc_cube_f32 c; memset(&c, 0, sizeof c);
    c.d_data = (const float*)base; c.nz = 37; c.ny = 6; c.nx = 40; c.row_stride = 40; c.plane_stride = 240;
    EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, &c, &mask, nullptr, 1.0, 0.0, &out, nullptr, 0, base, 1 << 20, nullptr, nullptr), SPC_ERR_INVALID,
           "moments with the voxel list: d_cen NULL");
    EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, nullptr, &mask, dummy, 1.0, 0.0, &out, nullptr, 0, base, 1 << 20, nullptr, nullptr), SPC_ERR_INVALID,
           "moments with the voxel list: cube NULL");
    EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, nullptr, 0, nullptr, 0, nullptr, nullptr), SPC_ERR_HIP,
           "moments with the voxel list: no bits, no lists: spc_moments_f32, no device");
    setenv("SPC_MOMENTS_VLIST", "0", 1);
    spc_moments_vlist junk; memset(&junk, 0xff, sizeof junk);
    EXPECT(spc_moments_vlist_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, nullptr, 0, nullptr, 0, nullptr, &junk), SPC_ERR_HIP,
           "moments: SPC_MOMENTS_VLIST=0 and no bits: the voxel list is not looked at");
    unsetenv("SPC_MOMENTS_VLIST");
    printf(fails ? "%d host checks FAILED\n" : "all host checks passed\n", fails);
    return fails ? 1 : 0;
}
