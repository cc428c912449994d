// Stand-alone host check of spc_moments_list_plan_f32 / _count_f32 / _fill_f32 and spc_moments_list_f32 (csrc/spc_moments.hip,
// csrc/spc_moments_forms.hip) for a CPU build under sanitizers: the argument checks, the desc a plan gives and the size and offset arithmetic held
// against it - the long-axis and the empty-mask cases among them - everything up to the device switch.  Every call that
// would launch names device 2^20, which no machine has, so no kernel is ever launched and no pointer is dereferenced (the
// buffers are host memory); the kernels need a device and are covered by tests/test_gpu_moments_list.py.  From the
// repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_moments.hip -o moments.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -c spectral_cube_amd/csrc/spc_moments_forms.hip -o forms.o
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/host_check_moments_list.cpp -o main.o
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
    // addresses that are never read: 256-byte aligned host blocks
    std::vector<char> block(1 << 16);
    char* base = (char*)(((uintptr_t)block.data() + 255) & ~(uintptr_t)255);
    double dummy[8];
    spc_moment_outputs out; memset(&out, 0, sizeof out);
    out.d_m0 = out.d_m1 = out.d_m2 = dummy;
    spc_mask mask; memset(&mask, 0, sizeof mask);
    mask.flags = SPC_MASK_ARRAY; mask.d_array = (const uint8_t*)base;

    struct Case { int64_t nz, ny, nx; int zw, nsplit; int64_t zchunk, nblocks; const char* what; };
    const Case cases[] = {
        {4096, 2048, 2048, 4, 1, 4096, 16384, "the headline cube"},
        {1024, 1024, 1024, 8, 1, 1024, 4096, "1024^3"},
        {66000, 2, 8, 8, 16, 4125, 1, "more than 65535 planes"},
        {9, 4, 16, 1, 1, 9, 1, "fewer than 16 planes"},
        {37, 6, 40, 4, 1, 37, 1, "60 lane groups: dead lanes"},
        {300, 4, 64, 4, 4, 75, 1, "a z split"},
    };
    for (const Case& k : cases) {
        spc_cube_f32 c; memset(&c, 0, sizeof c);
        c.d_data = (const float*)base; c.nz = k.nz; c.ny = k.ny; c.nx = k.nx; c.row_stride = k.nx; c.plane_stride = k.ny * k.nx;
        const size_t wsn = spc_moments_workspace_bytes(k.nz, k.ny, k.nx);
        spc_moments_list_desc d; memset(&d, 0xff, sizeof d);
        char what[160];
        snprintf(what, sizeof what, "plan: %s", k.what);
        EXPECT(spc_moments_list_plan_f32(&c, &mask, &out, wsn ? base : nullptr, wsn, &d), SPC_OK, what);
        snprintf(what, sizeof what, "plan: %s: (zw %d, nsplit %d, zchunk %lld, nblocks %lld, nsub %lld)", k.what, d.zw, d.nsplit,
                 (long long)d.zchunk, (long long)d.nblocks, (long long)d.nsub);
        CHECK(d.zw == k.zw && d.nsplit == k.nsplit && d.zchunk == k.zchunk && d.nblocks == k.nblocks && d.nsub == (int64_t)k.zw * k.nsplit, what);
        CHECK((int64_t)d.nsplit * d.zchunk >= k.nz && (int64_t)(d.nsplit - 1) * d.zchunk < k.nz, "      the splits cover the planes, none is empty");
        const size_t bits = spc_mask_bits_bytes(k.nz, k.ny, k.nx);
        CHECK(bits == (size_t)d.nblocks * (size_t)k.nz * 32, "      the bits hold 32 bytes per block and plane");
        const size_t n = (size_t)(d.nblocks * d.nsub);
        // count: the checks, then the device switch
        spc_moments_list_desc d2; memset(&d2, 0, sizeof d2);
        uint32_t* len = (uint32_t*)(base + 1024);
        uint32_t* lines = (uint32_t*)(base + 2048);
        snprintf(what, sizeof what, "count: %s: valid, no device", k.what);
        EXPECT(spc_moments_list_count_f32(NO_DEVICE, nullptr, &c, &mask, &out, wsn ? base : nullptr, wsn, base, bits, len, lines, n, &d2), SPC_ERR_HIP, what);
        CHECK(memcmp(&d, &d2, sizeof d) == 0, "      count fills the desc of the plan");
        EXPECT(spc_moments_list_count_f32(NO_DEVICE, nullptr, &c, &mask, &out, wsn ? base : nullptr, wsn, base, bits, len, lines, n - 1, &d2), SPC_ERR_INVALID,
               "count: one sublist short");
        EXPECT(spc_moments_list_count_f32(NO_DEVICE, nullptr, &c, &mask, &out, wsn ? base : nullptr, wsn, base, bits - 1, len, lines, n, &d2), SPC_ERR_UNSUPPORTED,
               "count: bits one byte short: the launch would not read them");
        EXPECT(spc_moments_list_count_f32(NO_DEVICE, nullptr, &c, &mask, &out, wsn ? base : nullptr, wsn, nullptr, bits, len, lines, n, &d2), SPC_ERR_INVALID,
               "count: no bits");
        EXPECT(spc_moments_list_count_f32(NO_DEVICE, nullptr, &c, &mask, &out, wsn ? base : nullptr, wsn, base, bits, nullptr, lines, n, &d2), SPC_ERR_INVALID,
               "count: d_len NULL");
        // fill: sizes from a row count.  rows = 0 is the empty mask: no samples, no meta, still a valid call
        for (uint64_t rows : {(uint64_t)0, (uint64_t)1, (uint64_t)n * 3}) {
            spc_moments_list l; memset(&l, 0, sizeof l);
            l.desc = d; l.rows = rows; l.nsublists = n;
            l.d_off = (const uint64_t*)(base + 4096); l.d_len = len;
            l.d_samples = rows ? base + 8192 : nullptr; l.samples_bytes = (size_t)rows * 1024;
            l.d_meta = rows ? base + 8192 + 512 : nullptr; l.meta_bytes = (size_t)rows * 256;
            snprintf(what, sizeof what, "fill: %s, %llu rows: valid, no device", k.what, (unsigned long long)rows);
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &l), SPC_ERR_HIP, what);
            snprintf(what, sizeof what, "moments with the list: %s, %llu rows: valid, no device", k.what, (unsigned long long)rows);
            EXPECT(spc_moments_list_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, wsn ? base : nullptr, wsn, base, bits, &l), SPC_ERR_HIP, what);
            if (rows) {
                spc_moments_list s = l; s.samples_bytes -= 1;
                EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: samples one byte short");
                s = l; s.meta_bytes -= 1;
                EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: meta one byte short");
                s = l; s.d_samples = base + 8192 + 4;
                EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: samples not 16-byte aligned");
                s = l; s.d_meta = nullptr;
                EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: meta NULL with rows");
            }
            spc_moments_list s = l; s.nsublists = n - 1;
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: one sublist short");
            s = l; s.desc.nsub += 1;
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: nsub is not nsplit * zw");
            s = l; s.desc.zw = 2; s.desc.nsub = 2 * s.desc.nsplit;
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: zw 2");
            s = l; s.desc.nblocks += 1;
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: nblocks of another cube");
            s = l; s.desc.zchunk -= 1;
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: the splits do not cover the planes");
            s = l; s.desc.nsplit += 1; s.desc.nsub = (int64_t)s.desc.nsplit * s.desc.zw; s.nsublists = (size_t)(s.desc.nblocks * s.desc.nsub);
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, &s), SPC_ERR_INVALID, "fill: an empty split");
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits - 1, &l), SPC_ERR_INVALID, "fill: bits one byte short");
            EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, nullptr, bits, &l), SPC_ERR_INVALID, "fill: no bits");
        }
        EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &c, base, bits, nullptr), SPC_ERR_INVALID, "fill: list NULL");
        EXPECT(spc_moments_list_plan_f32(&c, &mask, &out, wsn ? base : nullptr, wsn, nullptr), SPC_ERR_INVALID, "plan: desc NULL");
    }
    // where there is no list
    spc_cube_f32 c; memset(&c, 0, sizeof c);
    c.d_data = (const float*)base; c.nz = 37; c.ny = 6; c.nx = 40; c.row_stride = 40; c.plane_stride = 240;
    spc_moments_list_desc d;
    spc_mask none; memset(&none, 0, sizeof none);
    EXPECT(spc_moments_list_plan_f32(&c, &none, &out, nullptr, 0, &d), SPC_ERR_UNSUPPORTED, "plan: no mask array");
    EXPECT(spc_moments_list_plan_f32(&c, nullptr, &out, nullptr, 0, &d), SPC_ERR_UNSUPPORTED, "plan: no mask");
    spc_cube_f32 odd = c; odd.nx = 42; odd.row_stride = 42; odd.plane_stride = 252;
    EXPECT(spc_moments_list_plan_f32(&odd, &mask, &out, nullptr, 0, &d), SPC_ERR_UNSUPPORTED, "plan: nx = 42: 8-byte lanes");
    spc_cube_f32 off = c; off.d_data = (const float*)(base + 4);
    EXPECT(spc_moments_list_plan_f32(&off, &mask, &out, nullptr, 0, &d), SPC_ERR_UNSUPPORTED, "plan: a cube that is not 16-byte aligned");
    spc_cube_f32 longz = c; longz.nz = 1LL << 28; longz.ny = 1; longz.nx = 4; longz.row_stride = 4; longz.plane_stride = 4;
    EXPECT(spc_moments_list_plan_f32(&longz, &mask, &out, base, spc_moments_workspace_bytes(longz.nz, 1, 4), &d), SPC_ERR_UNSUPPORTED, "plan: nz = 2^28");
    spc_moments_list l; memset(&l, 0, sizeof l);
    EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &longz, base, spc_mask_bits_bytes(longz.nz, 1, 4), &l), SPC_ERR_INVALID, "fill: nz = 2^28");
    longz.nz -= 1;
    EXPECT(spc_moments_list_plan_f32(&longz, &mask, &out, base, spc_moments_workspace_bytes(longz.nz, 1, 4), &d), SPC_OK, "plan: nz = 2^28 - 1");
    CHECK(d.nblocks == 1 && (int64_t)d.nsplit * d.zchunk >= longz.nz, "      its splits cover the planes");
    EXPECT(spc_moments_list_fill_f32(NO_DEVICE, nullptr, &odd, base, 1 << 20, &l), SPC_ERR_UNSUPPORTED, "fill: nx = 42");
    setenv("SPC_MOMENTS_MASK_FIRST", "0", 1);
    EXPECT(spc_moments_list_plan_f32(&c, &mask, &out, nullptr, 0, &d), SPC_ERR_UNSUPPORTED, "plan: SPC_MOMENTS_MASK_FIRST=0");
    unsetenv("SPC_MOMENTS_MASK_FIRST");
    setenv("SPC_MOMENTS_LIST", "0", 1);
    EXPECT(spc_moments_list_plan_f32(&c, &mask, &out, nullptr, 0, &d), SPC_ERR_UNSUPPORTED, "plan: SPC_MOMENTS_LIST=0");
    unsetenv("SPC_MOMENTS_LIST");
    // the checks of spc_moments_f32 come first, as they always did
    EXPECT(spc_moments_list_plan_f32(nullptr, &mask, &out, nullptr, 0, &d), SPC_ERR_INVALID, "plan: cube NULL");
    EXPECT(spc_moments_list_plan_f32(&c, &mask, nullptr, nullptr, 0, &d), SPC_ERR_INVALID, "plan: outputs NULL");
    EXPECT(spc_moments_list_f32(NO_DEVICE, nullptr, &c, &mask, nullptr, 1.0, 0.0, &out, nullptr, 0, base, 1 << 20, nullptr), SPC_ERR_INVALID,
           "moments with the list: d_cen NULL");
    EXPECT(spc_moments_list_f32(NO_DEVICE, nullptr, &c, &mask, dummy, 1.0, 0.0, &out, nullptr, 0, nullptr, 0, nullptr), SPC_ERR_HIP,
           "moments with the list: no bits, no list: spc_moments_f32, no device");
    printf(fails ? "%d host checks FAILED\n" : "all host checks passed\n", fails);
    return fails ? 1 : 0;
}
