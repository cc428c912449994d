// spc_select.hip - order statistics of float32 rays: median / percentile / mad_std per spaxel along the spectral axis
// (spc_percentile_axis0_f32; rays along y come in as a view with the first two axes exchanged) and along x
// (spc_percentile_axis2_f32).  Replaces da.nanmedian / np.nanpercentile / astropy stats.mad_std applied per ray by
// DaskSpectralCubeMixin.median / percentile / mad_std (spectral_cube/dask_spectral_cube.py:657-731), which sort or partition
// every ray on the host.
//
// No sort: the k-th smallest of a ray is found by descending the digits of an order-preserving integer key (sign-flipped
// IEEE bits), most significant first, for the two order statistics numpy's 'linear' percentile interpolates between; mad_std
// is the same selection on |x - centre| with the per-spaxel median as centre.  Three kernels:
//  * select_reg_kernel - what runs for rays of up to 4096 samples: a block reads its TS adjacent rays ONCE into register keys
//    and descends radix 16 over the registers (spc_select_impl.h).  select_reg_launch below is its table: block shape
//    (TS, KPL, block size) by ray length, 18 rows, each with or without a mask array and descriptor loads;
//  * select16_axis0_kernel - longer rays (up to 65535 samples) of 16-byte aligned cubes: radix 16 with per-spaxel histograms
//    in LDS, 8 streaming reads of the cube;
//  * select_axis0_kernel - any length and alignment: two key bits per pass in registers, 17 streaming reads.
// Whole-cube statistics are in spc_select_global.hip, sigma clipping in spc_sigma_clip.hip, float64 rays in spc_select_f64.hip.
#include "spc_select_impl.h"

namespace {

struct SelArgs {
    const float* cube;
    int64_t nz, ny, nx, row_stride, plane_stride;
    MaskDev mask;
    double q;                 // percentile in [0, 100]
    const float* center;      // NULL, or (ny, nx) map: select on |x - center|
    float scale;              // result multiplier (mad_std: 1.4826...)
    float* out;               // (ny, nx)
    // register-resident kernel only: step between adjacent spaxels of a row (1 for rays along z or y; the row stride of
    // the cube when the rays run along x) and whether consecutive LANES should walk along the ray (rays along x: the
    // samples of a ray are the contiguous ones)
    int64_t x_stride, m_x_stride;
    int along_ray;
    uint32_t key_min, key_span;            // sel_key_range of the mask's predicate terms (filled by the launcher)
    int xcd_group;                         // tiles of a row kept on one XCD (sel_tile_of_block): kXcdGroup
};

template <int VEC, bool ARR>
__global__ __launch_bounds__(256) void select_axis0_kernel(const SelArgs A) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t gpr = (A.nx + VEC - 1) / VEC;
    if (g >= A.ny * gpr) return;
    const int64_t y = g / gpr, x = (g - y * gpr) * VEC;
    const float* p = A.cube + y * A.row_stride + x;
    const uint8_t* pm = ARR ? A.mask.arr + y * A.mask.row_stride + x : nullptr;
    float cen[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) cen[c] = (A.center && x + c < A.nx) ? A.center[y * A.nx + x + c] : 0.f;
    const bool use_cen = A.center != nullptr;

    // one plane's samples of this lane: selection value and validity (0 / 1)
    struct Smp { float v[VEC]; int ok[VEC]; };
    auto load = [&](int64_t z) -> Smp {
        Smp r;
        float raw[VEC];
        unsigned mk[VEC];
        if (VEC == 4) {
            const f32x4s q4 = *reinterpret_cast<const f32x4s*>(p + z * A.plane_stride);
#pragma unroll
            for (int c = 0; c < VEC; ++c) raw[c] = q4[c];
            if (ARR) {
                const uint32_t m = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm + z * A.mask.plane_stride));
#pragma unroll
                for (int c = 0; c < VEC; ++c) mk[c] = (m >> (8 * c)) & 0xffu;
            }
        } else {
            raw[0] = p[z * A.plane_stride];
            if (ARR) mk[0] = pm[z * A.mask.plane_stride];
        }
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            bool ok = spc_pred_valid(A.mask, raw[c]);
            if (ARR) ok = ok && (mk[c] != 0);
            const float v = use_cen ? fabsf(raw[c] - cen[c]) : raw[c];
            r.v[c] = v;
            r.ok[c] = (ok && (v == v)) ? 1 : 0;
        }
        return r;
    };

    // pass 0: valid counts -> the two ranks of numpy's 'linear' percentile
    int n[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) n[c] = 0;
#pragma unroll 2
    for (int64_t z = 0; z < A.nz; ++z) {
        const Smp sm = load(z);
#pragma unroll
        for (int c = 0; c < VEC; ++c) n[c] += sm.ok[c];
    }
    int klo[VEC], khi[VEC];
    double frac[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        const double pos = A.q / 100.0 * (double)(n[c] > 0 ? n[c] - 1 : 0);
        const double fl = floor(pos);
        klo[c] = (int)fl;
        khi[c] = min((int)ceil(pos), max(n[c] - 1, 0));
        frac[c] = pos - fl;
    }
    uint32_t plo[VEC], phi[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) { plo[c] = 0u; phi[c] = 0u; }
    // two key bits per pass (16 passes): for each followed rank, count the prefix-matching samples
    // whose digit is 0, 1 or 2 (3 is the rest)
#pragma unroll 1
    for (int b = 30; b >= 0; b -= 2) {
        int clo[VEC][3], chi[VEC][3];
#pragma unroll
        for (int c = 0; c < VEC; ++c)
#pragma unroll
            for (int j = 0; j < 3; ++j) { clo[c][j] = 0; chi[c][j] = 0; }
#pragma unroll 2
        for (int64_t z = 0; z < A.nz; ++z) {
            const Smp sm = load(z);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                const uint32_t k = fkey(sm.v[c]);
                const uint32_t dg = (k >> b) & 3u;
                // (b + 2 == 32 in the first pass: no prefix yet; a 64-bit shift keeps that well defined)
                const int mlo = ((((uint64_t)(k ^ plo[c])) >> (b + 2)) == 0u ? 1 : 0) & sm.ok[c];
                const int mhi = ((((uint64_t)(k ^ phi[c])) >> (b + 2)) == 0u ? 1 : 0) & sm.ok[c];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int is = (dg == (uint32_t)j) ? 1 : 0;
                    clo[c][j] += mlo & is;
                    chi[c][j] += mhi & is;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            uint32_t d = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) if (klo[c] >= clo[c][j] && d == (uint32_t)j) { klo[c] -= clo[c][j]; d = j + 1; }
            plo[c] |= d << b;
            d = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) if (khi[c] >= chi[c][j] && d == (uint32_t)j) { khi[c] -= chi[c][j]; d = j + 1; }
            phi[c] |= d << b;
        }
    }
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        if (x + c >= A.nx) break;
        float res = NAN;
        if (n[c] > 0) {
            const double a = (double)funkey(plo[c]), bb = (double)funkey(phi[c]);
            // numpy's linear interpolation between the two order statistics (a + (b - a) * t; the
            // median of an even count is their mean)
            const double t = frac[c];
            res = (float)(((A.q == 50.0 && a == bb) ? a : (t == 0.5 ? 0.5 * (a + bb) : a + (bb - a) * t)) * (double)A.scale);   // (median of equal infinities)
        }
        A.out[y * A.nx + x + c] = res;
    }
}

// ---- four key bits per pass with per-spaxel histograms in LDS (8 reads of the cube instead of 17) ----
// Same descent, radix 16: a lane owns 4 adjacent spaxels and, for each of the two followed ranks, a
// 16-bin histogram per spaxel in LDS (two 16-bit counters per word: nz <= 65535; layout
// [word][rank][spaxel] so that a wave's updates fall into consecutive banks).  The bins are private to
// the lane, so the updates are fire-and-forget ds_add and no barrier is ever needed.  The first pass
// doubles as the valid count.  While both ranks still share their prefix (always, for an odd count)
// only one histogram is maintained.
constexpr int kSelSpaxels = 1024;                      // 256 lanes x 4

template <bool ARR>
__global__ __launch_bounds__(256) void select16_axis0_kernel(const SelArgs A) {
    __shared__ unsigned int hist[8][2][kSelSpaxels];     // 64 KB
    const int t = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * 256 + t;
    const int64_t gpr = A.nx / 4;
    const bool live = g < A.ny * gpr;
    const int64_t gg = live ? g : 0;
    const int64_t y = gg / gpr, x = (gg - y * gpr) * 4;
    const float* p = A.cube + y * A.row_stride + x;
    const uint8_t* pm = ARR ? A.mask.arr + y * A.mask.row_stride + x : nullptr;
    const bool use_cen = A.center != nullptr;
    float cen[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) cen[c] = use_cen ? A.center[y * A.nx + x + c] : 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w)
#pragma unroll
        for (int c = 0; c < 4; ++c) { hist[w][0][4 * t + c] = 0u; hist[w][1][4 * t + c] = 0u; }

    int n[4] = {0, 0, 0, 0}, klo[4] = {0, 0, 0, 0}, khi[4] = {0, 0, 0, 0};
    double frac[4] = {0, 0, 0, 0};
    uint32_t plo[4] = {0, 0, 0, 0}, phi[4] = {0, 0, 0, 0};
    bool same[4] = {true, true, true, true};
#pragma unroll 1
    for (int b = 28; b >= 0; b -= 4) {
#pragma unroll 2
        for (int64_t z = 0; z < A.nz; ++z) {
            const f32x4s q4 = *reinterpret_cast<const f32x4s*>(p + z * A.plane_stride);
            uint32_t m = 0x01010101u;
            if (ARR) m = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm + z * A.mask.plane_stride));
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float raw = q4[c];
                bool ok = spc_pred_valid(A.mask, raw) & (((m >> (8 * c)) & 0xffu) != 0);
                const float v = use_cen ? fabsf(raw - cen[c]) : raw;
                ok = ok && (v == v);
                const uint32_t k = fkey(v);
                const uint32_t dg = (k >> b) & 15u;
                const uint32_t inc = 1u << (16 * (dg & 1u));
                const bool mlo = ok && ((((uint64_t)(k ^ plo[c])) >> (b + 4)) == 0u);
                if (mlo) atomicAdd(&hist[dg >> 1][0][4 * t + c], inc);
                if (!same[c]) {
                    const bool mhi = ok && ((((uint64_t)(k ^ phi[c])) >> (b + 4)) == 0u);
                    if (mhi) atomicAdd(&hist[dg >> 1][1][4 * t + c], inc);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned cnt[2][16];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const unsigned a0 = hist[w][0][4 * t + c];
                const unsigned a1 = same[c] ? a0 : hist[w][1][4 * t + c];
                cnt[0][2 * w] = a0 & 0xffffu; cnt[0][2 * w + 1] = a0 >> 16;
                cnt[1][2 * w] = a1 & 0xffffu; cnt[1][2 * w + 1] = a1 >> 16;
                hist[w][0][4 * t + c] = 0u; hist[w][1][4 * t + c] = 0u;
            }
            if (b == 28) {                                   // first pass: every valid sample was counted
                int tot = 0;
#pragma unroll
                for (int d = 0; d < 16; ++d) tot += (int)cnt[0][d];
                n[c] = tot;
                const double pos = A.q / 100.0 * (double)(tot > 0 ? tot - 1 : 0);
                const double fl = floor(pos);
                klo[c] = (int)fl;
                khi[c] = min((int)ceil(pos), max(tot - 1, 0));
                frac[c] = pos - fl;
            }
            uint32_t dlo = 15, dhi = 15;
            bool flo = false, fhi = false;
#pragma unroll
            for (int d = 0; d < 15; ++d) {
                if (!flo) { if (klo[c] < (int)cnt[0][d]) { dlo = d; flo = true; } else klo[c] -= (int)cnt[0][d]; }
                if (!fhi) { if (khi[c] < (int)cnt[1][d]) { dhi = d; fhi = true; } else khi[c] -= (int)cnt[1][d]; }
            }
            plo[c] |= dlo << b;
            phi[c] |= dhi << b;
            same[c] = same[c] && (dlo == dhi);
        }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float res = NAN;
        if (n[c] > 0) {
            const double a = (double)funkey(plo[c]), bb = (double)funkey(phi[c]);
            const double tt = frac[c];
            res = (float)(((A.q == 50.0 && a == bb) ? a : (tt == 0.5 ? 0.5 * (a + bb) : a + (bb - a) * tt)) * (double)A.scale);
        }
        A.out[y * A.nx + x + c] = res;
    }
}

template <int TS, int KPL, bool ARR, bool DESC, int BT = 256>
// (blocks per CU the registers allow, as the compiler reports them - round-5 verdict: twelve instantiations asked for five and
//  got three; the bound now names what is reached: 128-ray tiles keep more state per lane)
__global__ __launch_bounds__(BT, BT == 256 ? (KPL == 128 ? 2 : (TS == 128 ? 3 : 5)) : (BT == 512 ? 4 : 1)) void select_reg_kernel(const SelArgs A) {
    __shared__ SelShared<TS> S;
    constexpr int kLanesPerRay = BT / TS;
    const int t = threadIdx.x;
    // ray of the tile, slice of the ray: adjacent lanes hold adjacent spaxels - or, for rays along x, adjacent samples
    const int r = A.along_ray ? t / kLanesPerRay : t % TS, j = A.along_ray ? t % kLanesPerRay : t / TS;
    const int64_t tiles_x = (A.nx + TS - 1) / TS;
    const int64_t tile = sel_tile_of_block(blockIdx.x, gridDim.x, A.xcd_group);
    const int64_t y = tile / tiles_x, x0 = (tile % tiles_x) * TS;
    const int nz = (int)A.nz;
    const bool col_in = x0 + r < A.nx;
    const bool use_cen = A.center != nullptr;
    const float cen = (use_cen && col_in) ? A.center[y * A.nx + x0 + r] : 0.f;
    sel_reset<TS, BT>(S);
    __syncthreads();
    // ---- the one read of the cube: keys into registers (excluded / NaN / beyond nz: the largest key)
    uint32_t key[KPL];
    const int rc = col_in ? r : (int)(A.nx - 1 - x0);
    const int64_t tile_off = y * A.row_stride + x0 * A.x_stride, m_tile_off = ARR ? y * A.mask.row_stride + x0 * A.m_x_stride : 0;
    const int mine = sel_load_keys<TS, KPL, ARR, DESC, BT>(A.cube, A.plane_stride, A.x_stride, tile_off, A.mask.arr, A.mask.plane_stride, A.m_x_stride,
                                                 m_tile_off, rc, j, nz, col_in, A.key_min, A.key_span, use_cen, cen, key);
    if (mine) atomicAdd(&S.nvalid[r], (uint32_t)mine);
    __syncthreads();
    const int n = (int)S.nvalid[r];
    uint32_t key_lo, key_hi;
    double frac;
    ray_select<TS, KPL, BT>(S, key, KeyIdentity{}, r, j, n, A.q, key_lo, key_hi, frac);
    if (j == 0 && col_in) A.out[y * A.nx + x0 + r] = n > 0 ? sel_value(key_lo, key_hi, frac, (double)A.scale, A.q == 50.0) : NAN;
}

// ---- the launch table of select_reg_kernel: block shape by ray length ----------------------------------------------
//   Base  (256 threads): 32 / 16 / 8 adjacent spaxels per block for rays of up to 512 / 1024 / 4096 samples, 16 .. 64 keys per
//          lane - 128 for the 2049 .. 4096 samples of 8 spaxels;
//   Short (256 threads, rays of up to 256 samples): few lanes per ray.  What a pass costs beyond counting the keys - the lane's
//          share of the histogram atomics, the barrier, every lane's walk over the 16 totals - is paid per LANE, and with 8
//          lanes on a ray of 100 samples it is most of the pass (0.8 - 1.1 ms per pass at 100 x 2048 x 4096 against 0.25 ms
//          for the same bytes in rays of 1024): 2 lanes per ray up to 128 samples (128 spaxels per block), 4 up to 256 (64);
//   Wide  (512 threads, rays of 257 .. 4096 samples): the lanes of a wave cover 64 / 32 / 16 / 8 ADJACENT spaxels for rays of
//          up to 512 / 1024 / 2048 / 4096 samples - a plane's samples of a block are one 256 / 128 / 64 / 32-byte run - and a
//          lane always holds 64 keys.  With 256 threads (16 spaxels, 64-byte runs at 1024 channels) the one read of the cube
//          ran at 2.1 TB/s and made up 2.0 of the 2.9 ms at 1024^3; 32 spaxels: 0.92 ms.
// 18 rows, each with and without a mask array and descriptor loads: the 72 instantiations of the kernel.  Four Base rows no ray
// length reaches - <16, 16>, <16, 32> (513 .. 1024 samples on 16 lanes need 33 .. 64 keys per lane) and <8, 16>, <8, 32> (more than
// 1024 samples on 32 lanes likewise): 16 instantiations kept because the set of kernels is.  Descriptor loads
// need the block's planes within 2 GiB (sel_desc_fits) and SPC_SELECT_DESC, whose default is the caller's: measured no gain
// for the Base table (3.64 against 3.25 ms with a uint8 mask, 2.61 against 2.65 ms without, 1024^3 - its time is in the digit
// passes).
enum class SelTable { Base, Short, Wide };
static void select_reg_launch(SelTable table, const SelArgs& A, int desc_default, hipStream_t st) {
    const int64_t nz = A.nz;
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const int bt = table == SelTable::Wide ? 512 : 256;
    const int ts = table == SelTable::Short ? (nz <= 128 ? 128 : 64)
                 : table == SelTable::Wide ? (nz <= 512 ? 64 : (nz <= 1024 ? 32 : (nz <= 2048 ? 16 : 8)))
                                           : sel_ts256(nz);
    const int kpl = sel_kpl(nz, bt / ts);
    const bool desc = sel_desc_fits(ts, std::max<int64_t>(A.plane_stride, arr ? A.mask.plane_stride : 0),
                                    std::max<int64_t>(A.x_stride, arr ? A.m_x_stride : 0), bt) &&
                      spc_switch("SPC_SELECT_DESC", desc_default) != 0;
    const dim3 grid((unsigned)(A.ny * ((A.nx + ts - 1) / ts)));
    auto row = [&](auto ts_c, auto kpl_c, auto bt_c) {
        constexpr int TS = decltype(ts_c)::value, KPL = decltype(kpl_c)::value, BT = decltype(bt_c)::value;
        sel_with_bool(arr, [&](auto arr_c) {
            sel_with_bool(desc, [&](auto desc_c) {
                hipLaunchKernelGGL((select_reg_kernel<TS, KPL, decltype(arr_c)::value, decltype(desc_c)::value, BT>), grid, dim3(BT), 0, st, A);
            });
        });
    };
    auto row256_by_kpl = [&](auto ts_c) {                       // 16, 32 or 64 keys per lane
        if (kpl == 16) row(ts_c, SelInt<16>{}, SelInt<256>{});
        else if (kpl == 32) row(ts_c, SelInt<32>{}, SelInt<256>{});
        else row(ts_c, SelInt<64>{}, SelInt<256>{});
    };
    if (table == SelTable::Wide) {
        if (ts == 64) row(SelInt<64>{}, SelInt<64>{}, SelInt<512>{});
        else if (ts == 32) row(SelInt<32>{}, SelInt<64>{}, SelInt<512>{});
        else if (ts == 16) row(SelInt<16>{}, SelInt<64>{}, SelInt<512>{});
        else row(SelInt<8>{}, SelInt<64>{}, SelInt<512>{});
    } else if (table == SelTable::Short) {
        if (ts == 64) row(SelInt<64>{}, SelInt<64>{}, SelInt<256>{});
        else row256_by_kpl(SelInt<128>{});
    } else {
        if (kpl == 128) row(SelInt<8>{}, SelInt<128>{}, SelInt<256>{});
        else if (ts == 32) row256_by_kpl(SelInt<32>{});
        else if (ts == 16) row256_by_kpl(SelInt<16>{});
        else row256_by_kpl(SelInt<8>{});
    }
}

// what both entries check and fill before they shape their view of the cube
static int select_args(SelArgs* A, const spc_cube_f32* cube, double q, const float* d_center, float scale, float* d_out) {
    const int rc = spc_check_cube_any_order(cube);
    if (rc) return rc;
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(q >= 0.0 && q <= 100.0, "Percentiles must be in the range [0, 100]");
    A->q = q; A->center = d_center; A->scale = scale; A->out = d_out;
    return SPC_OK;
}

}  // namespace

extern "C" int spc_percentile_axis0_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                        double q, const float* d_center, float scale, float* d_out) {
    SelArgs A{};
    int rc = select_args(&A, cube, q, d_center, scale, d_out);
    if (rc) return rc;
    rc = sel_set_cube<true>(&A, cube, mask);
    if (rc) return rc;
    SPC_DEVICE(device);
    A.x_stride = 1; A.m_x_stride = 1; A.along_ray = 0;
    A.xcd_group = kXcdGroup;
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const bool v4 = (cube->nx % 4 == 0) && (cube->row_stride % 4 == 0) && (cube->plane_stride % 4 == 0) &&
                    ((((uintptr_t)cube->d_data) & 15) == 0) &&
                    (!arr || ((A.mask.row_stride % 4 == 0) && (A.mask.plane_stride % 4 == 0) && ((((uintptr_t)A.mask.arr) & 3) == 0)));
    hipStream_t st = (hipStream_t)stream;
    // rays in registers (one read of the cube): up to 128 keys per lane, any strides (a y-ray view included)
    if (spc_switch("SPC_SELECT_REG", 1) != 0 && cube->nz <= 4096 && cube->ny * ((cube->nx + 7) / 8) < (1LL << 31)) {
        const int bt = spc_switch("SPC_SELECT_BT", 0);           // 256: the Base table also where Short or Wide would run
        // (rays of up to 256 samples never take the Wide table - 32 spaxels per block already, and the per-ray costs of the
        //  descent dominate: 2.26 against 2.46 ms at 256 x 2048 x 2048 - and neither do rays above 2048 samples with a mask ARRAY,
        //  whose 8 spaxels per block make 8-byte runs of mask bytes either way: 4.1 against 5.1 ms at 4096 x 512 x 512)
        const bool keep256 = cube->nz <= 256 || (cube->nz > 2048 && arr);
        const SelTable table = (cube->nz <= 256 && bt == 0 && spc_switch("SPC_SELECT_SHORT", 1) != 0) ? SelTable::Short
                             : (bt != 256 && !keep256)                                               ? SelTable::Wide
                                                                                                     : SelTable::Base;
        select_reg_launch(table, A, table == SelTable::Base ? 0 : 1, st);
        SPC_LAUNCH_CHECK();
        return SPC_OK;
    }
    if (v4 && cube->nz <= 65535 && spc_switch("SPC_SELECT_RADIX16", 1) != 0) {
        const int64_t n = cube->ny * (cube->nx / 4);
        dim3 grid((unsigned)((n + 255) / 256));
        if (arr) hipLaunchKernelGGL(select16_axis0_kernel<true>, grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL(select16_axis0_kernel<false>, grid, dim3(256), 0, st, A);
    } else if (v4) {
        const int64_t n = cube->ny * (cube->nx / 4);
        dim3 grid((unsigned)((n + 255) / 256));
        if (arr) hipLaunchKernelGGL((select_axis0_kernel<4, true>), grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL((select_axis0_kernel<4, false>), grid, dim3(256), 0, st, A);
    } else {
        const int64_t n = cube->ny * cube->nx;
        dim3 grid((unsigned)((n + 255) / 256));
        if (arr) hipLaunchKernelGGL((select_axis0_kernel<1, true>), grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL((select_axis0_kernel<1, false>), grid, dim3(256), 0, st, A);
    }
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

// The same statistic along x (median / percentile / mad_std with axis=2) without a transposed copy of the cube: the
// register-resident kernel on the view whose "spaxels" are the (z, y) pairs and whose rays are the rows - consecutive
// lanes take consecutive samples of a ray (contiguous in memory).  d_center / d_out: (nz, ny).  Rows of more than 4096
// samples: SPC_ERR_UNSUPPORTED (the caller transposes, spc_fill_masked_transpose_f32, and selects along y).
extern "C" int spc_percentile_axis2_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                        double q, const float* d_center, float scale, float* d_out) {
    SelArgs A{};
    int rc = select_args(&A, cube, q, d_center, scale, d_out);
    if (rc) return rc;
    if (cube->nx > 4096 || cube->nz * ((cube->ny + 7) / 8) >= (1LL << 31)) {
        spc_set_error("rows of %lld samples do not fit the registers of a block (4096 at most)", (long long)cube->nx);
        return SPC_ERR_UNSUPPORTED;
    }
    rc = sel_set_cube<true>(&A, cube, mask);
    if (rc) return rc;
    SPC_DEVICE(device);
    // the view: samples along x (step 1), rows = channels (step plane_stride), adjacent spaxels = adjacent rows y
    A.nz = cube->nx; A.ny = cube->nz; A.nx = cube->ny;
    A.plane_stride = 1; A.row_stride = cube->plane_stride; A.x_stride = cube->row_stride;
    A.m_x_stride = A.mask.row_stride;
    { const int64_t mrow = A.mask.plane_stride; A.mask.plane_stride = 1; A.mask.row_stride = mrow; }
    A.along_ray = 1;
    select_reg_launch(SelTable::Base, A, 0, (hipStream_t)stream);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}
