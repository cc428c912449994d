// spc_sigma_clip.hip - sigma clipping of float32 rays along the spectral axis, the whole clip loop in one kernel:
// spc_sigma_clip_axis0_f32 (sigma_clip_spectrally, dask_spectral_cube.py:851-878; centre = median | mean, spread = std |
// mad_std).  A block loads its rays once into register keys (spc_select_impl.h), iterates on them - dense rays through the
// block's cached descents (clip_iterate), rays with few valid samples packed and sorted per wave (clip_packed_waves) - and
// writes the clipped rays once (the kernel: spc_sigma_clip_impl.h).  clip_launch below is the table of sigma_clip_reg_kernel: block
// shape by ray length, and for rays of 513 .. 1024 samples a probe of the mask decides between the 256- and the 512-thread shape.
// The kernels of spread = std are instantiated here, those of spread = mad_std in spc_sigma_clip_mad.hip.
#include "spc_sigma_clip_impl.h"

namespace {

template <bool ARR>
__global__ __launch_bounds__(256) void clip_probe_kernel(const ClipRegArgs A, int* d_max) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int64_t nsp = A.ny * A.nx;
    const int64_t sp = min(nsp - 1, (int64_t)blockIdx.x * (nsp / kProbeRays) + nsp / (2 * kProbeRays));
    const int64_t y = sp / A.nx, x = sp - y * A.nx;
    int c = 0;
    for (int64_t z = threadIdx.x; z < A.nz; z += 256) {
        const uint32_t k = fkey_bits(__float_as_uint(A.cube[z * A.plane_stride + y * A.row_stride + x]));
        bool ok = (k - A.key_min) < A.key_span;
        if (ARR) ok = ok && A.mask.arr[z * A.mask.plane_stride + y * A.mask.row_stride + x] != 0;
        c += ok ? 1 : 0;
    }
    if (c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(d_max, total);
}

// ---- the launch table of sigma_clip_reg_kernel: block shape by ray length -------------------------------------------
//   Base  (256 threads): clip_launch_base (spc_sigma_clip_impl.h), spread = std here, spread = mad_std in spc_sigma_clip_mad.hip:
//          2 x 40 instantiations;
//   Short (256 threads, rays of 65 .. 256 samples, spread = std): 2 lanes per ray up to 128 samples, 4 up to 256 - see the
//          selection's Short table; descriptor loads only (the caller checks sel_desc_fits): 4 instantiations;
//   Wide  (512 threads, rays of 513 .. 1024 samples, spread = std): 32 spaxels per block, descriptor loads only: 2.
enum class ClipTable { Base, Short, Wide };
static void clip_launch(ClipTable table, const ClipRegArgs& A, hipStream_t st) {
    if (table == ClipTable::Base) {
        if (A.spread_mad) spc_clip_launch_mad(&A, st);
        else clip_launch_base<false>(A, st);
        return;
    }
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const int ts = table == ClipTable::Wide ? 32 : (A.nz <= 128 ? 128 : 64);
    const dim3 grid((unsigned)(A.ny * ((A.nx + ts - 1) / ts)));
    auto row = [&](auto ts_c, auto bt_c) {                      // 64 keys per lane, spread = std, descriptor loads
        constexpr int TS = decltype(ts_c)::value, BT = decltype(bt_c)::value;
        sel_with_bool(arr, [&](auto arr_c) {
            hipLaunchKernelGGL((sigma_clip_reg_kernel<TS, 64, decltype(arr_c)::value, false, true, BT>), grid, dim3(BT), 0, st, A);
        });
    };
    if (table == ClipTable::Wide) row(SelInt<32>{}, SelInt<512>{});
    else if (ts == 128) row(SelInt<128>{}, SelInt<256>{});
    else row(SelInt<64>{}, SelInt<256>{});
}

}  // namespace

// astropy.stats.sigma_clip(axis=0, masked=False, cenfunc = median | mean, stdfunc = std | mad_std) with the rays resident in
// registers (sigma_clip_reg_kernel): one read and one write of the cube for all iterations.  d_out: (nz, ny, nx)
// C-contiguous float32, masked and clipped samples NaN.  Rays longer than 4096 channels: SPC_ERR_UNSUPPORTED (the
// caller iterates spc_percentile_axis0_f32 / spc_stats_axis_f32 / spc_clip_outside_f32 instead).
extern "C" int spc_sigma_clip_axis0_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                        double sigma_lower, double sigma_upper, int maxiters, int center_is_mean,
                                        int spread_is_mad, float* d_out, void* d_workspace, size_t workspace_bytes) {
    int rc = spc_check_cube_any_order(cube);
    if (rc) return rc;
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    if (cube->nz > 4096 || cube->ny * ((cube->nx + 7) / 8) >= (1LL << 31)) {
        spc_set_error("rays of %lld channels do not fit the registers of a block (4096 at most)", (long long)cube->nz);
        return SPC_ERR_UNSUPPORTED;
    }
    ClipRegArgs A{};
    rc = sel_set_cube<true>(&A, cube, mask);
    if (rc) return rc;
    SPC_DEVICE(device);
    A.out = d_out;
    A.lo_s = sigma_lower; A.hi_s = sigma_upper; A.maxiters = maxiters; A.cen_mean = center_is_mean ? 1 : 0;
    A.spread_mad = spread_is_mad ? 1 : 0;
    A.xcd_group = kXcdGroup;
    A.compact = spc_switch("SPC_SELECT_COMPACT", 2);   // 0: off, 1: packed rays through the block's loop, 2: every wave on its own
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const int64_t max_plane = std::max<int64_t>(cube->plane_stride, arr ? A.mask.plane_stride : 0);
    hipStream_t st = (hipStream_t)stream;
    // 256-thread blocks for the median forms: with 512 threads (wider runs per plane, see spc_select.hip's Wide table) the read +
    // write floor of the kernel drops from 4.2 to 2.3 ms at 1024^3, but an iteration with a descent costs 2.0 instead of 1.4 ms
    // (more barriers across 8 waves, the cached descents resume at the shallowest of 32 rays' levels, the loop ends with the
    // slowest of 32 rays): 10.4 against 8.6 ms for astropy's defaults.  Without a descent (centre = mean, spread = std) or
    // with a single iteration the wider blocks win: 2.3 - 3.4 against 4.2 ms.  SPC_SIGMA_BT=256 / 512 forces either.
    {
        const int force = spc_switch("SPC_SIGMA_BT", 0);
        const bool wide = force == 512 || (force != 256 && (A.cen_mean || A.maxiters == 1));
        const bool wide_ok = cube->nz > 512 && cube->nz <= 1024 && !A.spread_mad && sel_desc_fits(32, max_plane, 1, 512);
        // neither forced nor decided by the form: the mask decides (clip_probe_kernel), given a workspace word to decide in
        if (!wide && wide_ok && force == 0 && A.compact >= 2 && d_workspace != nullptr && workspace_bytes >= sizeof(int) &&
            cube->ny * cube->nx >= 4 * kProbeRays && spc_switch("SPC_SIGMA_PROBE", 1) != 0) {
            int* d_max = static_cast<int*>(d_workspace);
            SPC_HIP(hipMemsetAsync(d_max, 0, sizeof(int), st));
            if (arr) hipLaunchKernelGGL(clip_probe_kernel<true>, dim3(kProbeRays), dim3(256), 0, st, A, d_max);
            else hipLaunchKernelGGL(clip_probe_kernel<false>, dim3(kProbeRays), dim3(256), 0, st, A, d_max);
            A.probe = d_max;
        }
        if ((wide || A.probe != nullptr) && wide_ok) {
            clip_launch(ClipTable::Wide, A, st);
            SPC_LAUNCH_CHECK();
            if (A.probe == nullptr) return SPC_OK;
        }
    }
    const bool short_rays = cube->nz > 64 && cube->nz <= 256 && !A.spread_mad && spc_switch("SPC_SIGMA_SHORT", 1) != 0 &&
                            sel_desc_fits(cube->nz <= 128 ? 128 : 64, max_plane, 1, 256);
    clip_launch(short_rays ? ClipTable::Short : ClipTable::Base, A, st);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

size_t spc_ws_sigma_clip(void) { return 256; }
