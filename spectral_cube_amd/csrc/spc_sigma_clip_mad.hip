// spc_sigma_clip_mad.hip - the fused sigma-clip kernels with spread = mad_std (a second descent over |x - median| per iteration):
// 40 instantiations of sigma_clip_reg_kernel in a translation unit of their own, for build time.  Reached from
// spc_sigma_clip_axis0_f32 (spc_sigma_clip.hip) through spc_clip_launch_mad.
#include "spc_sigma_clip_impl.h"

void spc_clip_launch_mad(const void* args, hipStream_t st) {
    clip_launch_base<true>(*static_cast<const ClipRegArgs*>(args), st);
}
