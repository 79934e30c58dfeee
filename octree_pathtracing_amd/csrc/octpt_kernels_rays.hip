// octpt_kernels_rays.hip -- the ray-list instances (the camera whose first rays the caller supplies) of
// the wavefront seed, the general shade, the preview and the guide-buffer kernel: octpt_kernels.hip's text compiled with
// kCamRays, as a module of its own, so that the pinhole, the lens and the projected instances stay the code they are.
// The launchers stay in octpt_kernels.hip and take these instances through rays_seed_kernel, rays_shade_kernel,
// rays_preview_kernel and rays_gbuffer_kernel (octpt_internal.h).
#define OCTPT_RAYS_TU 1
#include "octpt_kernels.hip"
