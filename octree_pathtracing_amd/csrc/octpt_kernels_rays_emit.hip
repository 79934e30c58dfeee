// octpt_kernels_rays_emit.hip -- the emitter-sampling instances of the general shade for the ray-list
// camera (C41): octpt_kernels.hip's text compiled with OCTPT_EMIT_TU and kCamRays, as a module of its own, so that the
// other emitter instances stay the code they are.  launch_wf_shade takes them through rays_emit_shade_kernel
// (octpt_internal.h).
#define OCTPT_EMIT_TU 1
#define OCTPT_RAYS_TU 1
#include "octpt_kernels.hip"
