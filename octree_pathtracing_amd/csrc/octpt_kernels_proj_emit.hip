// octpt_kernels_proj_emit.hip -- the emitter-sampling instances of the general shade for a projected
// camera (C40): octpt_kernels.hip's text compiled with OCTPT_EMIT_TU and kCamProj, as a module of its own, so that
// octpt_kernels_emit.hip's instances stay the code they are.  launch_wf_shade takes them through
// proj_emit_shade_kernel (octpt_internal.h).
#define OCTPT_EMIT_TU 1
#define OCTPT_PROJ_TU 1
#include "octpt_kernels.hip"
