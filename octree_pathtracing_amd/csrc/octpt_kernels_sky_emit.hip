// octpt_kernels_sky_emit.hip -- the emitter-sampling instances of the general shade and the block
// scene's drain under a sky (C42): octpt_kernels.hip's text compiled with OCTPT_EMIT_TU and OCTPT_SKY_TU, as a module of
// its own, so that the other emitter instances stay the code they are.  launch_wf_shade and launch_wf_drain take them
// through sky_emit_shade_kernel and sky_emit_drain_kernel (octpt_internal.h).
#define OCTPT_EMIT_TU 1
#define OCTPT_SKY_TU 1
#include "octpt_kernels.hip"
