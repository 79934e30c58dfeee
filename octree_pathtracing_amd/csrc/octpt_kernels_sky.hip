// octpt_kernels_sky.hip -- the sky instances of the general shade, the drain and the preview:
// octpt_kernels.hip's text compiled with OCTPT_SKY_TU, as a module of its own, so that the instances launched under the
// DEFAULT sky stay the code they are.  The launchers take them through sky_shade_kernel, sky_drain_kernel and
// sky_preview_kernel (octpt_internal.h) when the context's sky is not DEFAULT.
#define OCTPT_SKY_TU 1
#include "octpt_kernels.hip"
