// octpt_kernels_proj.hip -- the projected instances (parallel, fisheye and panoramic cameras) of the
// megakernel, the wavefront seed, the general shade, the preview and the guide-buffer kernel: octpt_kernels.hip's text
// compiled with kCamProj / kProj, as a module of its own, so that the pinhole and the lens instances stay the code they
// are.  The launchers stay in octpt_kernels.hip and take these instances through proj_render_kernel, proj_seed_kernel,
// proj_shade_kernel, proj_preview_kernel and proj_gbuffer_kernel (octpt_internal.h).
#define OCTPT_PROJ_TU 1
#include "octpt_kernels.hip"
