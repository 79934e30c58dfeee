// octpt_kernels_lens.hip -- the thin-lens instances of the megakernel, the wavefront seed and the
// general shade: octpt_kernels.hip's text compiled with kLens, as a module of its own, so that the instances
// without a lens stay the code they are (see lens_render_kernel there).  The launchers stay in octpt_kernels.hip
// and take these instances through lens_render_kernel, lens_seed_kernel and lens_shade_kernel (octpt_internal.h).
#define OCTPT_LENS_TU 1
#include "octpt_kernels.hip"
