// octpt_kernels_emit.hip -- the emitter-sampling instances of the general shade and the drain:
// octpt_kernels.hip's text compiled with OCTPT_EMIT_TU, as a module of its own, so that the instances without emitter
// sampling stay the code they are.  The launchers stay in octpt_kernels.hip and take these instances through
// emit_shade_kernel and emit_drain_kernel (octpt_internal.h).
#define OCTPT_EMIT_TU 1
#include "octpt_kernels.hip"
