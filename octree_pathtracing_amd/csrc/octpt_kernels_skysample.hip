// octpt_kernels_skysample.hip -- the sky-sampling instances of the general shade and the drains:
// octpt_kernels.hip's text compiled with OCTPT_SKY_TU and OCTPT_SKYSAMPLE_TU, as a module of its own, so that every
// other instance, the sky's included, stays the code it is.  launch_wf_shade and launch_wf_drain take them through
// skysample_shade_kernel and skysample_drain_kernel (octpt_internal.h) when sky sampling is on, the sky is a MAP and
// its distribution's total is not 0.
#define OCTPT_SKY_TU 1
#define OCTPT_SKYSAMPLE_TU 1
#include "octpt_kernels.hip"
