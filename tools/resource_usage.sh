#!/bin/bash
# Registers, scratch, LDS and occupancy as the compiler reports them (kernel-resource-usage remarks) of
#   octpt_kernels.hip            the wavefront (resolve included), preview, guide-buffer, denoise, temporal, variance and
#                                tile-error kernels and the megakernel
#   octpt_kernels_lens.hip       the thin-lens instances of megakernel, seed and shade (the template arguments' last is Lb1)
#   octpt_kernels_sky.hip, octpt_kernels_sky_emit.hip   the sky instances of shade, the drain and the preview
#   octpt_kernels_skysample.hip  the sky-sampling instances of shade and the drain
#   octpt_build.hip              the section builder's count and emit kernels, the sky distribution's builder and sample
# tools/resource_usage.sh [-DFLAG ...].  CPU only (device-only compiles).
cd "$(dirname "$0")/.."
FLAGS=$(python3 -c "import __graft_entry__ as g; print(' '.join(f for f in g.HIPCC_FLAGS if f not in ('-shared', '-fPIC')))")
for SRC in octpt_kernels.hip octpt_kernels_lens.hip octpt_kernels_sky.hip octpt_kernels_sky_emit.hip octpt_kernels_skysample.hip octpt_build.hip; do
# the lens module compiles the whole text: only its own instances are listed
PAT='extend|shade|seed|drain|resolve|beam|preview|gbuffer|atrous|denoise|temporal|variance|tile_error|section_count|section_emit|render_kernel|sky_weight|sky_quantise|sky_row|sky_sample'
[ "$SRC" = octpt_kernels_lens.hip ] && PAT='render_kernel|wf_seed_kernel|wf_shade_kernel'
# the sky modules compile the whole text too: their own instances take a SkyScene
case "$SRC" in octpt_kernels_sky*) PAT='SkyScene';; esac
# ... and the sky-sampling module's a SkySampleScene
[ "$SRC" = octpt_kernels_skysample.hip ] && PAT='SkySampleScene'
/opt/rocm/bin/hipcc $FLAGS "$@" -c octree_pathtracing_amd/csrc/$SRC -o /tmp/octpt_res.o --offload-device-only \
    -Rpass-analysis=kernel-resource-usage 2>&1 | sed 's/ \[-Rpass-analysis=kernel-resource-usage\]//' | awk -v pat="$PAT" '
  /Function Name:/ {n = $NF}
  /remark:     VGPRs:/ {v = $NF}
  /remark:     TotalSGPRs: / {sg = $NF}
  /ScratchSize/ {sc = $NF}
  /Occupancy/ {occ = $NF}
  /LDS Size/ {if (n ~ pat) printf "%-70s VGPR %3s SGPR %3s scratch %3s LDS %5s occ %s\n", substr(n, 1, 70), v, sg, sc, $NF, occ}'
done
