// Host-side launch helpers shared by every launcher of libtnf_hip.so.
#pragma once
#include "dispatch.h"
#include "tnf_common.h"

namespace tnf {

// Launch a kernel that takes `smem` bytes of dynamic LDS; above 64 KB the kernel is first opted in to that much.
// check_launch stays with the caller: one per entry point.
template <class K, class... Args>
int launch_lds(const char* what, K kernel, dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args) {
    if (smem > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return fail(TNF_ELAUNCH, "%s: cannot reserve %zu B of LDS", what, smem);
    hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
    return TNF_OK;
}

// Arguments of a whole-flow launch (flow_fused2.hip, flow_fused3.hip): the offsets inside a parameter row come from the
// flow's layout.  log_q, Dr and stage_out start at zero; the launchers that use them set them.
inline Flow2Args flow2_args(const float* z, float* z_out, float* sum_log_det, float* log_prob, int64_t Mz, int64_t Mp,
                            int64_t N, int S, int U, const float* params, int64_t pstride, const float* bn_mean,
                            const float* bn_alpha, const FlowLayout& fl, const float* iv, unsigned* slow_count) {
    return Flow2Args{z, z_out, sum_log_det, log_prob, Mz, Mp, N, S, U, params, bn_mean, bn_alpha, pstride, fl.stage,
                     fl.p_up + fl.p_low, fl.p_up, iv, slow_count};
}

}  // namespace tnf
