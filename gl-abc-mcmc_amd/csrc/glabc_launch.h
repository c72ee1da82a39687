// glabc_launch.h -- host side of every launch: the grid size and the one place a launch's outcome becomes a status.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glabc.h"

namespace glabc {

// what glabc_last_hip_error() reports: defined in glabc_hip.hip, one per thread and per library (hidden visibility)
extern thread_local int g_last_hip_error;

// hipModuleLaunchKernel and the like hand their hipError_t in
inline int launch_status(hipError_t e)
{
    if (e == hipSuccess) return GLABC_OK;
    g_last_hip_error = (int)e;
    return GLABC_ERR_LAUNCH;
}

// after hipLaunchKernelGGL: reads and resets the runtime's error of this thread
inline int launch_status() { return launch_status(hipGetLastError()); }

// workgroups of `block` work-items that cover n of them
inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

}  // namespace glabc
