// gpu_check.hpp -- host helpers shared by the engine (nv_wavenet.hpp) and what is compiled once beside it: the error convention of
// the reference (HIP errors print "GPUassert: ..." and exit, nv_wavenet_util.cuh:34-40) and the classification of a pointer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#ifndef gpuErrChk
#define gpuErrChk(ans) { wnGpuAssert((ans), __FILE__, __LINE__); }
inline void wnGpuAssert(hipError_t code, const char* file, int line, bool abort = true) {
    if (code != hipSuccess) {
        fprintf(stderr, "GPUassert: %s %s %d\n", hipGetErrorString(code), file, line);
        if (abort) exit(code);
    }
}
#endif

namespace wn {

// the hipMemoryType of a pointer; -1 for one the runtime does not know
inline int pointer_type(const void* ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return attr.type;
}
inline bool is_device_ptr(const void* ptr) {
    const int type = pointer_type(ptr);
    return type == hipMemoryTypeDevice || type == hipMemoryTypeManaged;
}

}  // namespace wn
