// slots_sampler.hip -- the kernel that writes the changed columns' softmax scales, probability floors and cuts into the engine's table
// (slots_sampler.hpp).  Compiled once, both precisions.  At most 4 maxBatch entries of 8 bytes per step: one thread per entry.
#include "slots_sampler.hpp"

#include "gpu_check.hpp"

namespace wn {

TemperatureTable::~TemperatureTable() {
    if (softScale) gpuErrChk(hipFree(softScale));
}
void TemperatureTable::make() {
    std::vector<float> unit(4 * (size_t)columns, 0.0f);
    for (int b = 0; b < columns; b++) unit[b] = kSoftScaleUnit, unit[3 * (size_t)columns + b] = 1.0f;
    gpuErrChk(hipMalloc(&softScale, unit.size() * sizeof(float)));
    gpuErrChk(hipMemcpy(softScale, unit.data(), unit.size() * sizeof(float), hipMemcpyHostToDevice));
}
void TemperatureTable::set(int b, float t) {
    if (T.empty()) {
        if (t == 1.0f) return;
        T.assign(columns, 1.0f);
    }
    if (t != 1.0f && !softScale) make();
    nonUnit += (t != 1.0f) - (T[b] != 1.0f);
    T[b] = t;
}
void TemperatureTable::setP(int b, float p) {
    if (P.empty()) {
        if (p == 0.0f) return;
        P.assign(columns, 0.0f);
    }
    if (p != 0.0f && !softScale) make();
    nonZero += (p != 0.0f) - (P[b] != 0.0f);
    P[b] = p;
}
void TemperatureTable::setK(int b, int k) {
    if (K.empty()) {
        if (k == 0) return;
        K.assign(columns, 0);
    }
    if (k != 0 && !softScale) make();
    nonOffK += (k != 0) - (K[b] != 0);
    K[b] = k;
}
void TemperatureTable::setTopP(int b, float p) {
    if (Q.empty()) {
        if (p == 1.0f) return;
        Q.assign(columns, 1.0f);
    }
    if (p != 1.0f && !softScale) make();
    nonOffP += (p != 1.0f) - (Q[b] != 1.0f);
    Q[b] = p;
}
void TemperatureTable::reset(bool deviceBehind) {
    const bool rewrite = softScale && (nonUnit > 0 || nonZero > 0 || cutting() > 0 || deviceBehind);
    resetT();
    resetP();
    resetK();
    resetTopP();
    if (rewrite) {
        gpuErrChk(hipDeviceSynchronize());
        upload();
    }
}
void TemperatureTable::upload() {
    if (!softScale) return;
    std::vector<float> c(4 * (size_t)columns);
    for (int b = 0; b < columns; b++) {
        c[b] = temperature_scale(get(b));      // (T is empty when every value is 1, P when every floor is 0, K and Q when no cut)
        c[columns + b] = getP(b);
        c[2 * (size_t)columns + b] = top_k_entry(getK(b));
        c[3 * (size_t)columns + b] = getTopP(b);
    }
    gpuErrChk(hipMemcpy(softScale, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
}

__global__ __launch_bounds__(256) void slot_scale_kernel(float* __restrict__ table, int columns, const SlotScale* __restrict__ upd, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const SlotScale u = upd[i];
        if (u.column >= 0 && u.column < columns) table[u.column] = u.scale;
    }
}

bool slots_set_scales(hipStream_t stream, float* table, int columns, const SlotScale* upd, int n) {
    if (n <= 0) return true;
    if (table == NULL || upd == NULL || columns <= 0) return false;
    int grid = (n + 255) / 256;
    if (grid > 64) grid = 64;
    hipLaunchKernelGGL(slot_scale_kernel, dim3(grid), dim3(256), 0, stream, table, columns, upd, n);
    return hipGetLastError() == hipSuccess;
}

}  // namespace wn
