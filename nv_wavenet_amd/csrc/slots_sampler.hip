// slots_sampler.hip -- the kernel that writes the changed columns' softmax scales, probability floors and cuts into the engine's table
// (slots_sampler.hpp).  Compiled once, both precisions.  At most 4 maxBatch entries of 8 bytes per step: one thread per entry.
#include "slots_sampler.hpp"

#include "gpu_check.hpp"

namespace wn {

SamplingTable::~SamplingTable() {
    if (softScale) gpuErrChk(hipFree(softScale));
}
void SamplingTable::make() {
    gpuErrChk(hipMalloc(&softScale, kSamplingKinds * (size_t)columns * sizeof(float)));
    upload();      // (the host's values before the one that makes the table: off in every column)
}
void SamplingTable::set(int b, const Sampling& s) {
    const bool off = s == Sampling{};
    if (rows.empty()) {
        if (off) return;
        rows.assign(columns, Sampling{});
    }
    if (!off && !softScale) make();
    int now[kSamplingKinds], was[kSamplingKinds];
    sampling_words(s, now);
    sampling_words(rows[b], was);
    for (int k = 0; k < kSamplingKinds; k++) on[k] += (now[k] != 0) - (was[k] != 0);
    rows[b] = s;
}
void SamplingTable::reset(bool deviceBehind) {
    const bool rewrite = softScale && (on[kTemperature] > 0 || on[kMinP] > 0 || cutting() > 0 || deviceBehind);
    rows.clear();
    for (int& n : on) n = 0;
    if (rewrite) {
        gpuErrChk(hipDeviceSynchronize());
        upload();
    }
}
void SamplingTable::upload() {
    if (!softScale) return;
    std::vector<float> c(kSamplingKinds * (size_t)columns);
    for (int b = 0; b < columns; b++) {
        float entry[kSamplingKinds];
        sampling_entries(get(b), entry);      // (rows is empty when every value is off)
        for (int k = 0; k < kSamplingKinds; k++) c[k * (size_t)columns + b] = entry[k];
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
