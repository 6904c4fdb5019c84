// slots_prime.hip -- the two kernels that write forced samples into selector tables (slots_prime.hpp), and the lockstep engine's
// PrimeTable.  Compiled once, both precisions.
#include "slots_prime.hpp"

#include "gpu_check.hpp"
#include "wn_kernels.hpp"

namespace wn {

PrimeTable::~PrimeTable() {
    for (void* q : {(void*)yDev, (void*)nDev, (void*)sel})
        if (q) gpuErrChk(hipFree(q));
}
void PrimeTable::set(const int* y, const int* len, int batch, int maxLen, long long stride, int maxSamples) {
    gpuErrChk(hipDeviceSynchronize());
    n.assign(columns, 0);
    maxN = 0;
    primed = 0;
    for (int b = 0; b < batch; b++) {
        n[b] = len[b];
        if (n[b] > maxN) maxN = n[b];
        primed += n[b] > 0;
    }
    if (maxN == 0) return;
    if (maxLen > yStride) {
        if (yDev) gpuErrChk(hipFree(yDev));
        gpuErrChk(hipMalloc((void**)&yDev, (size_t)columns * maxLen * sizeof(int)));
        yStride = maxLen;
    }
    if (!nDev) gpuErrChk(hipMalloc((void**)&nDev, (size_t)columns * sizeof(int)));
    if (!sel) gpuErrChk(hipMalloc((void**)&sel, (size_t)maxSamples * columns * sizeof(float)));
    gpuErrChk(hipMemcpy2D(yDev, (size_t)yStride * sizeof(int), y, (size_t)stride * sizeof(int), (size_t)maxLen * sizeof(int), batch,
                          hipMemcpyDefault));
    gpuErrChk(hipMemcpy(nDev, n.data(), (size_t)columns * sizeof(int), hipMemcpyHostToDevice));
}
void PrimeTable::clear() {
    n.clear();
    maxN = 0;
    primed = 0;
}

// blockIdx.y walks the entries, x the step's samples: one 4-byte store per forced sample of the step
__global__ __launch_bounds__(256) void slot_prime_kernel(float* __restrict__ sel, int maxBatch, long long counter, int T, int W, int count,
                                                         const SlotPrime* __restrict__ tab, int n, const SlotDesc* __restrict__ desc,
                                                         const MelDesc* __restrict__ melDesc, int A) {
    for (int e = blockIdx.y; e < n; e += gridDim.y) {
        const SlotPrime q = tab[e];
        if (q.column < 0 || q.column >= maxBatch) continue;
        const bool mel = melDesc != nullptr && melDesc[q.column].state != 0;
        if (!mel && !desc[q.column].active) continue;
        const long long k0 = counter - (mel ? melDesc[q.column].start : desc[q.column].start);
        if (k0 < 0 || k0 >= q.n) continue;
        const long long left = (long long)q.n - k0;
        const int m = left < count ? (int)left : count;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
            sel[(size_t)((T + i) % W) * maxBatch + q.column] = prime_selector(q.y[k0 + i], A);
    }
}

__global__ __launch_bounds__(256) void prime_selectors_kernel(float* __restrict__ out, int first, int count, int batch, int maxBatch,
                                                              const int* __restrict__ y, int yStride, const int* __restrict__ n, int useRng,
                                                              unsigned key0, unsigned key1, const float* __restrict__ selIn, int A) {
    const size_t cells = (size_t)count * batch;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i % batch), t = first + (int)(i / batch);
        const size_t at = (size_t)t * maxBatch + b;
        float s;
        if (t < n[b]) s = prime_selector(y[(size_t)b * yStride + t], A);
        else if (useRng) s = philox_selector(key0, key1, (unsigned)t, (unsigned)b);
        else {
            s = selIn[at];
            if (s <= -1.0f) s = -0.5f;
        }
        out[at] = s;
    }
}

bool slots_prime(hipStream_t stream, float* sel, int maxBatch, long long counter, int T, int W, int count, const SlotPrime* tab, int n,
                 const SlotDesc* desc, const MelDesc* melDesc, int A) {
    if (n <= 0 || count <= 0) return true;
    if (sel == NULL || tab == NULL || desc == NULL || maxBatch <= 0 || n > maxBatch || W <= 0 || T < 0 || T >= W || count > W || A <= 0) return false;
    const int gx = (count + 255) / 256 > 16 ? 16 : (count + 255) / 256;
    hipLaunchKernelGGL(slot_prime_kernel, dim3(gx, n > 16384 ? 16384 : n), dim3(256), 0, stream, sel, maxBatch, counter, T, W, count, tab, n,
                       desc, melDesc, A);
    return hipGetLastError() == hipSuccess;
}

bool prime_selectors(hipStream_t stream, float* out, int first, int count, int batch, int maxBatch, const int* y, int yStride, const int* n,
                     int useRng, unsigned long long seed, const float* selIn, int A) {
    if (count <= 0) return true;
    if (out == NULL || y == NULL || n == NULL || first < 0 || batch < 1 || batch > maxBatch || (!useRng && selIn == NULL) || A <= 0) return false;
    size_t g = ((size_t)count * batch + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(prime_selectors_kernel, dim3((unsigned)g), dim3(256), 0, stream, out, first, count, batch, maxBatch, y, yStride, n, useRng,
                       (unsigned)seed, (unsigned)(seed >> 32), selIn, A);
    return hipGetLastError() == hipSuccess;
}

}  // namespace wn
