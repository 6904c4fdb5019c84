// slots_deliver.hip -- the kernel that delivers a step's samples piece by piece (slots_deliver.hpp).  Compiled once, both
// precisions.  A bandwidth kernel: a thread takes one group of 8 samples of one piece -- 32 bytes of the window in, two 16-byte
// stores of samples and one of PCM out.  The destination of a group is 16-byte aligned by construction (offsets are multiples of
// 8 elements); its source is not: a step starts at any window row T, so the rows of a group are only 4-byte aligned and are read
// with 4-byte-aligned 16-byte loads (global memory takes them; nothing is cast to a type that promises more).  Groups that
// straddle the window's wrap, and a piece's tail, go element by element.
#include "slots_deliver.hpp"

namespace wn {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef short shortx8 __attribute__((ext_vector_type(8)));
// 16 bytes at 4-byte alignment
struct __attribute__((packed, aligned(4))) intx4_a4 {
    intx4 v;
};

// blockDim = (gx, 256 / gx): x over the 8-sample groups of a piece, y over pieces; blockIdx.x strides the groups beyond gx,
// blockIdx.y strides the pieces (the grid of the other slot kernels, with the block folded so that short steps fill it).
__global__ __launch_bounds__(256) void slot_deliver_kernel(const int* __restrict__ y, const short* __restrict__ table, int T, int W,
                                                           const DeliverPiece* __restrict__ pieces, int nPieces,
                                                           int* __restrict__ samples, short* __restrict__ pcm) {
    for (int p = blockIdx.y * blockDim.y + threadIdx.y; p < nPieces; p += gridDim.y * blockDim.y) {
        const DeliverPiece pc = pieces[p];
        const int* const row = y + (size_t)pc.slot * W;
        const int groups = (pc.n + 7) >> 3;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int k = g << 3;
            int t = T + k;
            if (t >= W) t -= W;
            if (k + 8 <= pc.n && t + 8 <= W) {
                const intx4 a = ((const intx4_a4*)(row + t))->v, b = ((const intx4_a4*)(row + t + 4))->v;
                if (samples != NULL) {
                    intx4* const out = (intx4*)(samples + pc.offset + k);
                    out[0] = a;
                    out[1] = b;
                }
                if (pcm != NULL) {
                    shortx8 q;
                    q[0] = table[a[0]];
                    q[1] = table[a[1]];
                    q[2] = table[a[2]];
                    q[3] = table[a[3]];
                    q[4] = table[b[0]];
                    q[5] = table[b[1]];
                    q[6] = table[b[2]];
                    q[7] = table[b[3]];
                    *(shortx8*)(pcm + pc.offset + k) = q;
                }
            } else {
                const int m = pc.n - k < 8 ? pc.n - k : 8;
                for (int i = 0; i < m; i++) {
                    const int v = row[t + i < W ? t + i : t + i - W];
                    if (samples != NULL) samples[pc.offset + k + i] = v;
                    if (pcm != NULL) pcm[pc.offset + k + i] = table[v];
                }
            }
        }
    }
}

bool slots_deliver(hipStream_t stream, const int* y, const short* table, int T, int W, int count, const DeliverPiece* pieces, int nPieces,
                   int* samples, short* pcm) {
    if (nPieces <= 0) return true;
    if ((samples == NULL && pcm == NULL) || count <= 0 || count > W || T < 0 || T >= W) return false;
    const int groups = (count + 7) / 8;
    int gx = 1;
    while (gx < groups && gx < 256) gx <<= 1;
    const int gy = 256 / gx;
    int bx = (groups + gx - 1) / gx, by = (nPieces + gy - 1) / gy;
    if (bx > 64) bx = 64;
    if (by > 4096) by = 4096;
    hipLaunchKernelGGL(slot_deliver_kernel, dim3(bx, by), dim3(gx, gy), 0, stream, y, table, T, W, pieces, nPieces, samples, pcm);
    return hipGetLastError() == hipSuccess;
}

}  // namespace wn
