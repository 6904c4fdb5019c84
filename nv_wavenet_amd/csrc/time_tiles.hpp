// time_tiles.hpp -- the device functions of the time-parallel passes (time_kernels.hpp, mel_time.hip): 16 consecutive samples of one
// utterance in the MFMA N dimension, x of a sample as a scratch row laid out like a blob slot.
#pragma once

#include "wn_kernels.hpp"

namespace wn {

template <bool F16, int R> struct PCfg {
    using P = Prec<F16>;
    static constexpr int TPF = P::TPF;
    static constexpr int RT = R / 16, NW = RT >= 4 ? 4 : RT, HTW = RT / NW, KF_R = RT / TPF;      // (as Cfg: wave w owns tiles w, w + NW, ..)
    static constexpr int THREADS = NW * 64;
    static constexpr int KFC = feat_kfc<F16>();
    static constexpr int ROWB = KF_R * 64;                   // bytes of one sample's x in T_data = of one blob slot
};
// where the quad of channels 16 * tile + 4g .. + 3 lies in a scratch row / blob slot: piece [fragment][g], as slot_save_kernel lays them out
template <bool F16> WN_DEV int quad_off(int tile, int g) {
    if constexpr (F16) return (((tile >> 1) * 4 + g) << 4) + ((tile & 1) << 3);
    else return (tile * 4 + g) << 4;
}
// the rounding of lds_put_tile
template <bool F16> WN_DEV void put_quad(char* at, floatx4 v) {
    if constexpr (F16) *(half4*)at = half4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    else *(floatx4*)at = v;
}
WN_DEV int clamp_sample(int y, int A) { return y < 0 ? 0 : y >= A ? A - 1 : y; }

// B fragments of the features of this lane's sample (column kk of the caller's tensor, channels 4g .. of every 16), converted as
// the window feed converts them (slot_feed_kernel)
template <bool F16, int KFC>
WN_DEV void feature_frags(const void* x, int precision, long long cStride, long long tStride, long long kk, int nCond, int g,
                          typename Prec<F16>::frag (&cf)[KFC]) {
    using P = Prec<F16>;
    using elem = typename P::elem;
#pragma unroll
    for (int kf = 0; kf < KFC; kf++)
#pragma unroll
        for (int e = 0; e < P::EPL; e++) {
            const int c = (kf * P::TPF + (e >> 2)) * 16 + 4 * g + (e & 3);
            float v = 0.f;
            if (c < nCond) {
                const long long at = c * cStride + kk * tStride;
                v = precision == 16 ? (float)((const _Float16*)x)[at] : ((const float*)x)[at];
            }
            cf[kf][e] = (elem)v;
        }
}

}  // namespace wn
