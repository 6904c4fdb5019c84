// Host-only checker of the LDS layout of wn::wavenet_wg (tests/test_lds_layout_cpu.py compiles and runs it; no GPU): for every
// Cfg the library instantiates, from the Cfg constants alone,
//  * no two regions that are live in the same phase of a sample overlap
//      layers: x, h, tap image, ring slots, bias + embedding tables, y, skip (stored right behind the last layer);   head: skip, zs / logits, y, ring slots, bias + tables
//  * every planned ring slot is 16-byte aligned and inside the launch's LDS, and ringSlotOffset is injective over them
//  * the planner's total never exceeds the 160 KiB of a CU.
// The planner (nvWavenetInfer::placeLdsRing / planEmb, which need a device to construct) is restated here from the same constants,
// and its result for C3 is printed in the words of kernelInfo.
#include <cstdio>
#include <vector>

#include "wn_kernels.hpp"

static constexpr int kLdsMax = 160 * 1024;
static int failures = 0;

struct Region {
    const char* name;
    int lo, hi;
};

static void disjoint(const char* cfg, const char* phase, const std::vector<Region>& rs) {
    for (size_t i = 0; i < rs.size(); i++)
        for (size_t k = i + 1; k < rs.size(); k++)
            if (rs[i].lo < rs[k].hi && rs[k].lo < rs[i].hi && rs[i].lo < rs[i].hi && rs[k].lo < rs[k].hi) {
                printf("FAIL %s %s: %s [%d,%d) overlaps %s [%d,%d)\n", cfg, phase, rs[i].name, rs[i].lo, rs[i].hi, rs[k].name, rs[k].lo, rs[k].hi);
                failures++;
            }
}

// placeLdsRing: the largest dilation whose slots fit; *tail: bytes of dynamic LDS behind the tables
template <class C> static int place(int L, int maxD, int need, int* tail) {
    int D = 0;
    for (int d = 1; d <= maxD; d <<= 1)
        if (need + C::ringTailSlots(C::ldsRingSlots(L, maxD, d)) * C::RING_SLOT <= kLdsMax) D = d;
    *tail = C::ringTailSlots(C::ldsRingSlots(L, maxD, D)) * C::RING_SLOT;
    return D;
}
// embTables + planEmb of a dump-free launch that may keep ring slots in LDS
template <class C> static int plan_emb(int L, int maxD) {
    int n = (int)C::ldsBytes(L, 2, false) <= kLdsMax ? 2 : (int)C::ldsBytes(L, 1, false) <= kLdsMax ? 1 : 0;
    if (n == 2) {
        int tail;
        const int D2 = place<C>(L, maxD, (int)C::ldsBytes(L, 2, false), &tail), D1 = place<C>(L, maxD, (int)C::ldsBytes(L, 1, false), &tail);
        if (D2 == 0 || (D2 < 2 && D1 > D2)) n = 1;
    }
    return n;
}

template <bool F16, int R, int S, int A, int BT, int KFC> static void check_cfg() {
    using C = wn::Cfg<F16, R, S, A, BT, KFC>;
    char cfg[96];
    snprintf(cfg, sizeof(cfg), "Cfg<%s,%d,%d,%d,BT=%d,KFC=%d>", F16 ? "fp16" : "fp32", R, S, A, BT, KFC);
    static_assert(C::OFF_X % 16 == 0 && C::OFF_H % 16 == 0 && C::OFF_XP % 16 == 0 && C::OFF_BIAS % 16 == 0 && C::LDS_FIXED % 16 == 0, "images are 16-byte aligned");
    const int shapes[][2] = {{20, 512}, {20, 32}, {30, 512}, {12, 8}, {7, 4}, {6, 8}, {1, 1}};
    for (const auto& sh : shapes) {
        const int L = sh[0], maxD = sh[1];
        for (int nEmb = 0; nEmb <= 2; nEmb++) {
            const int need = (int)C::ldsBytes(L, nEmb, false);
            if (need > kLdsMax) continue;
            int tail;
            const int D = place<C>(L, maxD, need, &tail);
            const int slots = C::ldsRingSlots(L, maxD, D), total = need + tail;
            if (total > kLdsMax) {
                printf("FAIL %s L=%d maxD=%d emb=%d: %d bytes of LDS\n", cfg, L, maxD, nEmb, total);
                failures++;
            }
            std::vector<Region> ring;
            static char names[64][16];
            for (int s = 0; s < slots; s++) {
                const int off = C::ringSlotOffset(s, need);
                if (off % 16 != 0 || off < 0 || off + C::RING_SLOT > total) {
                    printf("FAIL %s L=%d maxD=%d emb=%d: slot %d at %d (launch has %d)\n", cfg, L, maxD, nEmb, s, off, total);
                    failures++;
                }
                if (s < 64) {
                    snprintf(names[s], sizeof(names[s]), "slot%d", s);
                    ring.push_back({names[s], off, off + C::RING_SLOT});      // (pairwise disjoint = injective)
                } else if (s == 64) {
                    // beyond the named ones the tail is a plain array behind the last of them: one region
                    ring.push_back({"slots64+", off, C::ringSlotOffset(slots - 1, need) + C::RING_SLOT});
                }
            }
            std::vector<Region> layers = ring, head = ring;
            const Region tables = {"bias+tables", C::OFF_BIAS, need - C::RING_INPLACE * C::RING_SLOT}, y = {"y", C::OFF_Y, C::OFF_Y + C::YBUF};
            layers.push_back({"x", C::OFF_X, C::OFF_X + C::XBUF});
            layers.push_back({"h", C::OFF_H, C::OFF_H + C::HBUF});
            layers.push_back({"tap", C::OFF_XP, C::OFF_XP + C::XPBUF});
            layers.push_back(tables);
            layers.push_back(y);
            // (the skip image is written behind the last layer with no barrier in between: other waves may still be reading x and the tap)
            layers.push_back({"skip", C::OFF_SK, C::OFF_SK + C::SKBUF});
            head.push_back({"skip", C::OFF_SK, C::OFF_SK + C::SKBUF});
            const int zsEnd = C::OFF_ZS + C::ZSBUF, lgEnd = C::OFF_LG + C::LGBUF;
            if (C::ALIAS_LG) head.push_back({"zs|logits", C::OFF_ZS, zsEnd > lgEnd ? zsEnd : lgEnd});      // (one after the other, a barrier between)
            else {
                head.push_back({"zs", C::OFF_ZS, zsEnd});
                head.push_back({"logits", C::OFF_LG, lgEnd});
            }
            head.push_back(tables);
            head.push_back(y);
            disjoint(cfg, "layers", layers);
            disjoint(cfg, "head", head);
            for (const std::vector<Region>* rs : {&layers, &head})
                for (const Region& r : *rs)
                    if (r.lo < 0 || r.hi > total) {
                        printf("FAIL %s L=%d maxD=%d emb=%d: %s [%d,%d) outside the launch's %d bytes\n", cfg, L, maxD, nEmb, r.name, r.lo, r.hi, total);
                        failures++;
                    }
        }
    }
    printf("ok %s overlay=%d in_place_slots=%d\n", cfg, C::OVERLAY ? 1 : 0, C::RING_INPLACE);
}

// the tile counts the engine builds for a shape (nvWavenetInfer::WG2 / WG3 / WG4), packed conditioning and features (KFC)
template <bool F16, int R, int S, int A> static void check_shape() {
    check_cfg<F16, R, S, A, 1, 0>();
    check_cfg<F16, R, S, A, 1, wn::feat_kfc<F16>()>();
    if constexpr (R < 128) {
        check_cfg<F16, R, S, A, 2, 0>();
        check_cfg<F16, R, S, A, 2, wn::feat_kfc<F16>()>();
    }
    if constexpr (F16 && R <= 64) {
        check_cfg<F16, R, S, A, 3, 0>();
        check_cfg<F16, R, S, A, 3, wn::feat_kfc<F16>()>();
        check_cfg<F16, R, S, A, 4, 0>();
    }
}

// C3 (R 64 / S 256 / A 256, 20 layers, maxDilation 512, fp16), dump-free packed launch: what kernelInfo prints
template <int BT> static void plan_c3() {
    using C = wn::Cfg<true, 64, 256, 256, BT>;
    const int nEmb = plan_emb<C>(20, 512), need = (int)C::ldsBytes(20, nEmb, false);
    int tail;
    const int D = place<C>(20, 512, need, &tail);
    printf("plan BT=%d,EMBLDS=%d lds=%d ring_in_lds=d<=%d slots=%d tail_slots=%d\n", BT, nEmb, need + tail, D, C::ldsRingSlots(20, 512, D),
           tail / C::RING_SLOT);
}

int main() {
#define X(R, S, A, P) check_shape<P == 16, R, S, A>();
    WN_LAYOUT_INSTANCES
#undef X
    plan_c3<1>();
    plan_c3<2>();
    plan_c3<3>();
    plan_c3<4>();
    printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
