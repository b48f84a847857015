// optimizer.hip — SGD and AdamW over the parameter arena: one flat and one tiled body, each written
// once over an update rule, and the launcher that picks the instantiation (optimizer.h).
// The arithmetic is that of common.h (sgd_update, adamw_update, clip_scale, ema_blend, group_hp).
#include "optimizer.h"

#include "ops_internal.h"

namespace vit {
namespace {
// An update rule: the optimizer state it keeps beside a float4 of p (float4 i of m + at / v + at), the
// hyper-parameters of a parameter-group segment, and the update of one float4.
// p -= lr*g   (optimizer_step, train_vit.rs:737-743)
struct SgdRule {
    static constexpr bool NULLABLE_SHADOW = false;  // the shadow is the compile-time SHADOW
    struct State {};
    static __device__ __forceinline__ float4* state4(float*, long long) { return nullptr; }
    static __device__ __forceinline__ State load(const float4*, const float4*, long long) { return {}; }
    static __device__ __forceinline__ void store(float4*, float4*, long long, const State&) {}
    static __device__ __forceinline__ OptimHp segment_hp(OptimHp hp, const GroupTab& gt, int seg) {
        hp.lr = group_hp(hp.lr, gt.lr_mul[seg]);
        return hp;
    }
    template <bool CLIP>
    static __device__ __forceinline__ void update4(float4& pv, float4 gv, State&, const OptimHp& hp, float c) {
        sgd_update4<CLIP>(pv, gv, hp.lr, c);
    }
};
// AdamW (oracle ref_adamw_step).  One pass: reads p, g, m, v and writes p, m, v
// (+ pbf) = 7 x 4 B (+2 B) per parameter, HBM-bound.
struct AdamwRule {
    static constexpr bool NULLABLE_SHADOW = true;  // pbf tested at run time (fp32 mode has none)
    struct State {
        float4 m, v;
    };
    static __device__ __forceinline__ float4* state4(float* q, long long at) { return reinterpret_cast<float4*>(q + at); }
    static __device__ __forceinline__ State load(const float4* m4, const float4* v4, long long i) {
        return State{m4[i], v4[i]};
    }
    static __device__ __forceinline__ void store(float4* m4, float4* v4, long long i, const State& st) {
        m4[i] = st.m;
        v4[i] = st.v;
    }
    static __device__ __forceinline__ OptimHp segment_hp(OptimHp hp, const GroupTab& gt, int seg) {
        hp.lr = group_hp(hp.lr, gt.lr_mul[seg]);
        hp.wd = group_hp(hp.wd, gt.wd_mul[seg]);
        return hp;
    }
    template <bool CLIP>
    static __device__ __forceinline__ void update4(float4& pv, float4 gv, State& st, const OptimHp& hp, float c) {
        adamw_update4<CLIP>(pv, gv, st.m, st.v, hp.lr, hp.b1, hp.b2, hp.omb1, hp.omb2, hp.bc1, hp.bc2, hp.eps, hp.wd, c);
    }
};

__device__ __forceinline__ uint2 shadow4(const float4& pv) {
    return make_uint2(pack_bf16x2(pv.x, pv.y), pack_bf16x2(pv.z, pv.w));
}

// A flat range: a grid-stride loop over the n4 float4s from p / g / m / v / em.e.
// CLIP: g' = c * g (clip_scale: its own rounding) in place of g.  SHADOW: also pbf = bf16(p').
// EMA: also e = ema_blend(e, p') from the value in registers: one more 16-byte read and
// write per float4 instead of a pass of its own that reads p again.  Its store goes ahead of the shadow's:
// the other order costs the tiled EMA kernels 2 to 4 more VGPRs under hipcc.
template <class R, bool CLIP, bool SHADOW, bool EMA>
__device__ __forceinline__ void flat_body(float* __restrict__ p, bf16_t* __restrict__ pbf,
                                          const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, EmaArg em, long long n4, const OptimHp& hp, float c) {
    const bool shadow = R::NULLABLE_SHADOW ? pbf != nullptr : SHADOW;
    float4* __restrict__ m4 = R::state4(m, 0);
    float4* __restrict__ v4 = R::state4(v, 0);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        float4 gv = reinterpret_cast<const float4*>(g)[i];
        typename R::State st = R::load(m4, v4, i);
        float4 ev;
        if (EMA) ev = reinterpret_cast<float4*>(em.e)[i];
        R::template update4<CLIP>(pv, gv, st, hp, c);
        reinterpret_cast<float4*>(p)[i] = pv;
        R::store(m4, v4, i, st);
        if (EMA) {
            ema_blend4(ev, pv, em.d, em.omd);
            reinterpret_cast<float4*>(em.e)[i] = ev;
        }
        if (shadow) reinterpret_cast<uint2*>(pbf)[i] = shadow4(pv);
    }
}

// One tile of a tiled range: n4 float4s from element beg (a multiple of 64) of the arenas, the
// hyper-parameters hp uniform over the tile.  A full tile issues its GROUP_UNROLL loads per array
// before the first use; a short one (the last of a segment) runs the strided loop.
template <class R, bool CLIP, bool SHADOW, bool EMA>
__device__ __forceinline__ void tile_body(float* __restrict__ p, bf16_t* __restrict__ pbf,
                                          const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, EmaArg em, long long beg, int n4, const OptimHp& hp,
                                          float c) {
    const bool shadow = R::NULLABLE_SHADOW ? pbf != nullptr : SHADOW;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + beg);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + beg);
    float4* __restrict__ m4 = R::state4(m, beg);
    float4* __restrict__ v4 = R::state4(v, beg);
    uint2* __restrict__ b2 = shadow ? reinterpret_cast<uint2*>(pbf + beg) : nullptr;
    float4* __restrict__ e4 = EMA ? reinterpret_cast<float4*>(em.e + beg) : nullptr;
    if (n4 == GROUP_TILE4) {
        float4 pv[GROUP_UNROLL], gv[GROUP_UNROLL], ev[GROUP_UNROLL];
        typename R::State st[GROUP_UNROLL];
#pragma unroll
        for (int k = 0; k < GROUP_UNROLL; k++) {
            const int i = threadIdx.x + k * GROUP_THREADS;
            pv[k] = p4[i];
            gv[k] = g4[i];
            st[k] = R::load(m4, v4, i);
            if (EMA) ev[k] = e4[i];
        }
#pragma unroll
        for (int k = 0; k < GROUP_UNROLL; k++) {
            const int i = threadIdx.x + k * GROUP_THREADS;
            R::template update4<CLIP>(pv[k], gv[k], st[k], hp, c);
            p4[i] = pv[k];
            R::store(m4, v4, i, st[k]);
            if (EMA) {
                ema_blend4(ev[k], pv[k], em.d, em.omd);
                e4[i] = ev[k];
            }
            if (shadow) b2[i] = shadow4(pv[k]);
        }
    } else {
        for (int i = threadIdx.x; i < n4; i += GROUP_THREADS) {
            float4 pv = p4[i];
            typename R::State st = R::load(m4, v4, i);
            R::template update4<CLIP>(pv, g4[i], st, hp, c);
            p4[i] = pv;
            R::store(m4, v4, i, st);
            if (EMA) {
                float4 ev = e4[i];
                ema_blend4(ev, pv, em.d, em.omd);
                e4[i] = ev;
            }
            if (shadow) b2[i] = shadow4(pv);
        }
    }
}
// A tiled range (parameter groups, common.h GroupTab): workgroups stride over the tiles
// [tile_begin, tile_begin + ntiles) of the whole arena, lr_e = lr * lr_mul and (AdamW) wd_e = wd * wd_mul
// of the tile's segment.  A gradient chunk is a tile sub-range.
template <class R, bool CLIP, bool SHADOW, bool EMA>
__device__ __forceinline__ void tiles_body(float* __restrict__ p, bf16_t* __restrict__ pbf,
                                           const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, EmaArg em, const GroupTab& gt, int tile_begin,
                                           int ntiles, const OptimHp& hp, float c) {
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        long long beg;
        int n4;
        const int seg = group_tile(gt, tile_begin + t, beg, n4);
        tile_body<R, CLIP, SHADOW, EMA>(p, pbf, g, m, v, em, beg, n4, R::segment_hp(hp, gt, seg), c);
    }
}

template <bool CLIP, bool SHADOW, bool EMA>
__global__ void sgd_flat_k(OptimArgs a) {
    flat_body<SgdRule, CLIP, SHADOW, EMA>(a.p, a.pbf, a.g, nullptr, nullptr, a.ema, a.n / 4, a.hp, CLIP ? a.rec->c : 1.0f);
}
template <bool CLIP, bool EMA>
__global__ void adamw_flat_k(OptimArgs a) {
    flat_body<AdamwRule, CLIP, false, EMA>(a.p, a.pbf, a.g, a.m, a.v, a.ema, a.n / 4, a.hp, CLIP ? a.rec->c : 1.0f);
}
template <bool CLIP, bool SHADOW, bool EMA>
__global__ __launch_bounds__(GROUP_THREADS) void sgd_tiles_k(OptimArgs a) {
    tiles_body<SgdRule, CLIP, SHADOW, EMA>(a.p, a.pbf, a.g, nullptr, nullptr, a.ema, a.gt, a.tile_begin, a.ntiles, a.hp,
                                           CLIP ? a.rec->c : 1.0f);
}
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(GROUP_THREADS) void adamw_tiles_k(OptimArgs a) {
    tiles_body<AdamwRule, CLIP, false, EMA>(a.p, a.pbf, a.g, a.m, a.v, a.ema, a.gt, a.tile_begin, a.ntiles, a.hp,
                                            CLIP ? a.rec->c : 1.0f);
}

// Every instantiation there is.  SGD: [tiled][CLIP][no shadow | shadow | shadow + EMA] (no shadow: fp32
// mode, whose EMA is ema_update behind the step); AdamW: [tiled][CLIP][EMA].
using OptimKernel = void (*)(OptimArgs);
const OptimKernel kSgd[2][2][3] = {
    {{sgd_flat_k<false, false, false>, sgd_flat_k<false, true, false>, sgd_flat_k<false, true, true>},
     {sgd_flat_k<true, false, false>, sgd_flat_k<true, true, false>, sgd_flat_k<true, true, true>}},
    {{sgd_tiles_k<false, false, false>, sgd_tiles_k<false, true, false>, sgd_tiles_k<false, true, true>},
     {sgd_tiles_k<true, false, false>, sgd_tiles_k<true, true, false>, sgd_tiles_k<true, true, true>}}};
const OptimKernel kAdamw[2][2][2] = {
    {{adamw_flat_k<false, false>, adamw_flat_k<false, true>}, {adamw_flat_k<true, false>, adamw_flat_k<true, true>}},
    {{adamw_tiles_k<false, false>, adamw_tiles_k<false, true>}, {adamw_tiles_k<true, false>, adamw_tiles_k<true, true>}}};

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }
}  // namespace

int group_grid(int ntiles) { return ntiles < 2048 ? ntiles : 2048; }

void optimizer_launch(OptKind kind, const OptimArgs& a, bool tiled, hipStream_t st) {
    const bool adamw = kind == OPT_ADAMW, clip = a.rec != nullptr, shadow = a.pbf != nullptr, ema = a.ema.e != nullptr;
    char what[48];
    snprintf(what, sizeof what, "%s_%s%s%s%s", adamw ? "adamw" : "sgd", tiled ? "tiles" : "flat", clip ? "_clip" : "",
             shadow ? "_shadow" : "", ema ? "_ema" : "");
    VIT_REQUIRE(adamw || shadow || !ema, "%s: SGD without a bf16 shadow has no fused EMA", what);
    // (the flat bodies have no scalar tail: arena and chunk extents are multiples of 64 elements)
    VIT_REQUIRE(tiled || (a.n % 4 == 0 && aligned16(a.p) && aligned16(a.g) && aligned16(a.m) && aligned16(a.v) &&
                          aligned16(a.ema.e) && ((uintptr_t)a.pbf & 7) == 0),
                "%s: a flat range must be whole 16-byte aligned float4s (n %lld)", what, a.n);
    if (tiled ? a.ntiles <= 0 : a.n <= 0) return;
    const OptimKernel k = adamw ? kAdamw[tiled][clip][ema] : kSgd[tiled][clip][shadow + ema];
    if (tiled)
        k<<<group_grid(a.ntiles), GROUP_THREADS, 0, st>>>(a);
    else
        k<<<grid_for(a.n / 4, 256), 256, 0, st>>>(a);
    after_launch(what);
    if (ema) count_hit(VIT_HIT_EMA);
}
}  // namespace vit
