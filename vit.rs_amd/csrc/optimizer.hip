// optimizer.hip — SGD, momentum SGD and AdamW over the parameter arena: one flat and one tiled body, each written
// once over an update rule, and the launcher that picks the instantiation (optimizer.h).
// The arithmetic is that of common.h (sgd_update, sgdm_update, adamw_update, clip_scale, ema_blend, group_hp).
// LAMB is three kernels of its own over the same tiles, behind the launcher's LambArgs form.
#include "optimizer.h"

#include <cmath>

#include "../../include/vit_trainer.h"
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

// Momentum SGD (torch.optim.SGD): the buffer b beside p (float4 i of m + at).  One pass:
// reads p, g, b and writes p, b (+ pbf) = 5 x 4 B (+2 B) per parameter.  wd_e != 0, nesterov and first are
// wave-uniform (hp comes from the kernel arguments and the segment's scalar loads).
struct SgdmRule {
    static constexpr bool NULLABLE_SHADOW = true;  // pbf tested at run time (fp32 mode has none)
    struct State {
        float4 b;
    };
    static __device__ __forceinline__ float4* state4(float* q, long long at) { return reinterpret_cast<float4*>(q + at); }
    static __device__ __forceinline__ State load(const float4* b4, const float4*, long long i) { return State{b4[i]}; }
    static __device__ __forceinline__ void store(float4* b4, float4*, long long i, const State& st) { b4[i] = st.b; }
    static __device__ __forceinline__ OptimHp segment_hp(OptimHp hp, const GroupTab& gt, int seg) {
        hp.lr = group_hp(hp.lr, gt.lr_mul[seg]);
        hp.wd = group_hp(hp.wd, gt.wd_mul[seg]);
        return hp;
    }
    template <bool CLIP>
    static __device__ __forceinline__ void update4(float4& pv, float4 gv, State& st, const OptimHp& hp, float c) {
        sgdm_update4<CLIP>(pv, gv, st.b, hp.lr, hp.mu, hp.omd, hp.wd, hp.nesterov != 0, hp.first != 0, c);
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
template <bool CLIP, bool EMA>
__global__ void sgdm_flat_k(OptimArgs a) {
    flat_body<SgdmRule, CLIP, false, EMA>(a.p, a.pbf, a.g, a.m, nullptr, a.ema, a.n / 4, a.hp, CLIP ? a.rec->c : 1.0f);
}
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(GROUP_THREADS) void sgdm_tiles_k(OptimArgs a) {
    tiles_body<SgdmRule, CLIP, false, EMA>(a.p, a.pbf, a.g, a.m, nullptr, a.ema, a.gt, a.tile_begin, a.ntiles, a.hp,
                                           CLIP ? a.rec->c : 1.0f);
}
// sgd_momentum_step (include/vit_ops.h): the scalar form, any n and any alignment
__global__ void sgdm_scalar_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ b, long long n,
                              OptimHp hp) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float bi = b[i];
        p[i] = sgdm_update(p[i], g[i], bi, hp.lr, hp.mu, hp.omd, hp.wd, hp.nesterov != 0, hp.first != 0);
        b[i] = bi;
    }
}

// Every instantiation there is.  SGD: [tiled][CLIP][no shadow | shadow | shadow + EMA] (no shadow: fp32
// mode, whose EMA is ema_update behind the step); AdamW and momentum SGD: [tiled][CLIP][EMA].
using OptimKernel = void (*)(OptimArgs);
const OptimKernel kSgd[2][2][3] = {
    {{sgd_flat_k<false, false, false>, sgd_flat_k<false, true, false>, sgd_flat_k<false, true, true>},
     {sgd_flat_k<true, false, false>, sgd_flat_k<true, true, false>, sgd_flat_k<true, true, true>}},
    {{sgd_tiles_k<false, false, false>, sgd_tiles_k<false, true, false>, sgd_tiles_k<false, true, true>},
     {sgd_tiles_k<true, false, false>, sgd_tiles_k<true, true, false>, sgd_tiles_k<true, true, true>}}};
const OptimKernel kAdamw[2][2][2] = {
    {{adamw_flat_k<false, false>, adamw_flat_k<false, true>}, {adamw_flat_k<true, false>, adamw_flat_k<true, true>}},
    {{adamw_tiles_k<false, false>, adamw_tiles_k<false, true>}, {adamw_tiles_k<true, false>, adamw_tiles_k<true, true>}}};
const OptimKernel kSgdm[2][2][2] = {
    {{sgdm_flat_k<false, false>, sgdm_flat_k<false, true>}, {sgdm_flat_k<true, false>, sgdm_flat_k<true, true>}},
    {{sgdm_tiles_k<false, false>, sgdm_tiles_k<false, true>}, {sgdm_tiles_k<true, false>, sgdm_tiles_k<true, true>}}};

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// ------------------------------------------------------------------ LAMB
// A tile is GROUP_TILE elements of one segment (the last may be short: cnt valid elements); thread t owns
// the float4s t + k * GROUP_THREADS, k < GROUP_UNROLL, of it, in the trainer (VEC: the tile starts on a
// 64-element boundary of the arenas) as in the lamb_step op (!VEC: any alignment).  A float4 wholly inside
// the segment is one 16-byte access under VEC; the others go element by element and stop at cnt, so
// nothing behind the tensor's own length is read into a sum or written.
template <bool VEC>
__device__ __forceinline__ float4 lamb_load4(const float* __restrict__ q, int i, int cnt) {
    if (VEC && 4 * i + 4 <= cnt) return reinterpret_cast<const float4*>(q)[i];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    const int e = 4 * i;
    if (e < cnt) r.x = q[e];
    if (e + 1 < cnt) r.y = q[e + 1];
    if (e + 2 < cnt) r.z = q[e + 2];
    if (e + 3 < cnt) r.w = q[e + 3];
    return r;
}
template <bool VEC>
__device__ __forceinline__ void lamb_store4(float* __restrict__ q, int i, int cnt, const float4& x) {
    if (VEC && 4 * i + 4 <= cnt) {
        reinterpret_cast<float4*>(q)[i] = x;
        return;
    }
    const int e = 4 * i;
    if (e < cnt) q[e] = x.x;
    if (e + 1 < cnt) q[e + 1] = x.y;
    if (e + 2 < cnt) q[e + 2] = x.z;
    if (e + 3 < cnt) q[e + 3] = x.w;
}
template <bool VEC>
__device__ __forceinline__ void lamb_store_shadow4(bf16_t* __restrict__ q, int i, int cnt, const float4& x) {
    if (VEC && 4 * i + 4 <= cnt) {
        reinterpret_cast<uint2*>(q)[i] = shadow4(x);
        return;
    }
    const int e = 4 * i;
    if (e < cnt) q[e] = f2bf(x.x);
    if (e + 1 < cnt) q[e + 1] = f2bf(x.y);
    if (e + 2 < cnt) q[e + 2] = f2bf(x.z);
    if (e + 3 < cnt) q[e + 3] = f2bf(x.w);
}
// acc += (double)x * (double)x as one fused multiply-add: the product of two fp32 values is exact in double
__device__ __forceinline__ void lamb_sq(double& acc, float x) { acc = __builtin_fma((double)x, (double)x, acc); }

// the direction of one float4 from the moments as they stand (both passes), its clipped gradient and the
// moments' advance in front of it (pass 1)
__device__ __forceinline__ float4 lamb_direction4(const float4& pv, const float4& mv, const float4& vv,
                                                  const OptimHp& hp) {
    return make_float4(adamw_direction(pv.x, mv.x, vv.x, hp.bc1, hp.bc2, hp.eps, hp.wd),
                       adamw_direction(pv.y, mv.y, vv.y, hp.bc1, hp.bc2, hp.eps, hp.wd),
                       adamw_direction(pv.z, mv.z, vv.z, hp.bc1, hp.bc2, hp.eps, hp.wd),
                       adamw_direction(pv.w, mv.w, vv.w, hp.bc1, hp.bc2, hp.eps, hp.wd));
}
template <bool CLIP>
__device__ __forceinline__ float4 lamb_moments4(const float4& pv, float4 gv, float4& mv, float4& vv,
                                                const OptimHp& hp, float c) {
    if (CLIP) {
        gv.x = clip_scale(c, gv.x); gv.y = clip_scale(c, gv.y);
        gv.z = clip_scale(c, gv.z); gv.w = clip_scale(c, gv.w);
    }
    float4 u;
    u.x = adamw_moments(pv.x, gv.x, mv.x, vv.x, hp.b1, hp.b2, hp.omb1, hp.omb2, hp.bc1, hp.bc2, hp.eps, hp.wd);
    u.y = adamw_moments(pv.y, gv.y, mv.y, vv.y, hp.b1, hp.b2, hp.omb1, hp.omb2, hp.bc1, hp.bc2, hp.eps, hp.wd);
    u.z = adamw_moments(pv.z, gv.z, mv.z, vv.z, hp.b1, hp.b2, hp.omb1, hp.omb2, hp.bc1, hp.bc2, hp.eps, hp.wd);
    u.w = adamw_moments(pv.w, gv.w, mv.w, vv.w, hp.b1, hp.b2, hp.omb1, hp.omb2, hp.bc1, hp.bc2, hp.eps, hp.wd);
    return u;
}
// p^2 and u^2 of float4 i into the thread's sums, x y z w in order; the elements at and behind cnt count as
// zero (their u is not looked at: it may be 0 / 0)
__device__ __forceinline__ void lamb_acc4(double& W, double& U, const float4& pv, const float4& u, int i, int cnt) {
    const int e = 4 * i;
    lamb_sq(W, pv.x);  // (loaded as 0 behind cnt)
    lamb_sq(W, pv.y);
    lamb_sq(W, pv.z);
    lamb_sq(W, pv.w);
    lamb_sq(U, e < cnt ? u.x : 0.f);
    lamb_sq(U, e + 1 < cnt ? u.y : 0.f);
    lamb_sq(U, e + 2 < cnt ? u.z : 0.f);
    lamb_sq(U, e + 3 < cnt ? u.w : 0.f);
}

// tile `tile` of a LAMB launch: its segment, first element and own length, and the segment's lr_e / wd_e.
// OP (the lamb_step op): one segment of a.o.n elements from the pointers, multipliers 1.
template <bool OP>
__device__ __forceinline__ int lamb_tile(const LambArgs& a, int tile, long long& beg, int& cnt, OptimHp& hp) {
    hp = a.o.hp;
    if (OP) {
        beg = (long long)tile * GROUP_TILE;
        const long long left = a.o.n - beg;
        cnt = left < GROUP_TILE ? (int)left : GROUP_TILE;
        return 0;
    }
    int n4;
    const int seg = group_tile(a.o.gt, tile, beg, n4);
    const long long left = a.seg_len[seg] - (long long)(tile - a.o.gt.tile0[seg]) * GROUP_TILE;
    cnt = left < GROUP_TILE ? (int)left : GROUP_TILE;
    hp = AdamwRule::segment_hp(hp, a.o.gt, seg);
    return seg;
}

// Pass 1, a workgroup per tile (grid-strided): m' and v' stored, u kept in registers, slots[tile] = the
// tile's {sum p^2, sum u^2}: per thread in element order, the xor butterfly over the wave, the waves in
// order through LDS (sumsq_partial_k's scheme).  The slot is that of the global tile number, so the bits
// do not depend on the grid.  A full tile issues its loads before the first use, like tile_body.
template <bool CLIP, bool OP>
__global__ __launch_bounds__(GROUP_THREADS) void lamb_moments_tiles_k(LambArgs a) {
    constexpr bool VEC = !OP;
    __shared__ double wsum[2][GROUP_THREADS / 64];
    const float c = CLIP ? a.o.rec->c : 1.0f;
    const int ntiles = OP ? lamb_tiles(a.o.n) : a.o.ntiles;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        long long beg;
        int cnt;
        OptimHp hp;
        lamb_tile<OP>(a, a.o.tile_begin + t, beg, cnt, hp);
        const float* __restrict__ p = a.o.p + beg;
        const float* __restrict__ g = a.o.g + beg;
        float* __restrict__ m = a.o.m + beg;
        float* __restrict__ v = a.o.v + beg;
        double W = 0.0, U = 0.0;
        if (VEC && cnt == GROUP_TILE) {
            float4 pv[GROUP_UNROLL], gv[GROUP_UNROLL], mv[GROUP_UNROLL], vv[GROUP_UNROLL];
#pragma unroll
            for (int k = 0; k < GROUP_UNROLL; k++) {
                const int i = threadIdx.x + k * GROUP_THREADS;
                pv[k] = reinterpret_cast<const float4*>(p)[i];
                gv[k] = reinterpret_cast<const float4*>(g)[i];
                mv[k] = reinterpret_cast<const float4*>(m)[i];
                vv[k] = reinterpret_cast<const float4*>(v)[i];
            }
#pragma unroll
            for (int k = 0; k < GROUP_UNROLL; k++) {
                const int i = threadIdx.x + k * GROUP_THREADS;
                const float4 u = lamb_moments4<CLIP>(pv[k], gv[k], mv[k], vv[k], hp, c);
                reinterpret_cast<float4*>(m)[i] = mv[k];
                reinterpret_cast<float4*>(v)[i] = vv[k];
                lamb_acc4(W, U, pv[k], u, i, GROUP_TILE);
            }
        } else {
            for (int i = threadIdx.x; 4 * i < cnt; i += GROUP_THREADS) {
                const float4 pv = lamb_load4<VEC>(p, i, cnt);
                float4 mv = lamb_load4<VEC>(m, i, cnt), vv = lamb_load4<VEC>(v, i, cnt);
                const float4 u = lamb_moments4<CLIP>(pv, lamb_load4<VEC>(g, i, cnt), mv, vv, hp, c);
                lamb_store4<VEC>(m, i, cnt, mv);
                lamb_store4<VEC>(v, i, cnt, vv);
                lamb_acc4(W, U, pv, u, i, cnt);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            W += __shfl_xor(W, o, 64);
            U += __shfl_xor(U, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            wsum[0][threadIdx.x >> 6] = W;
            wsum[1][threadIdx.x >> 6] = U;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double tw = wsum[0][0], tu = wsum[1][0];
#pragma unroll
            for (int w = 1; w < GROUP_THREADS / 64; w++) {
                tw += wsum[0][w];
                tu += wsum[1][w];
            }
            a.slots[a.o.tile_begin + t] = make_double2(tw, tu);
        }
        __syncthreads();  // wsum is free for the workgroup's next tile
    }
}

// Pass 2, a wave per segment: W and U = the segment's slots summed in a fixed order (lane l takes slots
// l, l + 64, ... of the segment in order, then the butterfly), the norms rounded to fp32 and the trust
// ratio: wn / un in fp32 (IEEE division) where the segment is adapted and both norms are positive (a NaN
// norm fails the comparison), 1 otherwise; timm's rule adapts a segment iff its weight decay is not zero,
// VIT_LAMB_ALWAYS_ADAPT every one; VIT_LAMB_TRUST_CLIP caps the ratio at 1.
template <bool OP>
__global__ __launch_bounds__(GROUP_THREADS) void lamb_ratio_k(LambArgs a) {
    const int nseg = OP ? 1 : a.o.gt.nseg;
    const int s = blockIdx.x * (GROUP_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= nseg) return;
    const int t0 = OP ? 0 : a.o.gt.tile0[s], t1 = OP ? lamb_tiles(a.o.n) : a.o.gt.tile0[s + 1];
    double W = 0.0, U = 0.0;
    for (int t = t0 + lane; t < t1; t += 64) {
        const double2 x = a.slots[t];
        W += x.x;
        U += x.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        W += __shfl_xor(W, o, 64);
        U += __shfl_xor(U, o, 64);
    }
    if (lane != 0) return;
    const float wd_e = OP ? a.o.hp.wd : group_hp(a.o.hp.wd, a.o.gt.wd_mul[s]);
    const float wn = (float)__builtin_sqrt(W), un = (float)__builtin_sqrt(U);
    const bool adapt = (a.flags & VIT_LAMB_ALWAYS_ADAPT) || wd_e != 0.f;
    float r = (adapt && wn > 0.f && un > 0.f) ? wn / un : 1.0f;
    if ((a.flags & VIT_LAMB_TRUST_CLIP) && !(r < 1.0f)) r = 1.0f;
    a.rec[s * LAMB_REC + 0] = wn;
    a.rec[s * LAMB_REC + 1] = un;
    a.rec[s * LAMB_REC + 2] = r;
}

// p' = p - step * u of one float4 with step = lr_e * r, every product and the difference rounded on its own
__device__ __forceinline__ float lamb_apply(float p, float u, float step) {
#pragma clang fp contract(off)
    return p - step * u;
}
__device__ __forceinline__ void lamb_apply4(float4& pv, const float4& u, float step) {
    pv.x = lamb_apply(pv.x, u.x, step); pv.y = lamb_apply(pv.y, u.y, step);
    pv.z = lamb_apply(pv.z, u.z, step); pv.w = lamb_apply(pv.w, u.w, step);
}
// Pass 3, tiles as in pass 1: u again from p and the stored m', v' by the function pass 1 used (nothing it
// reads has changed: the same bits), p' = p - (lr_e * r) * u, then AdamW's tail: the bf16 shadow (pbf
// non-null) and, EMA, e = ema_blend(e, p').
template <bool EMA, bool OP>
__global__ __launch_bounds__(GROUP_THREADS) void lamb_apply_tiles_k(LambArgs a) {
    constexpr bool VEC = !OP;
    const int ntiles = OP ? lamb_tiles(a.o.n) : a.o.ntiles;
    const bool shadow = a.o.pbf != nullptr;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        long long beg;
        int cnt;
        OptimHp hp;
        const int seg = lamb_tile<OP>(a, a.o.tile_begin + t, beg, cnt, hp);
        const float step = group_hp(hp.lr, a.rec[seg * LAMB_REC + 2]);
        float* __restrict__ p = a.o.p + beg;
        const float* __restrict__ m = a.o.m + beg;
        const float* __restrict__ v = a.o.v + beg;
        float* __restrict__ e = EMA ? a.o.ema.e + beg : nullptr;
        bf16_t* __restrict__ pb = shadow ? a.o.pbf + beg : nullptr;
        if (VEC && cnt == GROUP_TILE) {
            float4 pv[GROUP_UNROLL], mv[GROUP_UNROLL], vv[GROUP_UNROLL], ev[GROUP_UNROLL];
#pragma unroll
            for (int k = 0; k < GROUP_UNROLL; k++) {
                const int i = threadIdx.x + k * GROUP_THREADS;
                pv[k] = reinterpret_cast<const float4*>(p)[i];
                mv[k] = reinterpret_cast<const float4*>(m)[i];
                vv[k] = reinterpret_cast<const float4*>(v)[i];
                if (EMA) ev[k] = reinterpret_cast<const float4*>(e)[i];
            }
#pragma unroll
            for (int k = 0; k < GROUP_UNROLL; k++) {
                const int i = threadIdx.x + k * GROUP_THREADS;
                lamb_apply4(pv[k], lamb_direction4(pv[k], mv[k], vv[k], hp), step);
                reinterpret_cast<float4*>(p)[i] = pv[k];
                if (EMA) {
                    ema_blend4(ev[k], pv[k], a.o.ema.d, a.o.ema.omd);
                    reinterpret_cast<float4*>(e)[i] = ev[k];
                }
                if (shadow) reinterpret_cast<uint2*>(pb)[i] = shadow4(pv[k]);
            }
        } else {
            for (int i = threadIdx.x; 4 * i < cnt; i += GROUP_THREADS) {
                float4 pv = lamb_load4<VEC>(p, i, cnt);
                lamb_apply4(pv, lamb_direction4(pv, lamb_load4<VEC>(m, i, cnt), lamb_load4<VEC>(v, i, cnt), hp), step);
                lamb_store4<VEC>(p, i, cnt, pv);
                if (EMA) {
                    float4 ev = lamb_load4<VEC>(e, i, cnt);
                    ema_blend4(ev, pv, a.o.ema.d, a.o.ema.omd);
                    lamb_store4<VEC>(e, i, cnt, ev);
                }
                if (shadow) lamb_store_shadow4<VEC>(pb, i, cnt, pv);
            }
        }
    }
}
// LAMB: pass 1 [OP][CLIP], pass 3 [OP][EMA] (the op has neither clipping nor an EMA)
using LambKernel = void (*)(LambArgs);
const LambKernel kLambMoments[2][2] = {{lamb_moments_tiles_k<false, false>, lamb_moments_tiles_k<true, false>},
                                       {lamb_moments_tiles_k<false, true>, nullptr}};
const LambKernel kLambApply[2][2] = {{lamb_apply_tiles_k<false, false>, lamb_apply_tiles_k<true, false>},
                                     {lamb_apply_tiles_k<false, true>, nullptr}};
}  // namespace

int group_grid(int ntiles) { return ntiles < 2048 ? ntiles : 2048; }

OptimHp adamw_hp(float lr, const vit_adamw_t& hp, int t) {
    const float bc1 = 1.0f - (float)pow((double)hp.beta1, (double)t);
    const float bc2 = 1.0f - (float)pow((double)hp.beta2, (double)t);
    return OptimHp{lr, hp.beta1, hp.beta2, 1.0f - hp.beta1, 1.0f - hp.beta2, bc1, bc2, hp.eps, hp.weight_decay};
}

void optimizer_launch(OptKind kind, const OptimArgs& a, bool tiled, hipStream_t st) {
    const bool adamw = kind == OPT_ADAMW, sgdm = kind == OPT_SGDM, clip = a.rec != nullptr, shadow = a.pbf != nullptr,
               ema = a.ema.e != nullptr;
    char what[48];
    snprintf(what, sizeof what, "%s_%s%s%s%s", adamw ? "adamw" : sgdm ? "sgdm" : "sgd", tiled ? "tiles" : "flat",
             clip ? "_clip" : "", shadow ? "_shadow" : "", ema ? "_ema" : "");
    VIT_REQUIRE(adamw || sgdm || shadow || !ema, "%s: SGD without a bf16 shadow has no fused EMA", what);
    VIT_REQUIRE(!sgdm || a.m, "%s: no momentum buffer", what);
    // (the flat bodies have no scalar tail: arena and chunk extents are multiples of 64 elements)
    VIT_REQUIRE(tiled || (a.n % 4 == 0 && aligned16(a.p) && aligned16(a.g) && aligned16(a.m) && aligned16(a.v) &&
                          aligned16(a.ema.e) && ((uintptr_t)a.pbf & 7) == 0),
                "%s: a flat range must be whole 16-byte aligned float4s (n %lld)", what, a.n);
    if (tiled ? a.ntiles <= 0 : a.n <= 0) return;
    const OptimKernel k = adamw ? kAdamw[tiled][clip][ema] : sgdm ? kSgdm[tiled][clip][ema] : kSgd[tiled][clip][shadow + ema];
    if (tiled)
        k<<<group_grid(a.ntiles), GROUP_THREADS, 0, st>>>(a);
    else
        k<<<grid_for(a.n / 4, 256), 256, 0, st>>>(a);
    after_launch(what);
    if (ema) count_hit(VIT_HIT_EMA);
    if (sgdm) count_hit(VIT_HIT_SGDM);
}

void optimizer_launch(const LambArgs& a, bool tiled, hipStream_t st) {
    const OptimArgs& o = a.o;
    const bool clip = o.rec != nullptr, shadow = o.pbf != nullptr, ema = o.ema.e != nullptr, op = !tiled;
    char what[56];
    snprintf(what, sizeof what, "lamb_%s", tiled ? "tiles" : "flat");
    VIT_REQUIRE(o.p && o.g && o.m && o.v && a.slots && a.rec, "%s: null pointer", what);
    VIT_REQUIRE(tiled ? (a.seg_len && o.gt.tile0 && o.tile_begin == 0 && o.ntiles > 0) : (o.n >= 1 && !clip && !ema),
                "%s: %s", what, tiled ? "not the whole tiled arena" : "a flat range is n >= 1 elements, no clip, no EMA");
    const int ntiles = tiled ? o.ntiles : lamb_tiles(o.n), nseg = tiled ? o.gt.nseg : 1;
    snprintf(what, sizeof what, "lamb_moments_%s%s", tiled ? "tiles" : "flat", clip ? "_clip" : "");
    kLambMoments[op][clip]<<<group_grid(ntiles), GROUP_THREADS, 0, st>>>(a);
    after_launch(what);
    snprintf(what, sizeof what, "lamb_ratio_%s", tiled ? "tiles" : "flat");
    if (tiled)
        lamb_ratio_k<false><<<cdiv(nseg, GROUP_THREADS / 64), GROUP_THREADS, 0, st>>>(a);
    else
        lamb_ratio_k<true><<<1, GROUP_THREADS, 0, st>>>(a);
    after_launch(what);
    snprintf(what, sizeof what, "lamb_apply_%s%s%s", tiled ? "tiles" : "flat", shadow ? "_shadow" : "", ema ? "_ema" : "");
    kLambApply[op][ema]<<<group_grid(ntiles), GROUP_THREADS, 0, st>>>(a);
    after_launch(what);
    if (ema) count_hit(VIT_HIT_EMA);
}
}  // namespace vit

// (include/vit_ops.h) one tensor as one segment through the flat forms of the three LAMB kernels
void lamb_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int t, int flags, float* info) {
    using namespace vit;
    VIT_REQUIRE(n >= 1 && t >= 1 && p && g && m && v, "lamb_step: n %lld, t %d or a null pointer", n, t);
    VIT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && std::isfinite(eps) &&
                    weight_decay >= 0.f && std::isfinite(weight_decay) &&
                    !(flags & ~(VIT_LAMB_ALWAYS_ADAPT | VIT_LAMB_TRUST_CLIP)),
                "lamb_step: beta1 %g, beta2 %g of [0, 1), eps %g, weight_decay %g >= 0 or flags %d", (double)beta1,
                (double)beta2, (double)eps, (double)weight_decay, flags);
    const int ntiles = lamb_tiles(n);
    char* ws = (char*)workspace((size_t)ntiles * sizeof(double2) + 16);
    if (!ws) return;
    LambArgs a{};
    a.o.p = p;
    a.o.g = g;
    a.o.m = m;
    a.o.v = v;
    a.o.n = n;
    a.o.hp = adamw_hp(lr, vit_adamw_t{beta1, beta2, eps, weight_decay}, t);
    a.slots = (double2*)ws;
    a.rec = info ? info : (float*)(ws + (size_t)ntiles * sizeof(double2));
    a.flags = flags;
    optimizer_launch(a, false, stream());
}

// (include/vit_ops.h) torch.optim.SGD's momentum update of one tensor: common.h sgdm_update per element
void sgd_momentum_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening,
                       float weight_decay, int nesterov, int first) {
    using namespace vit;
    VIT_REQUIRE(n >= 0 && (n == 0 || (p && g && buf)), "sgd_momentum_step: n %lld or a null pointer", n);
    VIT_REQUIRE(std::isfinite(lr) && std::isfinite(momentum) && momentum >= 0.f && std::isfinite(dampening) &&
                    std::isfinite(weight_decay) && weight_decay >= 0.f,
                "sgd_momentum_step: lr %g, momentum %g >= 0, dampening %g or weight_decay %g >= 0 is not finite",
                (double)lr, (double)momentum, (double)dampening, (double)weight_decay);
    VIT_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f),
                "sgd_momentum_step: nesterov needs momentum > 0 and dampening 0 (momentum %g, dampening %g)",
                (double)momentum, (double)dampening);
    if (n == 0) return;
    OptimHp hp{};
    hp.lr = lr;
    hp.wd = weight_decay;
    hp.mu = momentum;
    hp.omd = (float)(1.0 - (double)dampening);
    hp.nesterov = nesterov != 0;
    hp.first = first != 0;
    sgdm_scalar_k<<<grid_for(n, 256), 256, 0, stream()>>>(p, g, buf, n, hp);
    after_launch("sgd_momentum_step");
    count_hit(VIT_HIT_SGDM);
}
