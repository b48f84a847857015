// optimizer.h — the optimizer kernels of the trainer behind one parameter block and one launcher
// (optimizer.hip; the matrix of instantiations is in DESIGN.md §16).
#pragma once
#include "../../include/vit_checkpoint.h"  // vit_adamw_t
#include "common.h"

namespace vit {
enum OptKind { OPT_SGD, OPT_ADAMW, OPT_SGDM };

struct OptimHp {
    float lr;
    float b1, b2, omb1, omb2, bc1, bc2, eps;  // AdamW only (common.h adamw_update)
    float wd;                                 // AdamW and momentum SGD
    float mu, omd;                            // momentum SGD only (common.h sgdm_update): momentum, 1 - dampening
    int nesterov, first;                      // ... Nesterov's form; the buffer is seeded by this step
};
// AdamW's / LAMB's hyper-parameters of update t >= 1: 1 - beta and the bias corrections as the oracle rounds
// them (pow in double, the result to fp32, 1.0f - that)
OptimHp adamw_hp(float lr, const vit_adamw_t& hp, int t);
// One optimizer launch.  A flat range is the n elements from p / g / ... (n % 4 == 0, 16-byte aligned
// pointers); a tiled range is the tiles [tile_begin, tile_begin + ntiles) of gt, with p / g / ... the
// arena bases and lr (AdamW, momentum SGD: and wd) multiplied per segment.
struct OptimArgs {
    float* p;
    bf16_t* pbf;         // the bf16 shadow of p; null = none
    const float* g;
    float *m, *v;        // AdamW's moments; momentum SGD: m is the momentum buffer, v unused
    OptimHp hp;
    const ClipRec* rec;  // null = unclipped
    EmaArg ema;          // e null = no EMA
    GroupTab gt;
    int tile_begin, ntiles;
    long long n;
};

// the workgroups of a tiled launch over ntiles tiles (8 per CU, the rest grid-strided)
int group_grid(int ntiles);
// Launches the instantiation for (kind, tiled, a.rec, a.pbf, a.ema.e) on st; an empty range launches
// nothing.  Plain SGD without a shadow has no EMA instantiation (fp32 mode runs ema_update behind the step):
// that combination is an error, as is a flat range that is not whole aligned float4s.  AdamW and momentum
// SGD test the shadow at run time: their EMA instantiations serve fp32 mode too.
void optimizer_launch(OptKind kind, const OptimArgs& a, bool tiled, hipStream_t st);

// LAMB: AdamW's direction u scaled per segment by the trust ratio |w| / |u|, in three
// launches: the moments and the per-tile sums of p^2 and u^2, the ratio per segment, the update.
// Tiled: o is an AdamW tiled range over ALL tiles of o.gt (a ratio needs its whole segment), seg_len[s] the
// segment's own elements (the sums and the update stop there: the padding behind is not touched).
// Flat (the lamb_step op): one segment of o.n elements from o.p / o.g / o.m / o.v, any alignment.
constexpr int LAMB_REC = 3;  // floats per segment record: |w|, |u|, ratio
struct LambArgs {
    OptimArgs o;
    const long long* seg_len;  // [nseg], tiled only
    double2* slots;            // [tiles] {sum p^2, sum u^2} of each tile, by global tile number
    float* rec;                // [nseg * LAMB_REC] (flat: one record)
    int flags;                 // VIT_LAMB_*
};
__host__ __device__ inline int lamb_tiles(long long n) {  // tiles of a flat range
    return (int)((n + GROUP_TILE - 1) / GROUP_TILE);
}
void optimizer_launch(const LambArgs& a, bool tiled, hipStream_t st);
}  // namespace vit
