// trainer.hip — native ViT training step (include/vit_trainer.h).
//
// Host orchestration of the reference's ViT::forward / ViT::backward / optimizer_step
// (/root/reference/train_vit.rs:188-373, 737-743) over the HIP kernels of this library, with
//   * one device arena for params and one for grads, layer-major in REVERSE layer order
//     [head | layer L-1 | ... | layer 0 | embed] so backward finalises one contiguous range per
//     layer; tensors 256-B aligned;
//   * a bf16 shadow of the params (GEMM operands), refreshed by the fused SGD kernel;
//   * data parallelism: one process per GPU, RCCL all-reduce (sum) of each finished gradient
//     chunk on a side stream, ordered by events, overlapped with the rest of backward;
//   * optional per-kernel-class HIP-event timing on the compute stream.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "augment.h"
#include "checkpoint_internal.h"
#include "erase.h"
#include "ops_internal.h"
#include "optimizer.h"
#include "../../include/vit_trainer.h"
#include "../../include/vit_checkpoint.h"
#include "../../include/vit_data.h"
#include "../../include/vit_jpeg.h"

namespace vit {
// jpeg.hip: the JPEG loader's current batch -> device uint8 [B][img][img][3] on st
bool jpeg_loader_decode_to(vit_jpeg_loader_t* l, uint8_t* out, int img, hipStream_t st, const int** labels,
                           int expect_n);
namespace {

enum TIdx {
    P_PATCH_W, P_PATCH_B, P_CLS, P_WPE, P_LN1W, P_LN1B, P_QKVW, P_QKVB, P_ATTPROJW, P_ATTPROJB,
    P_LN2W, P_LN2B, P_FCW, P_FCB, P_FCPROJW, P_FCPROJB, P_LNFW, P_LNFB, P_HEADW, P_HEADB
};

enum TimerClass {
    TC_PATCH, TC_LN_FWD, TC_QKV_FWD, TC_ATTN_FWD, TC_PROJ_FWD, TC_FC_FWD, TC_FCPROJ_FWD, TC_HEAD,
    TC_FCPROJ_DGRAD, TC_FCPROJ_WGRAD, TC_FC_DGRAD, TC_FC_WGRAD, TC_PROJ_DGRAD, TC_PROJ_WGRAD,
    TC_ATTN_BWD, TC_QKV_DGRAD, TC_QKV_WGRAD, TC_LN_BWD, TC_COLSUM, TC_PATCH_BWD, TC_SGD, TC_MISC,
    TC_QUANT, TC_COUNT
};
const char* kTimerNames[TC_COUNT] = {
    "patch_embed_fwd", "layernorm_fwd", "gemm_qkv_fwd", "attention_fwd", "gemm_proj_fwd",
    "gemm_fc_fwd", "gemm_fcproj_fwd", "head", "gemm_fcproj_dgrad", "gemm_fcproj_wgrad",
    "gemm_fc_dgrad", "gemm_fc_wgrad", "gemm_proj_dgrad", "gemm_proj_wgrad", "attention_bwd",
    "gemm_qkv_dgrad", "gemm_qkv_wgrad", "layernorm_bwd", "bias_colsum", "patch_embed_bwd", "sgd",
    "misc", "quantize_mx"};

// out[r][n] = vec[n] for r < rows (the bias start value of a split-K head GEMM)
__global__ void bcast_rows_k(float* __restrict__ out, const float* __restrict__ vec, int rows, int n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long long)rows * n) out[i] = vec[i % n];
}
// the CLS rows of a "bf16 + lo8" [B, T, C] tensor (common.h lo8_*) from fp32 rows in[b][c]
__global__ void rows_to_bf16_k(bf16_t* __restrict__ out, uint8_t* __restrict__ lo, long long ldo,
                               const float* __restrict__ in, int rows, int C) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)rows * C) return;
    const long long b = i / C, o = b * ldo + (i - b * C);
    const bf16_t h = f2bf(in[i]);
    out[o] = h;
    lo[o] = (uint8_t)lo8_encode(in[i], bf2f(h));
}
// ---- stochastic depth
// the per-row scale table [ntab][B*T] from the per-image one [ntab][B] (ntab = 2 L: layer, branch)
__global__ void dp_expand_k(float* __restrict__ rows, const float* __restrict__ img, long long n, int T) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        rows[i] = img[i / T];
}
// the last block's MLP branch gradient from the head's CLS rows in[b][c], image b scaled by rs[b * ld_rs]:
// u = fl32(rs * in) into sf[b][c] (fp32: the fcproj_b column sums) and bf16(u) into the CLS rows of the
// scaled plane out [B, T, C]
__global__ void rows_to_bf16_rs_k(bf16_t* __restrict__ out, long long ldo, float* __restrict__ sf,
                                  const float* __restrict__ in, const float* __restrict__ rs, long long ld_rs,
                                  int rows, int C) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)rows * C) return;
    const long long b = i / C;
    const float u = rs[b * ld_rs] * in[i];
    sf[i] = u;
    out[b * ldo + (i - b * C)] = f2bf(u);
}
// dst [rows][n] += src [rows][lds] (its first n columns)
__global__ void add_cols_k(float* __restrict__ dst, const float* __restrict__ src, int rows, int n, int lds) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (long long)rows * n;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / n;
        dst[i] += src[r * lds + (i - r * n)];
    }
}
// zero the 32-row blocks [(i * T) & ~31, + 32) of x [rows][n] (n % 8 == 0, 16-B aligned rows) for images
// i < B: block (x, i) takes 16-B chunks x, x + gridDim.x, .. of image i's block
__global__ void clear_cls_blocks_k(bf16_t* __restrict__ x, int T, long long rows, int n) {
    const long long r0 = ((long long)blockIdx.y * T) & ~31LL;
    const int cpr = n / 8;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < 32 * cpr; c += gridDim.x * blockDim.x) {
        const long long r = r0 + c / cpr;
        if (r < rows) reinterpret_cast<uint4*>(x + r * n)[c % cpr] = make_uint4(0u, 0u, 0u, 0u);
    }
}
__global__ void fill_k(float* p, float v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
// top-1 of each logits row (first index among equal maxima, as numpy.argmax) and the count of
// rows whose prediction equals the label (eval path).  One wave per row.
__global__ void argmax_rows_k(int* __restrict__ pred, int* __restrict__ correct,
                              const float* __restrict__ logits, const int* __restrict__ labels,
                              int B, int NC) {
    const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (row >= B) return;
    const float* x = logits + (long long)row * NC;
    float best = -INFINITY;
    int bi = NC;  // sentinel above every real index
    for (int j = lane; j < NC; j += 64) {
        const float xv = x[j];
        if (xv > best || bi == NC) { best = xv; bi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi < NC && (bi == NC || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    if (lane == 0) {
        pred[row] = bi;
        if (labels && bi == labels[row]) atomicAdd(correct, 1);
    }
}
// input pipeline: uint8 HWC images -> normalised fp32 CHW pixels, and the
// labels out of the staging buffer.  One thread per pixel: 3 B read, 3 x 4 B written (each channel
// plane coalesced across the wave).  pixel = (x / 255 - mean[c]) / std[c], correctly rounded.
__global__ void normalize_u8_k(float* __restrict__ px, int* __restrict__ lab_out,
                               const unsigned char* __restrict__ u8, const int* __restrict__ lab_in,
                               int B, int HW, float m0, float m1, float m2, float s0, float s1,
                               float s2) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (lab_in && i < B) lab_out[i] = lab_in[i];
    if (i >= (long long)B * HW) return;
    const long long b = i / HW, pix = i - b * HW;
    const unsigned char* src = u8 + i * 3;
    float* dst = px + b * 3 * HW + pix;
    dst[0] = ((float)src[0] / 255.0f - m0) / s0;
    dst[HW] = ((float)src[1] / 255.0f - m1) / s1;
    dst[2 * HW] = ((float)src[2] / 255.0f - m2) / s2;
}
__global__ void to_bf16_k(bf16_t* __restrict__ out, const float* __restrict__ in, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        out[i] = f2bf(in[i]);
}

// Device arena layout (no GPU needed; vit_layout_query exposes it): layer-major in REVERSE layer
// order [head | layer L-1 | ... | layer 0 | embed], each tensor 64-element aligned, so backward
// finalises one contiguous range per layer.  off[ti*L + l] = element offset of tensor ti, layer l
// (unlayered tensors: l = 0); chunk c = [chunk_off[c], chunk_off[c+1]): c = 0 head + final LN,
// 1..L layers L-1..0 (backward's completion order), L+1 embedding.
void compute_layout(int C, int L, int T, int KP, int NC, long long (&canon_size)[20], long long& n_params,
                    std::vector<long long>& off, long long (&chunk_off)[VIT_MAX_LAYERS + 3], int& n_chunks, long long& arena_elems) {
    const long long C_ = C, K = KP;
    const long long sz[20] = {C_ * K, C_, C_, (long long)T * C_,
                              L * C_, L * C_, L * 3 * C_ * C_, L * 3 * C_, L * C_ * C_, L * C_,
                              L * C_, L * C_, L * 4 * C_ * C_, L * 4 * C_, L * C_ * 4 * C_, L * C_,
                              C_, C_, (long long)NC * C_, NC};
    n_params = 0;
    for (int i = 0; i < 20; i++) {
        canon_size[i] = sz[i];
        n_params += sz[i];
    }
    off.assign(20 * L, 0);
    long long cur = 0;
    auto place = [&](int ti, int l, long long n) {
        off[ti * L + l] = cur;
        cur += (n + 63) & ~63LL;
    };
    n_chunks = L + 2;
    chunk_off[0] = 0;
    const int head[4] = {P_HEADW, P_HEADB, P_LNFW, P_LNFB};
    for (int ti : head) place(ti, 0, canon_size[ti]);
    chunk_off[1] = cur;
    for (int c = 1; c <= L; c++) {
        const int l = L - c;
        for (int ti = P_LN1W; ti <= P_FCPROJB; ti++) place(ti, l, canon_size[ti] / L);
        chunk_off[c + 1] = cur;
    }
    const int emb[4] = {P_PATCH_W, P_PATCH_B, P_CLS, P_WPE};
    for (int ti : emb) place(ti, 0, canon_size[ti]);
    chunk_off[L + 2] = cur;
    arena_elems = cur;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

}  // namespace

struct Trainer {
    vit_config_t cfg{};
    int B = 0, T = 0, NP = 0, C = 0, L = 0, NH = 0, NC = 0, KP = 0, prec = 0, device = 0;
    long long BT = 0;
    long long n_params = 0;       // canonical count
    long long arena_elems = 0;    // device arena (with alignment padding)
    long long canon_size[20]{};
    // device offsets: tensor ti, layer l (l=0 for unlayered)
    std::vector<long long> off;   // [20 * L]
    long long chunk_off[VIT_MAX_LAYERS + 3]{};  // chunk c: [chunk_off[c], chunk_off[c+1]) ; c=0 head, 1..L layers L-1..0, L+1 embed
    int n_chunks = 0;

    hipStream_t s = nullptr, s_comm = nullptr;
    // backward weight-gradient stream: the wgrad GEMMs of a layer run beside the dgrad / LN /
    // attention kernels of the main stream (they only read activations and write grads)
    hipStream_t s2 = nullptr;
    bool two_streams = true;
    enum BwdEv { EV_RESA, EV_RESB, EV_DFCH, EV_DQKV, EV_W1, EV_W2, EV_W3, EV_W4, EV_JOIN, EV_SG, EV_PRE_IN, EV_PRE, EV_LC_IN, EV_LC, EV_COUNT };
    hipEvent_t bev[EV_COUNT]{};
    // micro-batches: the batch is processed as NMB row ranges on NMB streams (ms[0] = s), so the
    // kernels of one half (GEMM epilogue bursts, LayerNorm, attention) overlap the other's GEMM
    // main loops; wgrads (on s2) still reduce over the whole batch
    static constexpr int MAXMB = 4;
    int nmb = 1, mb_want = 2;
    int pick_nmb(int want) const {
        if (!two_streams) return 1;
        for (int k = want < MAXMB ? want : MAXMB; k >= 2; k--)
            if (B % k == 0) return k;
        return 1;
    }
    hipStream_t ms[MAXMB]{};
    hipEvent_t mev[MAXMB][EV_COUNT]{};
    hipEvent_t fork_ev = nullptr, join_ev[MAXMB]{};
    std::vector<hipEvent_t> chunk_evm;
    std::vector<hipEvent_t> chunk_ev2;
    std::vector<hipEvent_t> chunk_ev;
    hipEvent_t comm_done = nullptr;

    float* params = nullptr;
    float* grads = nullptr;
    float* gemm_ws = nullptr;     // split-K slabs of the wgrad GEMMs (stream-ordered on s)
    float* attn_part = nullptr;   // per-(b,h) qkv-bias partial sums of the attention backward
    size_t gemm_ws_bytes = 0;
    bf16_t* pbf = nullptr;
    bf16_t* pbfT = nullptr;  // same offsets as pbf; only the four layer weight tensors are used
    float* pixels = nullptr;
    int* labels = nullptr;
    bool has_targets = true;  // false after set_batch without labels: forward only (:264-266)
    // soft targets: label smoothing (a hyper-parameter: persists, not checkpointed)
    // and the mix of the current batch (reset by every set_batch*).  labels_b[r] = labels[B-1-r],
    // allocated by the first mix.  A mix with lam == 1 (an empty cutmix box) changes no pixel and
    // leaves the targets hard, so the head then runs the launches of an unmixed batch.
    float smooth_eps = 0.f;
    bool mixed = false;
    float mix_lam = 1.f;
    int* labels_b = nullptr;
    // random erasing of the current batch (erase.hip; reset with `mixed`): the device list of
    // boxes is allocated by the first erase that has one, the pinned staging by erase::enqueue
    bool erased = false;
    void* erase_list = nullptr;
    erase::Stage erase_stage;
    bool two_labels() const { return mixed && mix_lam != 1.0f; }
    bool soft_targets() const { return smooth_eps > 0.f || two_labels(); }
    int* preds = nullptr;     // eval: [B] top-1 + one counter
    // uint8 upload: double-buffered device staging filled on s_copy, normalised on s
    hipStream_t s_copy = nullptr;
    unsigned char* u8_stage[2]{};
    int* lab_stage[2]{};
    hipEvent_t u8_copied[2]{}, u8_used[2]{};
    int u8_k = 0;
    // one-shot RandAugment plan for the next set_batch_u8 (augment.hip)
    aug::Prepared aug_plan;
    bool aug_pending = false;
    void* aug_scratch = nullptr;
    // stochastic depth (vit_trainer_set_drop_path): a one-shot table s[l][br][b] of scales for
    // the residual branches (br 0 = attention, 1 = MLP) of the next training forward and its backward.
    // dp_pending: set and not yet consumed; dp_fwd: the running forward applies dp_rows; dp_bwd: the last
    // training forward did (its backward follows it; an eval in between leaves it); dp_used: that table.
    // Device: dp_img [L][2][B] (uploaded by the setter), dp_rows [L][2][B*T] (expanded when consumed: the
    // GEMM epilogues and LayerNorm backwards read one scale per row), and in bf16 mode the two scaled bf16
    // planes dres_s / dres_s2 beside dres_bf / dres_bf2 and dcls_xs [B][C], the head's scaled CLS rows.
    // All allocated on first use.  The setter copies the host table into one of two pinned staging buffers
    // and enqueues the upload on s, so it neither waits for the steps in flight nor keeps the caller's
    // array; a staging buffer is rewritten only after the upload that read it (two tables ago) has run.
    std::vector<float> dp_pending, dp_used;
    float* dp_stage[2]{};
    hipEvent_t dp_staged[2]{};
    int dp_k = 0;
    bool dp_has_pending = false, dp_fwd = false, dp_bwd = false, dp_last_used = false;
    float *dp_img = nullptr, *dp_rows = nullptr, *dcls_xs = nullptr;
    bf16_t *dres_s = nullptr, *dres_s2 = nullptr;
    const float* dp_scale(int l, int br, long long r0) const { return dp_rows + ((long long)(l * 2 + br)) * BT + r0; }
    bool dp_alloc() {
        if (dp_img) return true;
        float* a = alloc<float>((long long)L * 2 * B);
        float* b = alloc<float>((long long)L * 2 * BT);
        bool ok = a && b;
        if (ok && lowp()) {
            dres_s = alloc<bf16_t>(BT * C);
            dres_s2 = alloc<bf16_t>(BT * C);
            dcls_xs = alloc<float>((long long)B * C);
            ok = dres_s && dres_s2 && dcls_xs;
        }
        for (int k = 0; k < 2 && ok; k++) {
            ok = hipHostMalloc((void**)&dp_stage[k], (size_t)L * 2 * B * sizeof(float), hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&dp_staged[k], hipEventDisableTiming) == hipSuccess;
            if (!ok) set_error("trainer: drop-path staging buffers");
        }
        if (!ok) return false;
        dp_rows = b;
        dp_img = a;
        return true;
    }
    bool set_drop_path(const float* host) {
        if (fp8()) {
            set_error("vit_trainer_set_drop_path: not supported in fp8 mode");
            return false;
        }
        if (!host) {
            dp_has_pending = false;
            return true;
        }
        const size_t n = (size_t)L * 2 * B;
        for (size_t i = 0; i < n; i++)
            if (!(std::isfinite(host[i]) && host[i] >= 0.f)) {
                set_error("vit_trainer_set_drop_path: layer %d branch %d image %d: scale %g is not finite and >= 0",
                          (int)(i / (2 * (size_t)B)), (int)(i / B % 2), (int)(i % B), (double)host[i]);
                return false;
            }
        if (!dp_alloc()) return false;
        dp_pending.assign(host, host + n);
        // the upload runs on the trainer's stream, behind the steps in flight (only the expand kernel of the
        // next training forward, on s too, reads dp_img), from the pinned copy: the caller's array has been
        // read when this returns
        const int k = dp_k++ & 1;
        VIT_HIP(hipEventSynchronize(dp_staged[k]));  // (never recorded: returns at once)
        memcpy(dp_stage[k], host, n * sizeof(float));
        VIT_HIP(hipMemcpyAsync(dp_img, dp_stage[k], n * sizeof(float), hipMemcpyHostToDevice, s));
        VIT_HIP(hipEventRecord(dp_staged[k], s));
        if (has_error()) return false;
        dp_has_pending = true;
        return true;
    }
    // at the start of a forward: a training forward (a batch with labels, not eval) consumes the pending table
    void dp_begin(bool training) {
        dp_fwd = false;
        if (!training) return;
        dp_fwd = dp_bwd = dp_last_used = dp_has_pending;
        if (!dp_fwd) return;
        dp_has_pending = false;
        dp_used = dp_pending;
        // every stream of the previous backward has joined s, so nothing still reads dp_rows
        const long long n = (long long)L * 2 * BT;
        dp_expand_k<<<grid_for(n, 256), 256, 0, s>>>(dp_rows, dp_img, n, T);
        after_launch("drop_path_expand");
    }
    // AdamW state (allocated on the first AdamW step / a checkpoint load with optimizer state)
    float *adam_m = nullptr, *adam_v = nullptr;
    int adam_t = 0;
    vit_adamw_t adam_hp{};
    std::vector<DevBuf> allocs;
    size_t dev_bytes = 0;
    int b_global = 0;

    // ---- bf16 activations
    struct LayerActs {
        bf16_t *ln1, *qkv, *atty, *ln2, *fchd, *fchg;  // fchd = gelu'(fc pre-activation), fchg = gelu(.)
        float *ln1_mean, *ln1_rstd, *lse, *res2, *ln2_mean, *ln2_rstd, *res3;
        // fp32-mode extras
        float *ln1f, *qkvf, *attyf, *preatt, *att, *attproj, *ln2f, *fchf, *fchgf, *fcproj;
    };
    std::vector<LayerActs> la;
    float* encoded = nullptr;
    // bf16 / fp8 mode, KP % 8 != 0 (ViT-H/14: 588): the patch GEMMs run on the bf16 engine over
    // KPP = KP rounded up to 64 columns: zero-padded im2col rows, a zero-padded bf16 weight copy
    // (refreshed with the transposed copies) and a padded fp32 weight-gradient scratch whose first
    // KP columns are added to the gradient arena
    bool patch_pad = false;
    int KPP = 0;
    bf16_t* wpatch_pad = nullptr;
    float* dwpatch_pad = nullptr;
    bf16_t* patches_bf = nullptr;
    float* patches_f = nullptr;
    float* emb_tmp = nullptr;
    float *cls_x = nullptr, *lnf = nullptr, *lnf_mean = nullptr, *lnf_rstd = nullptr;
    float *logits = nullptr, *probs = nullptr, *losses = nullptr;
    // grads scratch
    float *dlosses = nullptr, *dlogits = nullptr, *dlnf = nullptr, *dcls_x = nullptr;
    float *dres_a = nullptr, *dres_b = nullptr, *dln = nullptr;
    float* pos_sums = nullptr;  // [T][C] per-position column sums of the patch-embedding backward
    float* psg_part = nullptr;  // [PSG_CHUNKS][T][C] per-image-chunk partial sums of the same
    uint8_t *dres_lo = nullptr, *dres_lo2 = nullptr;  // lo8 planes of the bf16 residual-gradient stream
    // deterministic small gradients (no float atomics): stream-s scratch for the fixed-order column
    // sums of the head / fp32 path, and in bf16 / fp8 mode the per-layer partial rows of the
    // micro-batches' LayerNorm (dw | db | next bias), fc-bias and qkv-bias sums, double-buffered by
    // layer parity and reduced once per layer on the weight-gradient stream (sg_finalize)
    float* red_ws = nullptr;
    float* sg_part[2]{};
    long long sg_ln2 = 0, sg_ln1 = 0, sg_fcb = 0, sg_qkv = 0;  // offsets (floats) in sg_part[p]
    bf16_t* dln_bf = nullptr;  // bf16 mode: LN-output gradient from the fc / qkv dgrad GEMMs
    bf16_t *dres_bf = nullptr, *dres_bf2 = nullptr, *dfch = nullptr, *datty = nullptr, *dqkv = nullptr, *dpatch_bf = nullptr;
    float* dpatch_f = nullptr;
    // fp32-mode per-layer grad scratch (one layer, zeroed per layer)
    float *g_block = nullptr;
    long long g_block_elems = 0;
    float *g_dres2, *g_dfcproj, *g_dfchg, *g_dfch, *g_dln2, *g_dattproj, *g_datty, *g_dpreatt,
        *g_datt, *g_dqkv, *g_dln1;

    // ---- DP
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, overlap = 1;
    // option "dp_probe": each chunk is also copied, on s_comm right after its all-reduce, into this
    // snapshot arena (same layout as grads): snapshot == final grads bitwise proves every chunk
    // was final when the comm stream reduced it (at world 1 the sum itself is an identity)
    float* dp_snap = nullptr;
    bool dp_probe_on = false;

    // ---- timing
    bool timing = false;
    struct Rec { int cls; hipEvent_t a, b; hipStream_t st; };
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<Rec> recs;
    double t_ms[TC_COUNT]{};
    long long t_calls[TC_COUNT]{};
    double t_flops[TC_COUNT]{};

    // ------------------------------------------------------------------------------
    template <typename TT>
    TT* alloc(long long elems) {
        size_t bytes = (size_t)std::max<long long>(elems, 1) * sizeof(TT);
        bytes = (bytes + 255) & ~(size_t)255;
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            set_error("trainer: hipMalloc(%zu) failed", bytes);
            return nullptr;
        }
        allocs.push_back({p, bytes});
        dev_bytes += bytes;
        return (TT*)p;
    }

    bool layered(int ti) const { return ti >= P_LN1W && ti <= P_FCPROJB; }
    bool lowp() const { return prec != VIT_FP32; }  // bf16 or fp8 mode (the fast path)
    bool fp8() const { return prec == VIT_FP8; }
    // the four layer-weight kinds (every mode): tensor index and the forward view N x K of one layer
    static constexpr int NWK = 4;
    struct WKind { int ti; long long N, K; };
    WKind wkind(int k) const {
        const WKind t[NWK] = {{P_QKVW, 3LL * C, C}, {P_ATTPROJW, C, C}, {P_FCW, 4LL * C, C}, {P_FCPROJW, C, 4LL * C}};
        return t[k];
    }
    // the L layers of kind k lie a constant stride apart in the arenas, in reverse layer order: the
    // lowest-addressed layer l0 (what a batched launch over all layers is given) and the stride's magnitude
    struct WSpan { int l0; long long stride; };
    WSpan wspan(int k) const {
        const int ti = wkind(k).ti;
        const long long st = L > 1 ? off[ti * L + 1] - off[ti * L] : 0;
        return {st < 0 ? L - 1 : 0, st < 0 ? -st : st};
    }
    // ---- fp8 mode: MXFP8 copies of the four layer weights (forward B operand, [N][K]) and of their
    // transposes (input-gradient B operand, [Cin][OC]), refreshed after every optimizer step, and
    // per-micro-batch scratch for the quantized A operand of each fp8 GEMM
    struct QMat { uint8_t* q = nullptr; uint8_t* s = nullptr; };
    QMat wq[NWK], wtq[NWK];            // [L] matrices each, in the source's memory order
    uint8_t* act_q[4]{};
    uint8_t* act_s[4]{};
    // fused MX outputs (fp8 mode): the GELU output of fc fwd / the GELU' output of fcproj dgrad,
    // written by those GEMMs' epilogues and read as the next GEMM's A operand (VIT_FP8_FUSE=0
    // quantizes them in separate passes instead, for A/B)
    uint8_t* act_q2[4]{};
    uint8_t* act_s2[4]{};
    bool fuse_mx = true;
    // fp8 weight gradients: dout and inp quantized column-wise
    // (MX blocks of 32 consecutive tokens: the axis the weight gradient reduces over) into [OC][Kp] /
    // [Cin][Kp] e4m3 rows on the weight-gradient stream, then the MXFP8 engine with K-split slabs
    bool wt_cols = true;  // fp8: the dgrads' MX weight copy by column-quantizing W (VIT_FP8_WT_COLS=0: transpose + rows)
    QMat wg_a, wg_b;  // column-quantized dout / inp of the running weight gradient (stream-ordered)
    // fused row+column quantization (quantize_mx_rowcol_bf16): the column forms of ln1, atty, ln2
    // per layer (written by the forward GEMMs' quantize step, read by the backward's weight
    // gradients) and of dres3, dres2, dqkv (written by the input-gradient GEMMs' quantize step on
    // the micro-batch streams, read by the next weight gradient on s2; the waits that already
    // order dres / dqkv reuse order these too)
    bool rowcol_ok = false;
    long long kp_tok = 0;  // mx_cols_kp(B*T)
    QMat actc[3], dcol[3];
    // ... and of the 4C-wide GELU output (fc fwd epilogue, per layer) and its gradient dfch (fcproj
    // dgrad epilogue): with those and the row forms fused too (fuse_mx), neither bf16 tensor is
    // stored (GemmArgs::mxc_q; nothing else reads them in fp8 mode)
    QMat fchgc, dfchc;
    bool rowcol_on() const { return fp8() && rowcol_ok && ((long long)(B / nmb) * T) % 64 == 0; }
    bool epicol_on() const { return rowcol_on() && fuse_mx && (4 * C) % 64 == 0; }
    // fp8: LayerNorm forward straight into the MX forms (ln_forward_mx; else bf16 + rowcol), in whole
    // tiles: a leftover-row path for the last partial round measured 119.70 vs 119.47 ms/step without it
    // at ViT-H/14 (the other micro-batch stream already fills the partial round)
    bool lnmx_on() const { return rowcol_on() && ln_forward_mx_supported(C); }
    // fp8: the residual-gradient LayerNorm backwards also write both MX forms of dres2 / dres3
    // (ln_backward_stream's MX form; else the rowcol quantize)
    uint8_t* lnb_scr[4]{};  // per micro-batch stream: the LayerNorm backward -> MX kernel's scratch
    bool lnbmx_on() const { return rowcol_on() && ln_backward_mx_supported(C); }
    // the column-form span of micro-batch mb (R rows): the last one carries the padding tokens
    long long mb_ntok(int mb, long long R) const { return mb == nmb - 1 ? kp_tok - (long long)mb * R : R; }
    QMat fchgc_of(int l) const {
        return {fchgc.q + (long long)l * 4 * C * kp_tok, fchgc.s + (long long)l * mx_scale_bytes(4LL * C, (int)kp_tok)};
    }
    QMat actc_of(int k, int l) const {
        return {actc[k].q + (long long)l * C * kp_tok, actc[k].s + (long long)l * mx_scale_bytes(C, (int)kp_tok)};
    }
    int wslot(int k, int l) const { return std::abs(l - wspan(k).l0); }  // memory-order index of layer l's copy of kind k
    int wkind_of(int ti) const {
        for (int k = 0; k < NWK; k++) if (wkind(k).ti == ti) return k;
        return -1;
    }
    long long per_layer(int ti) const { return canon_size[ti] / L; }
    float* P(int ti, int l = 0) const { return params + off[ti * L + l]; }
    float* G(int ti, int l = 0) const { return grads + off[ti * L + l]; }
    bf16_t* W(int ti, int l = 0) const { return pbf + off[ti * L + l]; }
    // transposed bf16 copy of a layer weight ([Cin][OC]): the dgrad GEMMs read it K-contiguous
    bf16_t* WT(int ti, int l = 0) const { return pbfT + off[ti * L + l]; }
    // dgrad B operand: the transposed copy (K-contiguous, ldb = OC)
    void dgrad_b(GemmArgs& g, int ti, int l, int OC) const { g.B = WT(ti, l); g.ldb = OC; g.b_kcontig = true; }

    void build_layout() {
        compute_layout(C, L, T, KP, NC, canon_size, n_params, off, chunk_off, n_chunks, arena_elems);
    }

    // canonical <-> device copies (host staging)
    void canon_to_device(const float* host, float* dev) {
        pre_side_wait();  // (the arena clear / transposes on s2 must not race this copy)
        std::vector<float> stage((size_t)arena_elems, 0.f);
        long long c = 0;
        for (int ti = 0; ti < 20; ti++) {
            if (layered(ti)) {
                const long long n = per_layer(ti);
                for (int l = 0; l < L; l++, c += n) memcpy(&stage[off[ti * L + l]], host + c, n * 4);
            } else {
                memcpy(&stage[off[ti * L]], host + c, canon_size[ti] * 4);
                c += canon_size[ti];
            }
        }
        VIT_HIP(hipMemcpyAsync(dev, stage.data(), arena_elems * 4, hipMemcpyHostToDevice, s));
        VIT_HIP(hipStreamSynchronize(s));
    }
    void device_to_canon(const float* dev, float* host) {
        pre_side_wait();
        std::vector<float> stage((size_t)arena_elems);
        VIT_HIP(hipMemcpyAsync(stage.data(), dev, arena_elems * 4, hipMemcpyDeviceToHost, s));
        VIT_HIP(hipStreamSynchronize(s));
        long long c = 0;
        for (int ti = 0; ti < 20; ti++) {
            if (layered(ti)) {
                const long long n = per_layer(ti);
                for (int l = 0; l < L; l++, c += n) memcpy(host + c, &stage[off[ti * L + l]], n * 4);
            } else {
                memcpy(host + c, &stage[off[ti * L]], canon_size[ti] * 4);
                c += canon_size[ti];
            }
        }
    }

    // ---- timing helpers
    void tbeg(int cls, double flops, hipStream_t st = nullptr) {
        if (!timing) return;
        if (!st) st = s;
        if (ev_used + 2 > ev_pool.size()) {
            for (int k = 0; k < 64; k++) {
                hipEvent_t e;
                VIT_HIP(hipEventCreate(&e));
                ev_pool.push_back(e);
            }
        }
        Rec r{cls, ev_pool[ev_used], ev_pool[ev_used + 1], st};
        ev_used += 2;
        VIT_HIP(hipEventRecord(r.a, st));
        recs.push_back(r);
        t_flops[cls] += flops;
    }
    void tend() {
        if (!timing) return;
        VIT_HIP(hipEventRecord(recs.back().b, recs.back().st));
    }
    void collect() {
        if (recs.empty()) return;
        VIT_HIP(hipStreamSynchronize(s));
        VIT_HIP(hipStreamSynchronize(s2));
        for (int k = 1; k < MAXMB; k++) VIT_HIP(hipStreamSynchronize(ms[k]));
        for (auto& r : recs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                t_ms[r.cls] += ms;
                t_calls[r.cls] += 1;
            }
        }
        recs.clear();
        ev_used = 0;
    }

    void gemm(int cls, GemmArgs a, bool bf, hipStream_t st = nullptr) {
        if (!st) st = s;
        tbeg(cls, 2.0 * a.M * (double)a.N * a.K, st);
        if (bf) gemm_bf16(a, st); else gemm_f32(a, st);
        tend();
    }
    // cross-stream ordering: what is enqueued on `to` from here on runs after everything enqueued on `from` so far
    void order(hipEvent_t ev, hipStream_t from, hipStream_t to) {
        VIT_HIP(hipEventRecord(ev, from));
        VIT_HIP(hipStreamWaitEvent(to, ev, 0));
    }
    // fork the micro-batch streams off s (one record, a wait on each) / join them back into s
    void mb_fork() {
        if (nmb < 2) return;
        VIT_HIP(hipEventRecord(fork_ev, s));
        for (int k = 1; k < nmb; k++) VIT_HIP(hipStreamWaitEvent(ms[k], fork_ev, 0));
    }
    void mb_join() {
        for (int k = 1; k < nmb; k++) order(join_ev[k], ms[k], s);
    }

    // ------------------------------------------------------------------------------
    bool init(const vit_config_t* c, int batch, int precision, int dev) {
        cfg = *c;
        B = batch;
        C = c->channels; L = c->num_layers; NH = c->num_heads; NC = c->num_classes;
        NP = (c->img / c->patch) * (c->img / c->patch);
        T = NP + 1;
        KP = 3 * c->patch * c->patch;
        BT = (long long)B * T;
        prec = precision;
        device = dev;
        if (c->in_ch != 3 || C % NH || L < 1 || L > VIT_MAX_LAYERS || B < 1 || prec < VIT_FP32 || prec > VIT_FP8) {
            set_error("trainer: unsupported config");
            return false;
        }
        if (prec == VIT_FP8 && C % 64) {
            set_error("trainer: fp8 mode needs C %% 64 == 0 (MX k-steps of 64), C=%d", C);
            return false;
        }
        if (hipSetDevice(dev) != hipSuccess) { set_error("trainer: hipSetDevice(%d)", dev); return false; }
        // stream priorities: bf16 mode runs the weight-gradient stream high and the micro-batch streams
        // low, fp8 mode all equal.  Measured (bench.py, three interleaved rounds each,
        // profiles/r06_stream_prio.txt): ViT-B/16 bf16 wgrad-high vs equal: 7102-7106 vs 7059-7062 img/s
        // (+0.65 %), micro-batch-high: -0.2 %; ViT-H/14 fp8 wgrad-high vs equal: 1088 vs 1098 img/s
        // (-0.8 %), micro-batch-high: -2 % (which stream's kernels fill the others' partial rounds)
        const bool prio = prec == VIT_BF16;
        int p_lo = 0, p_hi = 0;
        if (prio) VIT_HIP(hipDeviceGetStreamPriorityRange(&p_lo, &p_hi));
        auto mk_stream = [&](hipStream_t* st, bool wgrad) {
            if (!prio) VIT_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
            else VIT_HIP(hipStreamCreateWithPriority(st, hipStreamNonBlocking, wgrad ? p_hi : p_lo));
        };
        mk_stream(&s, false);
        VIT_HIP(hipStreamCreateWithFlags(&s_comm, hipStreamNonBlocking));
        mk_stream(&s2, true);
        for (auto& e : bev) VIT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ms[0] = s;
        for (int k = 1; k < MAXMB; k++) mk_stream(&ms[k], false);
        for (auto& row : mev)
            for (auto& e : row) VIT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        VIT_HIP(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        for (auto& e : join_ev) VIT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        {
            const char* e = getenv("VIT_MICROBATCH");
            mb_want = e ? atoi(e) : 2;
            nmb = pick_nmb(mb_want);
        }
        chunk_evm.resize((size_t)(L + 2) * MAXMB);
        for (auto& e : chunk_evm) VIT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        chunk_ev.resize(L + 2);
        for (auto& e : chunk_ev) VIT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        chunk_ev2.resize(L + 2);
        for (auto& e : chunk_ev2) VIT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        VIT_HIP(hipEventCreateWithFlags(&comm_done, hipEventDisableTiming));
        build_layout();
        params = alloc<float>(arena_elems);
        grads = alloc<float>(arena_elems);
        pixels = alloc<float>((long long)B * 3 * c->img * c->img);
        labels = alloc<int>(B);
        preds = alloc<int>(B + 1);
        encoded = alloc<float>(BT * C);
        cls_x = alloc<float>((long long)B * C);
        lnf = alloc<float>((long long)B * C);
        lnf_mean = alloc<float>(B);
        lnf_rstd = alloc<float>(B);
        logits = alloc<float>((long long)B * NC);
        probs = alloc<float>((long long)B * NC);
        losses = alloc<float>(B);
        dlosses = alloc<float>(B);
        dlogits = alloc<float>((long long)B * NC);
        dlnf = alloc<float>((long long)B * C);
        dcls_x = alloc<float>((long long)B * C);
        if (!lowp()) {  // the bf16 / fp8 residual-gradient stream is bf16 (dres_bf / dres_bf2)
            dres_a = alloc<float>(BT * C);
            dres_b = alloc<float>(BT * C);
        }
        pos_sums = alloc<float>((long long)T * C);
        if (lowp()) psg_part = alloc<float>((long long)PSG_CHUNKS * T * C);
        {  // column-sum / LayerNorm partial rows on s (head, fp32 path)
            const long long a1 = (long long)ln_bwd_blocks(BT) * 2 * C;
            const long long a2 = (long long)cdiv(BT, 256) * std::max(4 * C, NC);
            red_ws = alloc<float>(std::max(a1, a2));
        }
        emb_tmp = alloc<float>((long long)B * NP * C);
        la.resize(L);
        if (!lowp()) {  // the fp32 engine's split-K slabs (<= ~16 MB: splits x tiles <= 1024 tiles of 64 x 64)
            gemm_ws_bytes = (size_t)32 << 20;
            gemm_ws = alloc<float>((long long)(gemm_ws_bytes / sizeof(float)));
        }
        if (lowp()) {
            if (!(attn_fused_supported(T, C, NH) || attn_generic_supported(T, C, NH)) || C % 8) {
                set_error("trainer: bf16 / fp8 path needs head size 32, 64, 80, 96 or 128 and C %% 8 == 0 (T=%d C=%d NH=%d)", T, C, NH);
                return false;
            }
            // a patch whose im2col row (3*P*P) is not a multiple of 8 bf16 (ViT-H/14: 588) cannot
            // feed the bf16 GEMM's 16-B loads as it is: padded to KPP columns (the fp32 GEMM from
            // the fp32 master weights, the earlier form, cost 3 ms/step at H/14)
            patch_pad = KP % 8 != 0;
            KPP = patch_pad ? (KP + 63) / 64 * 64 : KP;
            pbf = alloc<bf16_t>(arena_elems);
            pbfT = alloc<bf16_t>(arena_elems);
            patches_bf = alloc<bf16_t>((long long)B * NP * KPP);
            if (patch_pad) {
                wpatch_pad = alloc<bf16_t>((long long)C * KPP);
                dwpatch_pad = alloc<float>((long long)C * KPP);
                if (wpatch_pad) VIT_HIP(hipMemset(wpatch_pad, 0, (size_t)C * KPP * 2));
            }
            for (int l = 0; l < L; l++) {
                LayerActs& a = la[l];
                a.ln1 = alloc<bf16_t>(BT * C);
                a.ln1_mean = alloc<float>(BT);
                a.ln1_rstd = alloc<float>(BT);
                a.qkv = alloc<bf16_t>(BT * 3 * C);
                a.atty = alloc<bf16_t>(BT * C);
                a.lse = alloc<float>(BT * NH);
                a.res2 = alloc<float>(BT * C);
                a.ln2 = alloc<bf16_t>(BT * C);
                a.ln2_mean = alloc<float>(BT);
                a.ln2_rstd = alloc<float>(BT);
                a.fchd = alloc<bf16_t>(BT * 4 * C);
                a.fchg = alloc<bf16_t>(BT * 4 * C);
                a.res3 = alloc<float>(BT * C);
            }
            if (prec == VIT_BF16 && !has_error()) {
                // last_cls: with the option on, the last block's forward writes only the CLS
                // rows of these, while its full-size weight gradients, fcproj dgrad epilogue and LayerNorm 2
                // backward still read every row of them against gradient rows that are exact zeros.  Cleared
                // once here, so those products are 0 x finite (zeros, or rows an earlier last_cls=0 step
                // left), never 0 x NaN from uninitialised memory: this is what makes the full-size weight
                // gradients safe.
                LayerActs& a = la[L - 1];
                VIT_HIP(hipMemsetAsync(a.ln2_mean, 0, (size_t)BT * 4, s));
                VIT_HIP(hipMemsetAsync(a.ln2_rstd, 0, (size_t)BT * 4, s));
                VIT_HIP(hipMemsetAsync(a.res2, 0, (size_t)BT * C * 4, s));
                VIT_HIP(hipMemsetAsync(a.ln2, 0, (size_t)BT * C * 2, s));
                VIT_HIP(hipMemsetAsync(a.fchd, 0, (size_t)BT * 4 * C * 2, s));
                VIT_HIP(hipMemsetAsync(a.fchg, 0, (size_t)BT * 4 * C * 2, s));
            }
            dln_bf = alloc<bf16_t>(BT * C);
            dres_bf = alloc<bf16_t>(BT * C);
            dres_bf2 = alloc<bf16_t>(BT * C);
            dres_lo = alloc<uint8_t>(BT * C);
            dres_lo2 = alloc<uint8_t>(BT * C);
            dfch = alloc<bf16_t>(BT * 4 * C);
            datty = alloc<bf16_t>(BT * C);
            dqkv = alloc<bf16_t>(BT * 3 * C);
            dpatch_bf = alloc<bf16_t>((long long)B * NP * C);
            // slabs: <= 32 splits of the largest weight gradient (4C x C)
            gemm_ws_bytes = (size_t)32 * 4 * C * (size_t)std::max(C, KP) * sizeof(float);
            gemm_ws = alloc<float>((long long)(gemm_ws_bytes / sizeof(float)));
            attn_part = alloc<float>((long long)attn_backward_ws_floats(B, T, C, NH) + MAXMB * 3LL * C);  // bias partials | delta
            {  // per-layer small-gradient partial rows for up to MAXMB micro-batches
                const long long lnr = (long long)MAXMB * ln_bwd_blocks(BT), fcr = cdiv(BT, 96) + MAXMB;  // (96: ping-pong engine)
                sg_ln2 = 0;
                sg_ln1 = sg_ln2 + lnr * 3 * C;
                sg_fcb = sg_ln1 + lnr * 3 * C;
                sg_qkv = sg_fcb + fcr * 4 * C;
                const long long n = sg_qkv + (long long)MAXMB * 3 * C;
                sg_part[0] = alloc<float>(n);
                sg_part[1] = alloc<float>(n);
            }
            if (fp8()) {
                for (int k = 0; k < NWK; k++) {
                    const WKind w = wkind(k);
                    wq[k].q = alloc<uint8_t>(L * w.N * w.K);
                    wq[k].s = alloc<uint8_t>((long long)L * mx_scale_bytes(w.N, (int)w.K));
                    wtq[k].q = alloc<uint8_t>(L * w.N * w.K);
                    wtq[k].s = alloc<uint8_t>((long long)L * mx_scale_bytes(w.K, (int)w.N));
                }
                // A-operand scratch per micro-batch stream: rows x (widest K = 4C) bytes + scales.
                // Stream k runs only when there are > k micro-batches, so it holds at most
                // B/(k+1) images' rows.
                for (int k = 0; k < MAXMB; k++) {
                    const long long rows = (long long)(B / (k + 1)) * T;
                    if (rows <= 0) continue;
                    act_q[k] = alloc<uint8_t>(rows * 4 * C);
                    act_s[k] = alloc<uint8_t>((long long)mx_scale_bytes(rows, 4 * C));
                    act_q2[k] = alloc<uint8_t>(rows * 4 * C);
                    act_s2[k] = alloc<uint8_t>((long long)mx_scale_bytes(rows, 4 * C));
                    // the padding rows' scales (never written by the fused epilogues) stay 0
                    VIT_HIP(hipMemset(act_s2[k], 0, mx_scale_bytes(rows, 4 * C)));
                }
                const char* fe = getenv("VIT_FP8_FUSE");
                fuse_mx = !(fe && fe[0] == '0');
                const char* wc = getenv("VIT_FP8_WT_COLS");
                wt_cols = !(wc && wc[0] == '0') && C % 64 == 0;
                const long long kp = mx_cols_kp(BT);
                wg_a.q = alloc<uint8_t>(4LL * C * kp);
                wg_a.s = alloc<uint8_t>((long long)mx_scale_bytes(4LL * C, (int)kp));
                wg_b.q = alloc<uint8_t>(4LL * C * kp);
                wg_b.s = alloc<uint8_t>((long long)mx_scale_bytes(4LL * C, (int)kp));
                const char* rc = getenv("VIT_FP8_ROWCOL");
                rowcol_ok = !(rc && rc[0] == '0');
                kp_tok = kp;
                if (rowcol_ok) {
                    for (int k = 0; k < 3; k++) {
                        actc[k].q = alloc<uint8_t>((long long)L * C * kp);
                        actc[k].s = alloc<uint8_t>((long long)L * mx_scale_bytes(C, (int)kp));
                        const long long w = k == 2 ? 3LL * C : C;
                        dcol[k].q = alloc<uint8_t>(w * kp);
                        dcol[k].s = alloc<uint8_t>((long long)mx_scale_bytes(w, (int)kp));
                    }
                    fchgc.q = alloc<uint8_t>((long long)L * 4 * C * kp);
                    fchgc.s = alloc<uint8_t>((long long)L * mx_scale_bytes(4LL * C, (int)kp));
                    dfchc.q = alloc<uint8_t>(4LL * C * kp);
                    dfchc.s = alloc<uint8_t>((long long)mx_scale_bytes(4LL * C, (int)kp));
                    if (ln_backward_mx_supported(C))
                        for (int k = 0; k < MAXMB; k++) lnb_scr[k] = alloc<uint8_t>((long long)ln_backward_mx_scratch_bytes(C));
                }
            }
        } else {
            patches_f = alloc<float>((long long)B * NP * KP);
            dpatch_f = alloc<float>((long long)B * NP * C);
            const long long att_n = BT * NH * T;
            for (int l = 0; l < L; l++) {
                LayerActs& a = la[l];
                a.ln1f = alloc<float>(BT * C);
                a.ln1_mean = alloc<float>(BT);
                a.ln1_rstd = alloc<float>(BT);
                a.qkvf = alloc<float>(BT * 3 * C);
                a.attyf = alloc<float>(BT * C);
                a.preatt = alloc<float>(att_n);
                a.att = alloc<float>(att_n);
                a.attproj = alloc<float>(BT * C);
                a.res2 = alloc<float>(BT * C);
                a.ln2f = alloc<float>(BT * C);
                a.ln2_mean = alloc<float>(BT);
                a.ln2_rstd = alloc<float>(BT);
                a.fchf = alloc<float>(BT * 4 * C);
                a.fchgf = alloc<float>(BT * 4 * C);
                a.fcproj = alloc<float>(BT * C);
                a.res3 = alloc<float>(BT * C);
            }
            // one layer of reference grads_acts (train_vit.rs:346-357), zeroed per layer
            const long long sizes[11] = {BT * C, BT * C, BT * 4 * C, BT * 4 * C, BT * C, BT * C,
                                         BT * C, att_n, att_n, BT * 3 * C, BT * C};
            float** slots[11] = {&g_dres2, &g_dfcproj, &g_dfchg, &g_dfch, &g_dln2, &g_dattproj,
                                 &g_datty, &g_dpreatt, &g_datt, &g_dqkv, &g_dln1};
            g_block_elems = 0;
            for (int k = 0; k < 11; k++) g_block_elems += (sizes[k] + 63) & ~63LL;
            g_block = alloc<float>(g_block_elems);
            long long o = 0;
            for (int k = 0; k < 11; k++) {
                *slots[k] = g_block ? g_block + o : nullptr;
                o += (sizes[k] + 63) & ~63LL;
            }
        }
        VIT_HIP(hipMemsetAsync(grads, 0, arena_elems * 4, s));
        VIT_HIP(hipStreamSynchronize(s));
        return !has_error();
    }

    void destroy() {
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        for (int k = 0; k < 2; k++) {
            if (u8_copied[k]) (void)hipEventDestroy(u8_copied[k]);
            if (u8_used[k]) (void)hipEventDestroy(u8_used[k]);
        }
        if (s_copy) (void)hipStreamDestroy(s_copy);
        if (s) (void)hipStreamSynchronize(s);
        if (s_comm) (void)hipStreamSynchronize(s_comm);
        if (s2) (void)hipStreamSynchronize(s2);
        for (int k = 1; k < MAXMB; k++) if (ms[k]) (void)hipStreamSynchronize(ms[k]);
        if (comm) ncclCommDestroy(comm);
        for (int k = 0; k < 2; k++) {
            if (dp_stage[k]) (void)hipHostFree(dp_stage[k]);
            if (dp_staged[k]) (void)hipEventDestroy(dp_staged[k]);
        }
        erase_stage.release();
        for (auto& a : allocs) (void)hipFree(a.p);
        for (auto e : chunk_ev) (void)hipEventDestroy(e);
        for (auto e : chunk_ev2) (void)hipEventDestroy(e);
        for (auto e : bev) if (e) (void)hipEventDestroy(e);
        for (auto& row : mev)
            for (auto e : row) if (e) (void)hipEventDestroy(e);
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        for (auto e : join_ev) if (e) (void)hipEventDestroy(e);
        for (auto e : chunk_evm) if (e) (void)hipEventDestroy(e);
        for (int k = 1; k < MAXMB; k++) if (ms[k]) (void)hipStreamDestroy(ms[k]);
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        if (comm_done) (void)hipEventDestroy(comm_done);
        if (s) (void)hipStreamDestroy(s);
        if (s_comm) (void)hipStreamDestroy(s_comm);
        if (s2) (void)hipStreamDestroy(s2);
    }

    // side pre-work (bf16 / fp8 with two streams, timing off): the gradient-arena
    // clear and the transposed weight copies run on s2 beside the forward instead of ahead of it on s.
    // pre_side_begin orders s2 after everything enqueued on s so far; pre_side_end records EV_PRE,
    // which s waits for before the backward's first gradient write (backward_bf16)
    bool pre_side_on() const { return two_streams && lowp() && !timing && s2; }
    hipStream_t pre_side_begin() {
        order(bev[EV_PRE_IN], s, s2);
        return s2;
    }
    void pre_side_end() {
        VIT_HIP(hipEventRecord(bev[EV_PRE], s2));
        pre_pending = true;
    }
    bool pre_pending = false;
    void pre_side_wait() {
        if (!pre_pending) return;
        VIT_HIP(hipStreamWaitEvent(s, bev[EV_PRE], 0));
        pre_pending = false;
    }
    void refresh_bf16() {
        if (!lowp()) return;
        pre_side_wait();  // an earlier refresh's transposes on s2 still read pbf
        to_bf16_k<<<grid_for(arena_elems, 256), 256, 0, s>>>(pbf, params, arena_elems);
        after_launch("params_to_bf16");
        refresh_transposed();
    }
    // pbfT <- transposes of the layer weights in pbf (after every SGD step): one launch per
    // weight kind over all L layers (the layers of a kind are a constant stride apart)
    void refresh_transposed() {
        tbeg(TC_MISC, 0);
        // bf16 mode: only the backward's dgrads read the transposes, so with side pre-work on they run
        // on s2 beside the next forward (s waits for them at the start of the backward).  fp8 mode
        // keeps them on s: refresh_fp8 below row-quantizes them (VIT_FP8_WT_COLS=0) right away
        const bool side = pre_side_on() && !fp8();
        hipStream_t ts = side ? pre_side_begin() : s;
        // fp8 mode reads no bf16 transposed copy (refresh_fp8 column-quantizes W for the dgrads)
        for (int k = 0; k < NWK && !(fp8() && wt_cols); k++) {
            const WKind w = wkind(k);
            const WSpan sp = wspan(k);
            transpose_bf16(WT(w.ti, sp.l0), W(w.ti, sp.l0), (int)w.N, (int)w.K, L, sp.stride, ts);
        }
        if (side) pre_side_end();
        if (patch_pad)  // the patch weight's padded copy (columns KP .. KPP-1 stay zero)
            VIT_HIP(hipMemcpy2DAsync(wpatch_pad, (size_t)KPP * 2, W(P_PATCH_W), (size_t)KP * 2, (size_t)KP * 2, C,
                                     hipMemcpyDeviceToDevice, s));
        tend();
        if (fp8()) refresh_fp8();
    }
    // MXFP8 weight copies: W [N][K] from the fp32 master, WT [Cin][OC] from the bf16 transpose;
    // one batched launch per kind over the L layers (a constant stride apart in the arena)
    void refresh_fp8() {
        tbeg(TC_QUANT, 0);
        for (int k = 0; k < NWK; k++) {
            const int ti = wkind(k).ti, l0 = wspan(k).l0;
            const long long N = wkind(k).N, K = wkind(k).K, as = wspan(k).stride;
            quantize_mx_batched_f32(wq[k].q, wq[k].s, P(ti, l0), N, (int)K, L, as, N * K,
                                    (long long)mx_scale_bytes(N, (int)K), s);
            if (wt_cols)  // Wt's MX rows = W's MX columns: byte-identical, without the bf16 transpose
                quantize_mx_cols_batched_bf16(wtq[k].q, wtq[k].s, W(ti, l0), N, (int)K, K, L, as, N * K,
                                              (long long)mx_scale_bytes(K, (int)N), s);
            else
                quantize_mx_batched_bf16(wtq[k].q, wtq[k].s, WT(ti, l0), K, (int)N, L, as, N * K,
                                         (long long)mx_scale_bytes(K, (int)N), s);
        }
        tend();
    }
    QMat wq_of(int ti, int l) const {
        const int k = wkind_of(ti), j = wslot(k, l);
        const WKind w = wkind(k);
        return {wq[k].q + (long long)j * w.N * w.K, wq[k].s + (long long)j * mx_scale_bytes(w.N, (int)w.K)};
    }
    QMat wtq_of(int ti, int l) const {
        const int k = wkind_of(ti), j = wslot(k, l);
        const WKind w = wkind(k);
        return {wtq[k].q + (long long)j * w.N * w.K, wtq[k].s + (long long)j * mx_scale_bytes(w.K, (int)w.N)};
    }
    // a forward (transposed = false) or input-gradient (true) GEMM of weight ti, layer l: bf16
    // mode as given; fp8 mode quantizes the bf16 A operand into the stream's scratch and runs the
    // MXFP8 engine against the weight's fp8 copy
    // pre: the A operand already in MX form (a fused epilogue wrote it); otherwise it is quantized
    // here.  mx_out: ask this GEMM's epilogue for the MX copy of its bf16 output (fp8 mode, fused)
    // colq: also write the column form of this micro-batch's A rows into colq (rowcol_on());
    // rec_ev: then record micro-batch event rec_ev (the weight gradient that reads colq waits on it)
    // pre: PRE_EPI = in act_q2 (a fused GEMM epilogue wrote it), PRE_LN = in act_q (ln_forward_mx)
    enum { PRE_NONE = 0, PRE_EPI = 1, PRE_LN = 2 };
    void gemm_w(int cls, GemmArgs a, int ti, int l, bool transposed, int mb, hipStream_t st, int pre = PRE_NONE,
                bool mx_out = false, const QMat* colq = nullptr, int rec_ev = -1) {
        if (!fp8()) { gemm(cls, a, true, st); return; }
        if (mx_out) { a.mx_q = act_q2[mb]; a.mx_s = act_s2[mb]; }
        const uint8_t* aq = act_q[mb];
        const uint8_t* as = act_s[mb];
        if (pre == PRE_EPI) {
            aq = act_q2[mb];
            as = act_s2[mb];
        } else if (pre == PRE_NONE) {
            tbeg(TC_QUANT, 0, st);
            if (colq) {
                const long long r0 = (long long)mb * (B / nmb) * T;
                const long long ntok = mb_ntok(mb, a.M);
                quantize_mx_rowcol_bf16(act_q[mb], act_s[mb], colq->q, colq->s, (const bf16_t*)a.A, a.M, a.K, a.lda,
                                        kp_tok, r0, ntok, st);
            } else {
                quantize_mx_bf16(act_q[mb], act_s[mb], (const bf16_t*)a.A, a.M, a.K, a.lda, a.K, st);
            }
            tend();
            if (rec_ev >= 0 && two_streams) VIT_HIP(hipEventRecord(mev[mb][rec_ev], st));
        }
        const QMat w = transposed ? wtq_of(ti, l) : wq_of(ti, l);
        a.A = aq; a.lda = a.K; a.a_scale = as;
        a.B = w.q; a.ldb = a.K; a.b_scale = w.s; a.b_kcontig = true;
        tbeg(cls, 2.0 * a.M * (double)a.N * a.K, st);
        gemm_fp8(a, st);
        tend();
    }

    // ------------------------------------------------------------------ last_cls
    // The head reads only the CLS row of each image from the last block's output, so in the last block
    // the row-wise ops after attention (attention projection, LayerNorm 2, fc + GELU, fcproj, and the fc /
    // attention-projection input gradients) run on the B CLS rows only, in place at row stride T in the
    // buffers of the full-size step.  bf16 mode only (fp32 is the parity path; the fp8 column forms span
    // 32-token blocks).  The last block's three weight gradients and the two kernels that take its small
    // gradients' partial sums (the fcproj dgrad: fc_b; LayerNorm 2 backward: ln2_w, ln2_b, attproj_b) stay
    // full size or (option last_cls_bwd, DESIGN.md §12.1: all but LayerNorm 2 backward) take forms that add
    // the same values in the same order, so every gradient keeps the full-size step's bits; the gradient
    // rows the trimmed kernels no longer write are cleared once per step (last_cls_clear).
    bool last_cls = true;    // option last_cls
    // option last_cls_bwd (honoured with last_cls on): 1 = the last block's three weight gradients skip the
    // K-steps without a CLS row (bit-identical: the skipped products are exact zeros), 0 = dense
    // 2 (default) = also the last block's fcproj input gradient on the CLS rows, its fc-bias column sums
    // stored per row into the partial rows of the full-size call (GemmArgs::colsum_row_period)
    int lc_bwd = 2;
    bool lc_d1_clean = false;  // this step's clears covered dfch's CLS blocks and the last block's fc-bias rows
    bool lc_active = false;  // the running step's forward ran trimmed (the backward follows it)
    bool lc_dirty = true;    // a backward (or nothing yet) wrote the shared gradient scratch since the last clear
    bool lc_pending = false; // the clears are in flight on s2 (EV_LC)
    bool last_cls_on() const { return last_cls && prec == VIT_BF16; }
    // the bf16 weight gradient dW[OC,Cin] += dout^T . inp over all B*T rows (wgrad)
    GemmArgs wgrad_args(const bf16_t* dout, int OC, const bf16_t* inp, int Cin, float* dW, int k_period) const {
        GemmArgs w;
        w.A = dout; w.lda = OC; w.a_kcontig = false;
        w.B = inp; w.ldb = Cin; w.b_kcontig = false;
        w.C = dW; w.ldc = Cin; w.M = OC; w.N = Cin; w.K = (int)BT; w.epi = EPI_F32_ATOMIC;
        w.ws = gemm_ws; w.ws_bytes = gemm_ws_bytes;
        // split-K fill: beside the micro-batch streams (concurrency on) the engine default (45 %: fewer
        // splits, their half-filled rounds shared); alone on the GPU (concurrency off: the bench's
        // per-kernel timing pass) 80 % of the slots
        w.fill_pct = two_streams ? 0 : 80;
        w.k_period = k_period;  // (bf16 engine: dout's rows off k_period are exact zeros, last_cls_bwd)
        return w;
    }
    // layer l's fcproj input gradient of micro-batch mb, full size: dfch = (dres3 . fcprojw) * gelu'(fch) (stored
    // as fchd), its column sums (fc_b) into the micro-batch's partial rows
    GemmArgs d1_args(int l, int mb, const bf16_t* dres3) const {
        const long long R = (long long)(B / nmb) * T, r0 = mb * R;
        GemmArgs d1;
        d1.A = dres3 + r0 * C; d1.lda = C; dgrad_b(d1, P_FCPROJW, l, C);
        d1.C = dfch + r0 * 4 * C; d1.ldc = 4 * C; d1.aux = la[l].fchd + r0 * 4 * C; d1.ldaux = 4 * C;
        d1.M = (int)R; d1.N = 4 * C; d1.K = C; d1.epi = EPI_BF16_MUL;
        d1.colsum_part = sg_rows(l, sg_fcb) + (long long)mb * gemm_colsum_rows(d1, fp8()) * 4 * C;
        return d1;
    }
    // fc-bias column-sum partial rows per micro-batch: those of the full-size fcproj dgrad (engine-dependent; the
    // call has the same shape in every layer and micro-batch)
    int fcb_rows() const { return gemm_colsum_rows(d1_args(0, 0, dres_bf), fp8()); }
    // last_cls_bwd = 2: the last block's d1_args gathered on the CLS rows, when T >= 128, the full-size call
    // would run on the 256x256 engine (not the ping-pong engine, whose partial rows are 96 tall) and the fc
    // weight gradient of the step skips the K-steps without a CLS row (it then reads dfch in the CLS rows'
    // 32-row blocks only).  false: d1 stays full size
    bool d1_gather(GemmArgs& d1) const {
        if (!(last_cls_on() && lc_bwd >= 2 && T >= 128 && d1.M >= 256)) return false;
        GemmArgs g = d1;
        g.M = B / nmb; g.lda = (long long)T * C; g.ldc = (long long)T * 4 * C; g.ldaux = (long long)T * 4 * C;
        g.rows_gathered = true; g.colsum_row_period = T;
        if (!gemm_colsum_period_ok(g) || gemm_colsum_rows(g, false) != fcb_rows()) return false;
        if (!gemm_bf16_kskip(wgrad_args(dfch, 4 * C, la[L - 1].ln2, C, G(P_FCW, L - 1), T))) return false;
        d1 = g;
        return true;
    }
    // dln_bf (the fc dgrad's output) and datty are scratch shared by all layers: after a backward they
    // hold layer 0's rows.  The last block's LayerNorm 2 backward and attention backward read every row
    // of them, and the trimmed fc / attproj dgrads write only the CLS rows, so the rest must be zero
    // (what the full-size kernels computed there).  Once per step, on s2
    // beside the forward: ordered by EV_LC_IN after everything enqueued on s so far (the previous
    // backward's micro-batch streams and s2 have joined s), and the backward's first kernel waits for
    // EV_LC (last_cls_wait) before any stream of it can write these buffers.
    void last_cls_clear() {
        if (!lc_dirty) return;
        hipStream_t cs = s;
        if (two_streams && s2) {
            order(bev[EV_LC_IN], s, s2);
            cs = s2;
        }
        VIT_HIP(hipMemsetAsync(dln_bf, 0, (size_t)BT * C * 2, cs));
        VIT_HIP(hipMemsetAsync(datty, 0, (size_t)BT * C * 2, cs));
        // last_cls_bwd = 2: the gathered fcproj dgrad writes only the CLS rows of dfch and of the fc-bias
        // partial rows.  The fc weight gradient reads dfch in the CLS rows' 32-row blocks, which hold layer
        // 0's rows (nothing else reads a non-CLS row of dfch in the last block), and the fixed-order reduce
        // reads every partial row
        GemmArgs d1 = d1_args(L - 1, 0, dres_bf);
        lc_d1_clean = d1_gather(d1);
        if (lc_d1_clean) {
            VIT_HIP(hipMemsetAsync(sg_rows(L - 1, sg_fcb), 0, (size_t)nmb * fcb_rows() * 4 * C * sizeof(float), cs));
            clear_cls_blocks_k<<<dim3(8, B), 256, 0, cs>>>(dfch, T, BT, 4 * C);
        }
        if (cs != s) {
            VIT_HIP(hipEventRecord(bev[EV_LC], cs));
            lc_pending = true;
        }
        lc_dirty = false;
    }
    void last_cls_wait() {
        if (!lc_pending) return;
        VIT_HIP(hipStreamWaitEvent(s, bev[EV_LC], 0));
        lc_pending = false;
    }

    // ------------------------------------------------------------------ head (both modes)
    // split-K of the M = B head GEMMs (bf16 / fp8 modes): about four 16-deep K-steps per work item.
    // The engine's rule stops at >= 8 K-steps per split (192-256 workgroups of 12-16 dependent
    // K-steps: 20-47 us per GEMM at B = 256, on the critical path between forward and backward);
    // bounded by the slab workspace
    int head_split(int M, int N, int K) const {
        int sp = std::min(16, std::max(1, K / 64));
        while (sp > 1 && (size_t)sp * M * N * sizeof(float) > gemm_ws_bytes) sp--;
        return sp;
    }
    void head_forward() {
        tbeg(TC_HEAD, 2.0 * B * C * NC);
        // lnf on the CLS row of each image (D15)
        const float* last = la[L - 1].res3;
        VIT_HIP(hipMemcpy2DAsync(cls_x, C * 4, last, (size_t)T * C * 4, C * 4, B, hipMemcpyDeviceToDevice, s));
        ln_forward_f32(lnf, lnf_mean, lnf_rstd, cls_x, P(P_LNFW), P(P_LNFB), B, C, s);
        GemmArgs a;
        a.A = lnf; a.lda = C; a.B = P(P_HEADW); a.ldb = C; a.C = logits; a.ldc = NC;
        a.bias = P(P_HEADB); a.M = B; a.N = NC; a.K = C; a.epi = EPI_F32_STORE;
        if (lowp()) {
            // fast path: the M = B head GEMMs have 64 output tiles for 256 CUs, so they run
            // split-K through fp32 slabs onto the broadcast bias (fp32 mode keeps the ordered sums)
            bcast_rows_k<<<cdiv((long long)B * NC, 256), 256, 0, s>>>(logits, P(P_HEADB), B, NC);
            a.bias = nullptr;
            a.epi = EPI_F32_ATOMIC;
            a.splitk = head_split(a.M, a.N, a.K);
        }
        a.ws = gemm_ws; a.ws_bytes = gemm_ws_bytes;
        gemm_f32(a, s);
        if (has_targets && soft_targets()) {
            softmax_ce_soft(probs, losses, logits, labels, two_labels() ? labels_b : nullptr, mix_lam,
                            smooth_eps, B, NC, s);
        } else {
            softmax_rows(probs, logits, B, NC, s);
            if (has_targets) ce_forward(losses, probs, labels, B, NC, s);
        }
        tend();
    }
    // dres_cur (zeroed) <- lnf backward on CLS rows (fp32 dres, or the bf16 stream dres_bf)
    void head_backward(float* dres, bf16_t* dres_bf = nullptr, uint8_t* dres_lo = nullptr) {
        tbeg(TC_HEAD, 4.0 * B * C * NC);
        fill_k<<<cdiv(B, 256), 256, 0, s>>>(dlosses, 1.0f / (float)b_global, B);
        VIT_HIP(hipMemsetAsync(dlogits, 0, (size_t)B * NC * 4, s));
        if (soft_targets())
            ce_soft_backward(dlogits, dlosses, probs, labels, two_labels() ? labels_b : nullptr, mix_lam,
                             smooth_eps, B, NC, s);
        else
            ce_backward(dlogits, dlosses, probs, labels, B, NC, s);
        VIT_HIP(hipMemsetAsync(dlnf, 0, (size_t)B * C * 4, s));
        GemmArgs a;  // dlnf += dlogits . head_w
        a.A = dlogits; a.lda = NC; a.a_kcontig = true;
        a.B = P(P_HEADW); a.ldb = C; a.b_kcontig = false;
        a.C = dlnf; a.ldc = C; a.M = B; a.N = C; a.K = NC; a.epi = lowp() ? EPI_F32_ATOMIC : EPI_F32_ACC;
        if (lowp()) a.splitk = head_split(a.M, a.N, a.K);
        a.ws = gemm_ws; a.ws_bytes = gemm_ws_bytes;
        gemm_f32(a, s);
        GemmArgs w;  // dhead_w += dlogits^T . lnf
        w.A = dlogits; w.lda = NC; w.a_kcontig = false;
        w.B = lnf; w.ldb = C; w.b_kcontig = false;
        w.C = G(P_HEADW); w.ldc = C; w.M = NC; w.N = C; w.K = B; w.epi = lowp() ? EPI_F32_ATOMIC : EPI_F32_ACC;
        if (lowp()) w.splitk = head_split(w.M, w.N, w.K);
        w.ws = gemm_ws; w.ws_bytes = gemm_ws_bytes;
        gemm_f32(w, s);
        colsum_f32(G(P_HEADB), dlogits, B, NC, NC, s, red_ws);
        VIT_HIP(hipMemsetAsync(dcls_x, 0, (size_t)B * C * 4, s));
        ln_backward_f32(dcls_x, G(P_LNFW), G(P_LNFB), dlnf, cls_x, P(P_LNFW), lnf_mean, lnf_rstd, B, C, s, red_ws);
        if (dres_bf) {
            VIT_HIP(hipMemsetAsync(dres_bf, 0, (size_t)BT * C * 2, s));
            VIT_HIP(hipMemsetAsync(dres_lo, 0, (size_t)BT * C, s));
            rows_to_bf16_k<<<cdiv((long long)B * C, 256), 256, 0, s>>>(dres_bf, dres_lo, (long long)T * C, dcls_x, B, C);
        } else {
            VIT_HIP(hipMemsetAsync(dres, 0, (size_t)BT * C * 4, s));
            VIT_HIP(hipMemcpy2DAsync(dres, (size_t)T * C * 4, dcls_x, C * 4, C * 4, B, hipMemcpyDeviceToDevice, s));
        }
        tend();
    }

    // ------------------------------------------------------------------ bf16 fast path
    // patch embedding (encoder_forward, train_vit.rs:196 -> ViT), each micro-batch on its stream.  The im2col rows
    // and the weight's rows are KPP wide: KP, or padded (patch_pad: zero-padded rows, the padded weight copy)
    void patch_forward() {
        const int Bm = B / nmb;
        for (int mb = 0; mb < nmb; mb++) {
            hipStream_t st = ms[mb];
            const long long img0 = (long long)mb * Bm;
            bf16_t* pt = patches_bf + img0 * NP * KPP;
            const float* px = pixels + img0 * 3 * cfg.img * cfg.img;
            tbeg(TC_PATCH, 2.0 * Bm * NP * (double)KP * C, st);
            if (patch_pad) im2col_pad_bf16(pt, px, Bm, cfg.img, cfg.patch, KPP, st);
            else im2col_bf16(pt, px, Bm, cfg.img, cfg.patch, st);
            GemmArgs a;
            a.A = pt; a.lda = KPP; a.B = patch_pad ? wpatch_pad : W(P_PATCH_W); a.ldb = KPP;
            a.C = emb_tmp + img0 * NP * C; a.ldc = C; a.bias = P(P_PATCH_B);
            a.M = Bm * NP; a.N = C; a.K = KPP; a.epi = EPI_F32_STORE;
            gemm_bf16(a, st);
            patch_assemble(encoded + img0 * T * C, emb_tmp + img0 * NP * C, P(P_CLS), P(P_WPE), Bm, NP, C, st);
            tend();
        }
    }
    // LayerNorm 1 (second = false: of the block's input) or 2 (of res2) of layer l: what its forward and its
    // backward share.  Pointers at row 0; colk: the index of its output's column form in actc
    struct LnSite { bf16_t* out; float *mean, *rstd; const float* inp; int tw, tb, colk; };
    LnSite ln_site(int l, bool second) const {
        const LayerActs& a = la[l];
        if (second) return {a.ln2, a.ln2_mean, a.ln2_rstd, a.res2, P_LN2W, P_LN2B, 2};
        return {a.ln1, a.ln1_mean, a.ln1_rstd, l == 0 ? encoded : la[l - 1].res3, P_LN1W, P_LN1B, 0};
    }
    // its forward on micro-batch mb: `rows` rows at row stride rs (last_cls: the CLS rows, in place), into bf16, or
    // (lnmx_on(): whole micro-batches only) into its two MX forms alone: the next GEMM's A operand in act_q and
    // the column form its weight gradient reads
    void ln_fwd(int l, int mb, bool second, long long rows, long long rs) {
        const LnSite n = ln_site(l, second);
        hipStream_t st = ms[mb];
        const long long r0 = (long long)mb * (B / nmb) * T;
        tbeg(TC_LN_FWD, 0, st);
        if (lnmx_on()) {
            const QMat c = actc_of(n.colk, l);
            ln_forward_mx(act_q[mb], act_s[mb], c.q, c.s, n.mean + r0, n.rstd + r0, n.inp + r0 * C, P(n.tw, l), P(n.tb, l),
                          rows, C, kp_tok, r0, mb_ntok(mb, rows), st, nullptr);
        } else {
            ln_forward_bf16(n.out + r0 * C, n.mean + r0, n.rstd + r0, n.inp + r0 * C, P(n.tw, l), P(n.tb, l), rows, C, st, rs);
        }
        tend();
    }
    void forward_bf16() {
        const int Bm = B / nmb;
        const long long R = (long long)Bm * T;  // rows per micro-batch
        lc_active = last_cls_on();
        if (lc_active) last_cls_clear();
        mb_fork();
        patch_forward();
        for (int l = 0; l < L; l++) {
            LayerActs& a = la[l];
            const float* xl = l == 0 ? encoded : la[l - 1].res3;
            // last_cls: the row-wise ops after attention take the Bm CLS rows (row stride T, in place)
            const bool lc = lc_active && l == L - 1;
            const int Mr = lc ? Bm : (int)R;
            const long long rs = lc ? T : 1;
            // ... on the engine their full-size form takes (GemmArgs::rows_gathered: R rows would run on the
            // 256x256 engine, so do the Bm), which keeps every CLS row's bits what they were
            const bool lcg = lc && R >= 256;
            for (int mb = 0; mb < nmb; mb++) {
                hipStream_t st = ms[mb];
                const long long r0 = (long long)mb * R;
                const float* x = xl + r0 * C;
                const bool rc = rowcol_on(), lm = lnmx_on();
                QMat c_ln1 = rc ? actc_of(0, l) : QMat{}, c_atty = rc ? actc_of(1, l) : QMat{},
                     c_ln2 = rc ? actc_of(2, l) : QMat{};
                ln_fwd(l, mb, false, R, 1);
                GemmArgs q;
                q.A = a.ln1 + r0 * C; q.lda = C; q.B = W(P_QKVW, l); q.ldb = C; q.C = a.qkv + r0 * 3 * C;
                q.ldc = 3 * C; q.bias = P(P_QKVB, l); q.M = (int)R; q.N = 3 * C; q.K = C; q.epi = EPI_BF16_STORE;
                gemm_w(TC_QKV_FWD, q, P_QKVW, l, false, mb, st, lm ? PRE_LN : PRE_NONE, false,
                       rc && !lm ? &c_ln1 : nullptr);
                tbeg(TC_ATTN_FWD, 4.0 * Bm * (double)T * T * C, st);
                attn_forward_fused(a.atty + r0 * C, a.lse + (long long)mb * Bm * NH * T, a.qkv + r0 * 3 * C, Bm, T, C, NH, st);
                tend();
                GemmArgs pr;
                pr.A = a.atty + r0 * C; pr.lda = rs * C; pr.B = W(P_ATTPROJW, l); pr.ldb = C; pr.C = a.res2 + r0 * C;
                pr.ldc = rs * C; pr.bias = P(P_ATTPROJB, l); pr.aux = x; pr.ldaux = rs * C;
                pr.M = Mr; pr.N = C; pr.K = C; pr.epi = EPI_F32_RESID; pr.rows_gathered = lcg;
                if (dp_fwd) {  // res2 = x + fl32(s * attproj(..)): the row scales at the rows' stride
                    pr.epi = EPI_F32_RESID_RS; pr.row_scale = dp_scale(l, 0, r0); pr.ld_row_scale = rs;
                }
                gemm_w(TC_PROJ_FWD, pr, P_ATTPROJW, l, false, mb, st, PRE_NONE, false, rc ? &c_atty : nullptr);
                ln_fwd(l, mb, true, Mr, rs);
                GemmArgs f;
                // fc: fchg = gelu(pre) for fcproj, fchd = gelu'(pre) for the fcproj dgrad (one sigmoid)
                f.A = a.ln2 + r0 * C; f.lda = rs * C; f.B = W(P_FCW, l); f.ldb = C; f.C = a.fchd + r0 * 4 * C;
                f.C2 = a.fchg + r0 * 4 * C; f.ldc = rs * 4 * C; f.bias = P(P_FCB, l); f.M = Mr; f.N = 4 * C;
                f.K = C; f.epi = EPI_BF16_GELU_D; f.rows_gathered = lcg;
                if (epicol_on()) {  // the GELU output only as its row (mx_out) and column MX forms
                    const QMat g = fchgc_of(l);
                    f.C2 = nullptr;
                    f.mxc_q = g.q; f.mxc_s = g.s; f.mxc_ld = kp_tok; f.mxc_off = r0;
                }
                gemm_w(TC_FC_FWD, f, P_FCW, l, false, mb, st, lm ? PRE_LN : PRE_NONE, fuse_mx,
                       rc && !lm ? &c_ln2 : nullptr);
                GemmArgs fp;
                fp.A = a.fchg + r0 * 4 * C; fp.lda = rs * 4 * C; fp.B = W(P_FCPROJW, l); fp.ldb = 4 * C;
                fp.C = a.res3 + r0 * C; fp.ldc = rs * C; fp.bias = P(P_FCPROJB, l); fp.aux = a.res2 + r0 * C;
                fp.ldaux = rs * C; fp.M = Mr; fp.N = C; fp.K = 4 * C; fp.epi = EPI_F32_RESID; fp.rows_gathered = lcg;
                if (dp_fwd) {
                    fp.epi = EPI_F32_RESID_RS; fp.row_scale = dp_scale(l, 1, r0); fp.ld_row_scale = rs;
                }
                gemm_w(TC_FCPROJ_FWD, fp, P_FCPROJW, l, false, mb, st, fuse_mx ? PRE_EPI : PRE_NONE);
            }
        }
        mb_join();
        head_forward();
    }

    // dW[OC,Cin] += dout^T . inp (reduction over all B*T rows, split-K slabs) on the weight-
    // gradient stream once every micro-batch stream has passed `ready` (dout final there); the
    // event `done` marks the end of its reads of dout / inp
    // dout_c / inp_c: column forms already written (rowcol_on(); dout_c's producer recorded `ready`)
    void wgrad(int cls, const bf16_t* dout, int OC, const bf16_t* inp, int Cin, float* dW, int ready,
               int done, const QMat* dout_c = nullptr, const QMat* inp_c = nullptr, int k_period = 0) {
        GemmArgs w = wgrad_args(dout, OC, inp, Cin, dW, k_period);
        hipStream_t st = two_streams ? s2 : s;
        if (two_streams) {
            for (int mb = 0; mb < nmb; mb++) {
                if (dout_c) VIT_HIP(hipStreamWaitEvent(s2, mev[mb][ready], 0));
                else order(mev[mb][ready], ms[mb], s2);
            }
        }
        if (fp8()) {
            const long long kp = mx_cols_kp(BT);
            const QMat qa = dout_c ? *dout_c : wg_a, qb = inp_c ? *inp_c : wg_b;
            if (!dout_c || !inp_c) {
                tbeg(TC_QUANT, 0, st);
                if (!dout_c) quantize_mx_cols_bf16(wg_a.q, wg_a.s, dout, BT, OC, OC, st);
                if (!inp_c) quantize_mx_cols_bf16(wg_b.q, wg_b.s, inp, BT, Cin, Cin, st);
                tend();
            }
            w.A = qa.q; w.lda = kp; w.a_kcontig = true; w.a_scale = qa.s;
            w.B = qb.q; w.ldb = kp; w.b_kcontig = true; w.b_scale = qb.s;
            w.K = (int)kp;
            tbeg(cls, 2.0 * w.M * (double)w.N * BT, st);
            gemm_fp8(w, st);
            tend();
        } else {
            tbeg(cls, 2.0 * w.M * (double)w.N * w.K, st);
            gemm_bf16(w, st);
            tend();
        }
        if (two_streams) VIT_HIP(hipEventRecord(bev[done], s2));
    }
    // a micro-batch stream may overwrite a buffer once the wgrad that reads it (`done`) finished
    void after_wgrad(int done, hipStream_t st) {
        if (two_streams) VIT_HIP(hipStreamWaitEvent(st, bev[done], 0));
    }

    float* sg_rows(int l, long long off) const { return sg_part[l & 1] + off; }
    // the layer's small gradients from the micro-batches' partial rows, in a fixed order, on the
    // weight-gradient stream once every micro-batch stream has finished the layer (LN1 backward).
    // Layer l-2 reuses this parity's rows only after waits on wgrad events recorded after this
    // reduce (after_wgrad in layer l-1 / l-2), so one pair of buffers suffices.
    void sg_finalize(int l, long long R) {
        hipStream_t st = two_streams ? s2 : s;
        for (int mb = 0; mb < nmb && two_streams; mb++) order(mev[mb][EV_SG], ms[mb], s2);
        const int nb = nmb * ln_bwd_blocks(R), w1 = l > 0 ? 3 * C : 2 * C;
        const float* p2 = sg_rows(l, sg_ln2);
        const float* p1 = sg_rows(l, sg_ln1);
        RowsJob jobs[8] = {
            {G(P_LN2W, l), p2, nb, 3 * C, C},
            {G(P_LN2B, l), p2 + C, nb, 3 * C, C},
            {G(P_ATTPROJB, l), p2 + 2 * C, nb, 3 * C, C},
            {G(P_LN1W, l), p1, nb, w1, C},
            {G(P_LN1B, l), p1 + C, nb, w1, C},
            {G(P_FCB, l), sg_rows(l, sg_fcb), nmb * fcb_rows(), 4 * C, 4 * C},
            {G(P_QKVB, l), sg_rows(l, sg_qkv), nmb, 3 * C, 3 * C},
            {l > 0 ? G(P_FCPROJB, l - 1) : nullptr, p1 + 2 * C, nb, w1, C},
        };
        tbeg(TC_COLSUM, 0, st);
        rows_reduce_add(jobs, l > 0 ? 8 : 7, st);
        tend();
    }

    // LayerNorm backward of the residual-gradient stream on micro-batch mb (R rows) of layer l:
    //   LN2 (second): dres2 = dres3 + LN2'(dln2) into dres_bf2 / dres_lo2; attproj_b += colsum(dres2)
    //   LN1:          dres  = dres2 + LN1'(dln1) into dres_bf / dres_lo;   fcproj_b of layer l-1 += colsum(dres)
    // dw | db | that bias go to the micro-batch's partial rows (sg_finalize).  Where a residual branch reads the
    // output (LN2, and LN1 above layer 0), also what that branch's GEMMs take in its place: with stochastic
    // depth the plane scaled by the branch's rows (the bias from the products), in fp8 mode (lnbmx_on()) its two
    // MX forms, the dgrad's A operand in act_q and the wgrad's dout in dcol, whose weight gradient waits for
    // the EV_RESB / EV_RESA recorded here
    void ln_bwd(int l, int mb, bool second, long long R) {
        const LnSite n = ln_site(l, second);
        const long long r0 = mb * R;
        const bool branch = second || l > 0;
        LnbArgs a;
        a.dres_out = (second ? dres_bf2 : dres_bf) + r0 * C; a.lo_out = (second ? dres_lo2 : dres_lo) + r0 * C;
        a.dres_in = (second ? dres_bf : dres_bf2) + r0 * C; a.lo_in = (second ? dres_lo : dres_lo2) + r0 * C;
        a.dw = G(n.tw, l); a.db = G(n.tb, l);
        a.dres_colsum = second ? G(P_ATTPROJB, l) : l > 0 ? G(P_FCPROJB, l - 1) : nullptr;
        a.dout = dln_bf + r0 * C; a.inp = n.inp + r0 * C; a.w = P(n.tw, l); a.mean = n.mean + r0; a.rstd = n.rstd + r0;
        a.rows = R; a.C = C;
        a.part = sg_rows(l, second ? sg_ln2 : sg_ln1) + (long long)mb * ln_bwd_blocks(R) * (a.dres_colsum ? 3 : 2) * C;
        const bool mx = branch && lnbmx_on();
        if (mx) {
            const QMat& c = dcol[second ? 1 : 0];
            a.qr = act_q[mb]; a.slr = act_s[mb]; a.qc = c.q; a.slc = c.s;
            a.ldqc = kp_tok; a.tok_off = r0; a.ntok = mb_ntok(mb, R); a.scratch = lnb_scr[mb];
        } else if (branch && dp_bwd) {
            a.dres_scaled = (second ? dres_s2 : dres_s) + r0 * C;
            a.row_scale = second ? dp_scale(l, 0, r0) : dp_scale(l - 1, 1, r0);
        }
        tbeg(TC_LN_BWD, 0, ms[mb]);
        ln_backward_stream(a, ms[mb]);
        if (mx && two_streams) VIT_HIP(hipEventRecord(mev[mb][second ? EV_RESB : EV_RESA], ms[mb]));
        tend();
    }
    void backward_bf16() {
        pre_side_wait();  // the arena clear and the transposed weights (side pre-work on s2)
        last_cls_wait();  // the per-step clears of dln_bf / datty (the micro-batch streams fork off s below)
        lc_dirty = true;
        const bool d1_clean = lc_d1_clean;  // (this backward overwrites what the clears prepared)
        lc_d1_clean = false;
        // the residual-gradient stream is "bf16 + lo8" (common.h: a bf16 plane, the GEMM operand,
        // plus a byte plane of its rounding residual; a 16-bit significand in 3 bytes): dres3 (the
        // layer output's gradient) in rbA/loA, dres2 in rbB/loB; each LayerNorm backward reads one
        // and writes the other (its column sum, the next bias gradient, is taken in fp32)
        bf16_t* rbA = dres_bf;   // dres3 (read by the fcproj dgrad / wgrad and LN2 backward)
        bf16_t* rbB = dres_bf2;  // dres2 (read by the attproj dgrad / wgrad and LN1 backward)
        head_backward(nullptr, rbA, dres_lo);
        chunk_done(0);
        // bias gradients are fused into the kernels that produce each gradient tensor:
        //   fcproj_b += colsum(dres3): LN1-backward of layer l+1 (head rows for the last layer)
        //   fc_b     += colsum(dfch):  fcproj dgrad epilogue
        //   attproj_b+= colsum(dres2): LN2-backward
        //   qkv_b    += colsum(dqkv):  attention backward
        // stochastic depth: the pass-through gradient stays rbA / rbB; each branch's GEMMs
        // read a second bf16 plane, bf16(fl32(s * dres)), and its last bias gradient sums the fp32 products.
        // sA / sB are written by the kernels that write rbA / rbB (the LayerNorm backwards; the head's rows
        // below), on the same streams, and read by the same GEMMs, so the EV_RESA / EV_RESB / after_wgrad
        // ordering of rbA / rbB orders them too.  Off the CLS rows of the last block they are exact zeros,
        // as rbA / rbB are (0 * s), so last_cls and last_cls_bwd hold unchanged.
        const bool dp = dp_bwd;
        const bf16_t* sA = dp ? dres_s : rbA;   // the fcproj dgrad's / wgrad's dout
        const bf16_t* sB = dp ? dres_s2 : rbB;  // the attproj dgrad's / wgrad's dout
        if (dp) {
            VIT_HIP(hipMemsetAsync(dres_s, 0, (size_t)BT * C * 2, s));
            rows_to_bf16_rs_k<<<cdiv((long long)B * C, 256), 256, 0, s>>>(dres_s, (long long)T * C, dcls_xs, dcls_x,
                                                                         dp_scale(L - 1, 1, 0), T, B, C);
            after_launch("drop_path_head_rows");
            colsum_f32(G(P_FCPROJB, L - 1), dcls_xs, B, C, C, s, red_ws);
        } else {
            colsum_f32(G(P_FCPROJB, L - 1), dcls_x, B, C, C, s, red_ws);
        }
        mb_fork();
        const int Bm = B / nmb;
        const long long R = (long long)Bm * T;
        for (int l = L - 1; l >= 0; l--) {
            LayerActs& a = la[l];
            // last_cls: dres3 is zero off the CLS rows (head_backward), so dfch, dln2 and dres2 are too: the
            // fc and attproj input gradients run on the Bm CLS rows (row stride T, in place), and the rows
            // they skip were cleared (last_cls_clear).  The weight gradients, the fcproj dgrad and LayerNorm 2
            // backward (whose partial rows make fc_b, ln2_w, ln2_b and attproj_b) stay full size, or
            // (last_cls_bwd, below) take forms that add the same values in the same order: they keep their bits
            const bool lc = lc_active && l == L - 1;
            const int Mr = lc ? Bm : (int)R;
            const long long rs = lc ? T : 1;
            const bool lcg = lc && R >= 256;  // (as in forward_bf16: the engine of the full-size form)
            // last_cls_bwd: the three weight gradients' dout (dres3, dfch, dres2) is exact zeros off the CLS
            // rows, so their split-K engine walks only the K-steps that hold a CLS row (GemmArgs::k_period)
            const int kper = lc && lc_bwd >= 1 ? T : 0;
            // rowcol: the weight gradients whose dout column form the dgrads' quantize step (or the LayerNorm
            // backward) writes are issued behind those dgrads (s2 waits on the event recorded after the
            // quantize), every other one ahead of them.  Each is described once; in fp8 mode sA / sB are rbA / rbB
            // and kper is 0
            const bool rc = rowcol_on(), ec = epicol_on();
            const QMat c_ln1 = rc ? actc_of(0, l) : QMat{}, c_atty = rc ? actc_of(1, l) : QMat{},
                       c_ln2 = rc ? actc_of(2, l) : QMat{}, c_fchg = ec ? fchgc_of(l) : QMat{};
            auto w_fcproj = [&] {  // fcprojw += dres3^T . fchg
                wgrad(TC_FCPROJ_WGRAD, sA, C, a.fchg, 4 * C, G(P_FCPROJW, l), EV_RESA, EV_W1, rc ? &dcol[0] : nullptr,
                      ec ? &c_fchg : nullptr, kper);
            };
            auto w_attproj = [&] {  // attprojw += dres2^T . atty
                wgrad(TC_PROJ_WGRAD, sB, C, a.atty, C, G(P_ATTPROJW, l), EV_RESB, EV_W3, rc ? &dcol[1] : nullptr,
                      rc ? &c_atty : nullptr, kper);
            };
            auto w_qkv = [&] {  // qkvw += dqkv^T . ln1
                wgrad(TC_QKV_WGRAD, dqkv, 3 * C, a.ln1, C, G(P_QKVW, l), EV_DQKV, EV_W4, rc ? &dcol[2] : nullptr,
                      rc ? &c_ln1 : nullptr);
            };
            // lbm: the LayerNorm backwards write dres2 / dres3's MX forms (dres3 of the last layer comes
            // from the head and is quantized by the fcproj dgrad as before)
            const bool lbm = lnbmx_on(), resa_pre = lbm && l < L - 1;
            // fcproj: dfch = (dres3 . fcprojw) * gelu'(fch) (stored as fchd)
            if (!rc) w_fcproj();
            for (int mb = 0; mb < nmb; mb++) {
                const long long r0 = mb * R;
                after_wgrad(EV_W2, ms[mb]);  // the previous layer's fc wgrad has read dfch
                GemmArgs d1 = d1_args(l, mb, sA);
                // (last_cls_bwd = 2 in the last block: on the CLS rows, where this step's clears covered it)
                if (lc && d1_clean && !ec) d1_gather(d1);
                if (ec) {  // dfch only as its row (mx_out) and column MX forms
                    d1.C = nullptr;
                    d1.mxc_q = dfchc.q; d1.mxc_s = dfchc.s; d1.mxc_ld = kp_tok; d1.mxc_off = r0;
                }
                gemm_w(TC_FCPROJ_DGRAD, d1, P_FCPROJW, l, true, mb, ms[mb], resa_pre ? PRE_LN : PRE_NONE, fuse_mx,
                       rc && !resa_pre ? &dcol[0] : nullptr, resa_pre ? -1 : EV_RESA);
                if (ec && two_streams) VIT_HIP(hipEventRecord(mev[mb][EV_DFCH], ms[mb]));  // dfchc final
            }
            if (rc) w_fcproj();
            // fc: dln2 = dfch . fcw;  fcw += dfch^T . ln2
            wgrad(TC_FC_WGRAD, dfch, 4 * C, a.ln2, C, G(P_FCW, l), EV_DFCH, EV_W2, ec ? &dfchc : nullptr,
                  rc ? &c_ln2 : nullptr, kper);
            for (int mb = 0; mb < nmb; mb++) {
                const long long r0 = mb * R;
                GemmArgs d2;
                d2.A = dfch + r0 * 4 * C; d2.lda = rs * 4 * C; dgrad_b(d2, P_FCW, l, 4 * C);
                d2.C = dln_bf + r0 * C; d2.ldc = rs * C; d2.M = Mr; d2.N = C; d2.K = 4 * C; d2.epi = EPI_BF16_STORE;
                d2.rows_gathered = lcg;
                gemm_w(TC_FC_DGRAD, d2, P_FCW, l, true, mb, ms[mb], fuse_mx ? PRE_EPI : PRE_NONE);
                after_wgrad(EV_W3, ms[mb]);  // the previous layer's attproj wgrad has read rbB
                ln_bwd(l, mb, true, R);
            }
            // attproj
            if (!rc) w_attproj();
            for (int mb = 0; mb < nmb; mb++) {
                const long long r0 = mb * R;
                GemmArgs d3;
                d3.A = sB + r0 * C; d3.lda = rs * C; dgrad_b(d3, P_ATTPROJW, l, C);
                d3.C = datty + r0 * C; d3.ldc = rs * C; d3.M = Mr; d3.N = C; d3.K = C; d3.epi = EPI_BF16_STORE;
                d3.rows_gathered = lcg;
                gemm_w(TC_PROJ_DGRAD, d3, P_ATTPROJW, l, true, mb, ms[mb], lbm ? PRE_LN : PRE_NONE, false,
                       rc && !lbm ? &dcol[1] : nullptr, lbm ? -1 : EV_RESB);
                // attention (+ qkv_b)
                after_wgrad(EV_W4, ms[mb]);  // the previous layer's qkv wgrad has read dqkv
                tbeg(TC_ATTN_BWD, 8.0 * Bm * (double)T * T * C, ms[mb]);
                attn_backward_fused(dqkv + r0 * 3 * C, datty + r0 * C, a.qkv + r0 * 3 * C, a.atty + r0 * C,
                                    a.lse + (long long)mb * Bm * NH * T, Bm, T, C, NH, ms[mb],
                                    sg_rows(l, sg_qkv) + (long long)mb * 3 * C,
                                    attn_part + (long long)attn_backward_ws_floats(mb * Bm, T, C, NH), true);
                tend();
            }
            if (rc) w_attproj();
            // qkv
            if (!rc) w_qkv();
            for (int mb = 0; mb < nmb; mb++) {
                const long long r0 = mb * R;
                GemmArgs d4;
                d4.A = dqkv + r0 * 3 * C; d4.lda = 3 * C; dgrad_b(d4, P_QKVW, l, 3 * C);
                d4.C = dln_bf + r0 * C; d4.ldc = C; d4.M = (int)R; d4.N = C; d4.K = 3 * C; d4.epi = EPI_BF16_STORE;
                gemm_w(TC_QKV_DGRAD, d4, P_QKVW, l, true, mb, ms[mb], PRE_NONE, false, rc ? &dcol[2] : nullptr, EV_DQKV);
                after_wgrad(EV_W1, ms[mb]);  // this layer's fcproj wgrad has read rbA
                ln_bwd(l, mb, false, R);
            }
            if (rc) w_qkv();
            sg_finalize(l, R);
            chunk_done(L - l);
        }
        mb_join();
        if (two_streams) order(bev[EV_JOIN], s2, s);  // every wgrad done before the slab workspace / grads are reused
        patch_backward();
        chunk_done(L + 1);
    }
    // patch embedding backward (encoder_backward, train_vit.rs:371 -> ViT) from the final dres in dres_bf / dres_lo
    void patch_backward() {
        tbeg(TC_PATCH_BWD, 2.0 * B * NP * (double)KP * C);
        // cls / position / patch-bias gradients (psg: three small kernels, 43 us) on s2 beside the
        // patch weight gradient on s; s waits for them before the chunk is final
        const bool psg_side = two_streams && lowp();
        if (psg_side) {
            order(bev[EV_SG], s, s2);
            patch_small_grads(G(P_CLS), G(P_WPE), G(P_PATCH_B), dres_bf, dres_lo, B, T, C, s2, pos_sums, psg_part);
            VIT_HIP(hipEventRecord(bev[EV_JOIN], s2));
        }
        patch_gather_bf16(dpatch_bf, dres_bf, B, NP, C, s);
        GemmArgs w;
        w.A = dpatch_bf; w.lda = C; w.a_kcontig = false;
        w.B = patches_bf; w.ldb = KPP; w.b_kcontig = false;
        w.C = G(P_PATCH_W); w.ldc = KP; w.M = C; w.N = KP; w.K = B * NP; w.epi = EPI_F32_ATOMIC;
        w.ws = gemm_ws; w.ws_bytes = gemm_ws_bytes;
        // after the join nothing but the small-gradient kernels runs beside it: split-K for 80 %
        // of the slots (the 45 % default leaves half the CUs idle: 102 us with 234 workgroups)
        w.fill_pct = 80;
        if (patch_pad) {  // dW over KPP columns into the scratch, then its first KP columns into G
            VIT_HIP(hipMemsetAsync(dwpatch_pad, 0, (size_t)C * KPP * 4, s));
            w.C = dwpatch_pad; w.ldc = KPP; w.N = KPP;
        }
        gemm_bf16(w, s);
        if (patch_pad)
            add_cols_k<<<grid_for((long long)C * KP, 256), 256, 0, s>>>(G(P_PATCH_W), dwpatch_pad, C, KP, KPP);
        if (psg_side)
            VIT_HIP(hipStreamWaitEvent(s, bev[EV_JOIN], 0));
        else
            patch_small_grads(G(P_CLS), G(P_WPE), G(P_PATCH_B), dres_bf, dres_lo, B, T, C, s, pos_sums, psg_part);
        tend();
    }

    // ------------------------------------------------------------------ fp32 reference path
    void forward_f32() {
        im2col_f32(patches_f, pixels, B, cfg.img, cfg.patch, s);
        {
            GemmArgs a;
            a.A = patches_f; a.lda = KP; a.B = P(P_PATCH_W); a.ldb = KP; a.C = emb_tmp; a.ldc = C;
            a.bias = P(P_PATCH_B); a.M = B * NP; a.N = C; a.K = KP; a.epi = EPI_F32_STORE;
            gemm_f32(a, s);
        }
        patch_assemble(encoded, emb_tmp, P(P_CLS), P(P_WPE), B, NP, C, s);
        for (int l = 0; l < L; l++) {
            LayerActs& a = la[l];
            const float* x = l == 0 ? encoded : la[l - 1].res3;
            ln_forward_f32(a.ln1f, a.ln1_mean, a.ln1_rstd, x, P(P_LN1W, l), P(P_LN1B, l), BT, C, s);
            mm_fwd(a.qkvf, a.ln1f, P(P_QKVW, l), P(P_QKVB, l), C, 3 * C);
            attn_forward_f32(a.attyf, a.preatt, a.att, a.qkvf, B, T, C, NH, s);
            mm_fwd(a.attproj, a.attyf, P(P_ATTPROJW, l), P(P_ATTPROJB, l), C, C);
            if (dp_fwd) add_rs(a.res2, x, a.attproj, dp_scale(l, 0, 0), BT * C);
            else add(a.res2, x, a.attproj, BT * C);
            ln_forward_f32(a.ln2f, a.ln2_mean, a.ln2_rstd, a.res2, P(P_LN2W, l), P(P_LN2B, l), BT, C, s);
            mm_fwd(a.fchf, a.ln2f, P(P_FCW, l), P(P_FCB, l), C, 4 * C);
            gelu(a.fchgf, a.fchf, BT * 4 * C);
            mm_fwd(a.fcproj, a.fchgf, P(P_FCPROJW, l), P(P_FCPROJB, l), 4 * C, C);
            if (dp_fwd) add_rs(a.res3, a.res2, a.fcproj, dp_scale(l, 1, 0), BT * C);
            else add(a.res3, a.res2, a.fcproj, BT * C);
        }
        head_forward();
    }
    void mm_fwd(float* out, const float* inp, const float* w, const float* b, int Cin, int OC) {
        GemmArgs a;
        a.A = inp; a.lda = Cin; a.B = w; a.ldb = Cin; a.C = out; a.ldc = OC; a.bias = b;
        a.M = (int)BT; a.N = OC; a.K = Cin; a.epi = EPI_F32_STORE;
        gemm_f32(a, s);
    }
    void mm_bwd(float* dinp, float* dw, float* db, const float* dout, const float* inp,
                const float* w, int Cin, int OC) {
        GemmArgs d;
        d.A = dout; d.lda = OC; d.B = w; d.ldb = Cin; d.b_kcontig = false; d.C = dinp; d.ldc = Cin;
        d.M = (int)BT; d.N = Cin; d.K = OC; d.epi = EPI_F32_ACC;
        gemm_f32(d, s);
        GemmArgs g;
        g.A = dout; g.lda = OC; g.a_kcontig = false; g.B = inp; g.ldb = Cin; g.b_kcontig = false;
        g.C = dw; g.ldc = Cin; g.M = OC; g.N = Cin; g.K = (int)BT; g.epi = EPI_F32_ATOMIC;
        g.ws = gemm_ws; g.ws_bytes = gemm_ws_bytes;
        gemm_f32(g, s);
        colsum_f32(db, dout, (int)BT, OC, OC, s, red_ws);
    }
    void add(float* out, const float* a, const float* b, long long n);
    void gelu(float* out, const float* in, long long n);
    void gelu_bwd(float* dinp, const float* in, const float* dout, long long n);
    void res_bwd(float* d1, float* d2, const float* dout, long long n);
    // stochastic depth: out = a + fl32(rs[row] * b);  d1 += dout, d2 += fl32(rs[row] * dout)  (rows of C)
    void add_rs(float* out, const float* a, const float* b, const float* rs, long long n);
    void res_bwd_rs(float* d1, float* d2, const float* dout, const float* rs, long long n);

    void backward_f32() {
        float* dcur = dres_a;
        float* dnxt = dres_b;
        head_backward(dcur);
        chunk_done(0);
        for (int l = L - 1; l >= 0; l--) {
            LayerActs& a = la[l];
            const float* x = l == 0 ? encoded : la[l - 1].res3;
            VIT_HIP(hipMemsetAsync(g_block, 0, g_block_elems * 4, s));
            VIT_HIP(hipMemsetAsync(dnxt, 0, BT * C * 4, s));
            // train_vit.rs:359-368
            if (dp_bwd) res_bwd_rs(g_dres2, g_dfcproj, dcur, dp_scale(l, 1, 0), BT * C);
            else res_bwd(g_dres2, g_dfcproj, dcur, BT * C);
            mm_bwd(g_dfchg, G(P_FCPROJW, l), G(P_FCPROJB, l), g_dfcproj, a.fchgf, P(P_FCPROJW, l), 4 * C, C);
            gelu_bwd(g_dfch, a.fchf, g_dfchg, BT * 4 * C);
            mm_bwd(g_dln2, G(P_FCW, l), G(P_FCB, l), g_dfch, a.ln2f, P(P_FCW, l), C, 4 * C);
            ln_backward_f32(g_dres2, G(P_LN2W, l), G(P_LN2B, l), g_dln2, a.res2, P(P_LN2W, l),
                            a.ln2_mean, a.ln2_rstd, BT, C, s, red_ws);
            if (dp_bwd) res_bwd_rs(dnxt, g_dattproj, g_dres2, dp_scale(l, 0, 0), BT * C);
            else res_bwd(dnxt, g_dattproj, g_dres2, BT * C);
            mm_bwd(g_datty, G(P_ATTPROJW, l), G(P_ATTPROJB, l), g_dattproj, a.attyf, P(P_ATTPROJW, l), C, C);
            attn_backward_f32(g_dqkv, g_dpreatt, g_datt, g_datty, a.qkvf, a.att, B, T, C, NH, s);
            mm_bwd(g_dln1, G(P_QKVW, l), G(P_QKVB, l), g_dqkv, a.ln1f, P(P_QKVW, l), C, 3 * C);
            ln_backward_f32(dnxt, G(P_LN1W, l), G(P_LN1B, l), g_dln1, x, P(P_LN1W, l), a.ln1_mean,
                            a.ln1_rstd, BT, C, s, red_ws);
            std::swap(dcur, dnxt);
            chunk_done(L - l);
        }
        im2col_f32(patches_f, pixels, B, cfg.img, cfg.patch, s);
        patch_gather_f32(dpatch_f, dcur, B, NP, C, s);
        GemmArgs w;
        w.A = dpatch_f; w.lda = C; w.a_kcontig = false; w.B = patches_f; w.ldb = KP; w.b_kcontig = false;
        w.C = G(P_PATCH_W); w.ldc = KP; w.M = C; w.N = KP; w.K = B * NP; w.epi = EPI_F32_ATOMIC;
        w.ws = gemm_ws; w.ws_bytes = gemm_ws_bytes;
        gemm_f32(w, s);
        patch_small_grads(G(P_CLS), G(P_WPE), G(P_PATCH_B), dcur, B, T, C, s, pos_sums);
        chunk_done(L + 1);
    }

    // ------------------------------------------------------------------ DP
    // Early SGD (option early_sgd, one GPU, bf16 / fp8, two streams, the fused train step): chunk c's
    // gradients are final at chunk_done(c) (the DP overlap's ordering, checked bit-for-bit by the
    // dp_probe test), and no later backward kernel reads chunk c's weights, so its SGD update runs
    // on s_comm (no extra stream: a seventh stream re-maps the streams onto the 4 hardware queues
    // and cost bf16 6 %) right there, beside the rest of the backward, instead of one 216 us pass.
    // The update is elementwise: the same bits as the whole-arena pass.  step() then only waits.
    // Measured (tools/ab_step.py, same process, profiles/r06_early_sgd_ab.txt): on s_comm ViT-B/16
    // 35.57 vs 35.56 and 35.65 vs 35.54 ms/step (-0.2 %), ViT-L/16 114.47 vs 114.79 (+0.3 %), ViT-H/14
    // fp8 114.68 vs 116.08 and 114.99 vs 115.72 (+1.2 / +0.6 %) on two boxes: on in fp8 mode (-1: auto)
    int early_sgd = -1;
    bool early_sgd_on() const { return early_sgd < 0 ? fp8() : early_sgd != 0; }
    bool early_on = false, early_done = false;
    float early_lr = 0.f;
    void sgd_chunk(int c, bool fanned = false) {  // fanned: s_comm already waits for the chunk (its accumulate)
        if (!fanned) chunk_fan_in(c);
        // the chunk's flat range, or its tiles of the whole-arena tiled kernel: elementwise, the one pass's bits
        optimizer_launch(sgd_kind(), optim_args(c, early_lr, false, groups_on), groups_on, s_comm);
        if (!ema_fuse(sgdm_on())) ema_behind(c, s_comm);
    }
    // chunk c's gradients are final on s (and, in the bf16 / fp8 backward with concurrency on, on s2 and
    // ms[1..nmb)): s_comm waits for all of them.  early_on and clip_live each imply two_streams && lowp()
    // (vit_trainer_train_step, clip_overlap_on), so their chunks always take the side-stream events.
    void chunk_fan_in(int c) {
        order(chunk_ev[c], s, s_comm);
        if (!(two_streams && lowp())) return;
        order(chunk_ev2[c], s2, s_comm);
        for (int k = 1; k < nmb; k++) order(chunk_evm[(size_t)c * MAXMB + k], ms[k], s_comm);
    }
    // Global-norm gradient clipping (option of vit_trainer_set_grad_clip).  The sum of
    // squares of the gradients is taken per gradient chunk (the chunk_off ranges, in every mode, so
    // its bits do not depend on where the launches were issued) into per-workgroup double slots
    // (ops.hip sumsq_partials), chunk c's at clip_slot_off[c]; the step's finishing kernel sums all
    // slots in order and writes the clip record {S, norm, c} the clipped optimizer kernels read.
    // The ranges include the arena's alignment padding, which is zero: init and every
    // vit_trainer_zero_grad clear the whole arena, every gradient kernel writes G(ti, l) over the
    // tensor's own extent only, and the all-reduce sums zeros (tests/test_gpu_gradclip.py checks the
    // norm against the canonical, unpadded gradients).
    // Overlapped form (bf16 / fp8, concurrency on, timing off, DP overlap on): chunk c's partials run
    // on s_comm at chunk_done(c), behind the events sgd_chunk / the DP path wait for (and behind the
    // chunk's all-reduce), beside the rest of the backward; no stream of its own (see early_sgd).
    // Plain form (otherwise, or when the current backward issued none): all of them at step time on s.
    float clip_max = 0.f;  // 0 = off
    int clip_overlap = -1;
    double* clip_slots = nullptr;  // allocated on first enabling, with clip_rec
    ClipRec* clip_rec = nullptr;
    int clip_slot_off[VIT_MAX_LAYERS + 3]{};
    bool clip_live = false;        // this backward issues the partials on s_comm
    bool clip_parts_valid = false; // ... and has issued all of them (reset by zero_grad / backward)
    bool clip_comm_busy = false;   // s_comm may still write clip_slots
    bool clip_have_norm = false;
    bool clip_on() const { return clip_max > 0.f; }
    bool clip_overlap_on() const {
        if (!(lowp() && two_streams && !timing && s2) || (comm && !overlap)) return false;
        // auto = the plain form in bf16 and in fp8 mode.  Measured (tools/bench_clip.py, same process,
        // profiles/grad_clip_ab.txt): ViT-B/16 bf16 SGD plain 36.07 / 36.18 vs overlapped 36.15 / 36.15
        // ms/step, AdamW 36.35 / 36.45 vs 36.46 / 36.48, ViT-H/14 fp8 119.06 / 118.81 vs 118.89 / 118.91:
        // no difference outside the 0.1-0.2 ms spread of either, so the form without the
        // cross-stream events is the default
        return clip_overlap < 0 ? false : clip_overlap != 0;
    }
    bool clip_enable() {
        if (clip_slots) return true;
        int n = 0;
        for (int c = 0; c < n_chunks; c++) {
            clip_slot_off[c] = n;
            n += sumsq_blocks(chunk_off[c + 1] - chunk_off[c]);
        }
        clip_slot_off[n_chunks] = n;
        clip_slots = alloc<double>(n);
        clip_rec = (ClipRec*)alloc<double>(2);
        return clip_slots && clip_rec;
    }
    void clip_partials(int c, hipStream_t st) {
        sumsq_partials(clip_slots + clip_slot_off[c], grads + chunk_off[c], chunk_off[c + 1] - chunk_off[c], st);
    }
    // the clip record of the gradients as they stand (after pre_side_wait and finish_allreduce), on s
    void clip_norm() {
        if (clip_comm_busy) {
            order(comm_done, s_comm, s);
            clip_comm_busy = false;
        }
        if (!clip_parts_valid)
            for (int c = 0; c < n_chunks; c++) clip_partials(c, s);
        clip_finish(clip_rec, clip_slots, clip_slot_off[n_chunks], clip_max, s);
        clip_parts_valid = false;
        clip_have_norm = true;
    }
    // Gradient accumulation (vit_trainer_set_grad_accum): with acc_steps = N > 1 the backwards
    // are counted in windows of N.  Backward 1 copies the gradient arena into acc (one more fp32 arena,
    // allocated by the first such backward), backward k < N adds the arena to acc, backward N adds acc into the
    // arena itself: grads then holds (((g1 + g2) + g3) + ... + gN), one fp32 addition per term in this order,
    // and everything at step time (the clip norm, every optimizer launch, the all-reduce, get_grads) reads it
    // as it reads any gradient.  The padding is zero in every term and stays zero.
    // Two forms of the same elementwise statement (option "accum_overlap"): plain, one launch over the arena on
    // s at the end of the backward; overlapped, chunk c's range on s_comm at chunk_done(c) behind
    // chunk_fan_in(c), beside the rest of the backward (no stream of its own: see early_sgd).  The backward that
    // completes a window takes the per-chunk form whenever chunk_done has a consumer of the chunk (the early SGD,
    // the live clip partials, the overlapped all-reduce, in any precision mode): that consumer runs on s_comm
    // behind the chunk's final sum.  Backwards 1 .. N-1 have no consumer: no early SGD, no live partials, no
    // all-reduce (torch's no_sync).  After a backward that launched on s_comm, s is ordered behind s_comm
    // (vit_trainer_backward): the next zero_grad (on s, or on s2 behind s: pre_side_begin), the next backward's
    // writers, the step and the readbacks all follow s.
    int acc_steps = 1, acc_done = 0;
    int acc_overlap = -1;
    float* acc = nullptr;
    int acc_k = 0;             // the running backward is number acc_k of its window (0: accumulation is off)
    bool acc_chunked = false;  // ... and sums per chunk on s_comm
    bool acc_comm_busy = false;
    bool acc_overlap_on() const {
        if (!(lowp() && two_streams && !timing && s2)) return false;
        // auto = plain in bf16 mode, overlapped in fp8 mode (as early_sgd).  Measured (tools/bench_accum.py, same
        // process, N = 4, profiles/grad_accum_ab.txt), ms per micro-step in two processes: ViT-B/16 bf16 plain
        // 34.10 / 34.15 vs overlapped 34.18 / 34.22 (plain ahead in both, the ranges disjoint in one), ViT-H/14 fp8
        // plain 113.97 / 114.46 vs overlapped 113.58 / 113.79 (overlapped ahead by 0.3 and 0.6 %, the ranges disjoint
        // in one; ahead in both processes of an earlier run on another box too)
        return acc_overlap < 0 ? fp8() : acc_overlap != 0;
    }
    bool acc_open() const { return acc_done > 0 && acc_done < acc_steps; }
    // false, with the error set, while a window is open: the optimizer steps and the checkpoint writer
    bool acc_closed(const char* who) {
        if (!acc_open()) return true;
        set_error("%s: gradient accumulation: micro-step %d of %d", who, acc_done, acc_steps);
        return false;
    }
    // the number the next backward has in its window (0: off)
    int acc_next() const { return acc_steps > 1 ? (acc_done >= acc_steps ? 1 : acc_done + 1) : 0; }
    // elements [o, o + n) of the running backward's statement, on st
    void acc_range(long long o, long long n, hipStream_t st) {
        if (acc_k == 1)
            VIT_HIP(hipMemcpyAsync(acc + o, grads + o, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        else if (acc_k < acc_steps)
            grad_accumulate_on(acc + o, acc + o, grads + o, n, st);
        else
            grad_accumulate_on(grads + o, acc + o, grads + o, n, st);
    }
    void chunk_done(int c) {
        bool fanned = false;
        if (acc_chunked) {
            chunk_fan_in(c);
            fanned = true;
            acc_range(chunk_off[c], chunk_off[c + 1] - chunk_off[c], s_comm);
            acc_comm_busy = true;
        }
        if (acc_k && acc_k < acc_steps) return;
        if (early_on) {
            sgd_chunk(c, fanned);
            return;
        }
        if (clip_live && !(comm && overlap)) {  // the chunk's partials beside the rest of the backward
            if (!fanned) chunk_fan_in(c);
            clip_partials(c, s_comm);
            clip_comm_busy = true;
            return;
        }
        if (!comm || !overlap) return;
        if (!fanned) chunk_fan_in(c);
        const long long o = chunk_off[c], n = chunk_off[c + 1] - chunk_off[c];
        ncclResult_t r = ncclAllReduce(grads + o, grads + o, (size_t)n, ncclFloat32, ncclSum, comm, s_comm);
        if (r != ncclSuccess) set_error("ncclAllReduce(chunk %d): %s", c, ncclGetErrorString(r));
        if (dp_probe_on)
            VIT_HIP(hipMemcpyAsync(dp_snap + o, grads + o, (size_t)n * 4, hipMemcpyDeviceToDevice, s_comm));
        if (clip_live) {  // the norm of the reduced gradients: identical on every rank
            clip_partials(c, s_comm);
            clip_comm_busy = true;
        }
    }
    void finish_allreduce() {
        if (!comm) return;  // (world 1 with a communicator still runs RCCL: the tested path)
        if (!overlap) {
            ncclResult_t r = ncclAllReduce(grads, grads, (size_t)arena_elems, ncclFloat32, ncclSum, comm, s);
            if (r != ncclSuccess) set_error("ncclAllReduce: %s", ncclGetErrorString(r));
            if (dp_probe_on)
                VIT_HIP(hipMemcpyAsync(dp_snap, grads, (size_t)arena_elems * 4, hipMemcpyDeviceToDevice, s));
            return;
        }
        order(comm_done, s_comm, s);
    }

    // upload one uint8 batch (host) and normalise it into `pixels` (include/vit_data.h)
    bool set_batch_u8(const unsigned char* img, const int* lab, const float* mean, const float* sd) {
        return stage_batch(img, nullptr, lab, mean, sd);
    }
    // the JPEG loader's current batch (include/vit_jpeg.h): decoded on the copy stream into the
    // same uint8 staging, then the same normalise
    bool set_batch_jpeg(vit_jpeg_loader_t* jl, const float* mean, const float* sd) {
        return stage_batch(nullptr, jl, nullptr, mean, sd);
    }
    bool stage_batch(const unsigned char* img, vit_jpeg_loader_t* jl, const int* lab, const float* mean,
                     const float* sd) {
        const int HW = cfg.img * cfg.img;
        const size_t bytes = (size_t)B * HW * 3;
        if (!s_copy) {
            VIT_HIP(hipStreamCreateWithFlags(&s_copy, hipStreamNonBlocking));
            for (int k = 0; k < 2; k++) {
                u8_stage[k] = alloc<unsigned char>((long long)bytes);
                lab_stage[k] = alloc<int>(B);
                VIT_HIP(hipEventCreateWithFlags(&u8_copied[k], hipEventDisableTiming));
                VIT_HIP(hipEventCreateWithFlags(&u8_used[k], hipEventDisableTiming));
                VIT_HIP(hipEventRecord(u8_used[k], s));
            }
            if (has_error()) return false;
        }
        const int k = u8_k & 1;
        u8_k++;
        // the staging slot is free once the normalise of two uploads ago has run
        VIT_HIP(hipStreamWaitEvent(s_copy, u8_used[k], 0));
        if (jl) {  // host entropy decode already done by the loader; the pixel work runs here
            if (!jpeg_loader_decode_to(jl, u8_stage[k], cfg.img, s_copy, &lab, B)) return false;
        } else {
            VIT_HIP(hipMemcpyAsync(u8_stage[k], img, bytes, hipMemcpyHostToDevice, s_copy));
            if (aug_pending) {  // between the upload and the normalise, on the copy stream; the
                aug_pending = false;  // host waits for u8_copied below, so the plan has been read
                if (!aug::enqueue(aug_plan, u8_stage[k], aug_scratch, s_copy)) return false;
            }
        }
        if (lab) VIT_HIP(hipMemcpyAsync(lab_stage[k], lab, (size_t)B * 4, hipMemcpyHostToDevice, s_copy));
        order(u8_copied[k], s_copy, s);
        has_targets = lab != nullptr;
        mixed = false;
        erased = false;
        const long long n = (long long)B * HW;
        normalize_u8_k<<<cdiv(n, 256), 256, 0, s>>>(pixels, labels, u8_stage[k], lab ? lab_stage[k] : nullptr,
                                                     B, HW, mean[0], mean[1], mean[2], sd[0], sd[1], sd[2]);
        after_launch("normalize_u8");
        VIT_HIP(hipEventRecord(u8_used[k], s));
        // the host buffers may be reused once the DMA has read them (overlaps the GPU's queue)
        VIT_HIP(hipEventSynchronize(u8_copied[k]));
        return !has_error();
    }

    bool set_augment_plan(const vit_aug_op_t* plan, int depth, const unsigned char* fill3) {
        if (!plan) {
            aug_pending = false;
            return true;
        }
        aug::Prepared p;
        if (!aug::prepare(plan, B, cfg.img, depth, fill3, "vit_trainer_set_augment_plan", p)) return false;
        if (!aug_scratch) aug_scratch = alloc<unsigned char>((long long)aug::scratch_bytes(B, cfg.img));
        if (!aug_scratch) return false;
        aug_plan = std::move(p);
        aug_pending = true;
        return true;
    }

    // Exponential moving average of the weights (vit_trainer_set_ema): one fp32 arena in the
    // layout of params, allocated by the first enabling, advanced by every optimizer step while on: inside the
    // optimizer kernels (bf16 / fp8 mode, AdamW in every mode), or by ema_update behind the fp32-mode SGD.
    // ema_view (vit_trainer_ema_weights): the two arena pointers are exchanged, so `params` (and with it
    // P(), the shadows' source and get_params) is the average and `ema` the live weights; every call
    // that would train, overwrite or save either is refused until the exchange is undone.
    float* ema = nullptr;
    bool ema_on = false, ema_view = false;
    float ema_d = 0.f, ema_omd = 0.f;
    long long ema_updates = 0;
    // option "ema_fused" (default 1): 0 launches the optimizer kernels without EMA and ema_update behind
    // each on the same stream (12 B per parameter instead of 8; the same bits): the A/B of
    // tools/bench_ema.py.  fp32-mode plain SGD has no EMA instantiation (optimizer.hip) and always takes that
    // form; AdamW and momentum SGD (shadowless = true) have one that needs no shadow.
    bool ema_fused = true;
    bool ema_fuse(bool shadowless) const { return ema_on && ema_fused && (lowp() || shadowless); }
    // the stand-alone update of gradient chunk c (c < 0: the whole arena) behind an un-fused optimizer launch
    void ema_behind(int c, hipStream_t st) {
        if (!ema_on) return;
        const long long o = c < 0 ? 0 : chunk_off[c], n = c < 0 ? arena_elems : chunk_off[c + 1] - chunk_off[c];
        ema_update_on(ema + o, params + o, n, ema_d, ema_omd, st);
    }
    // s behind the optimizer work of the side streams (early SGD on s_comm, the side pre-work on s2)
    void ema_join() {
        pre_side_wait();
        order(comm_done, s_comm, s);
    }
    void ema_set_decay(float d) {
        ema_d = d;
        ema_omd = (float)(1.0 - (double)d);
    }
    // the average := the current parameters (device copy), count 0
    bool ema_seed() {
        if (!ensure_arena(ema, false)) return false;
        ema_join();
        VIT_HIP(hipMemcpyAsync(ema, params, (size_t)arena_elems * 4, hipMemcpyDeviceToDevice, s));
        VIT_HIP(hipStreamSynchronize(s));
        ema_updates = 0;
        return !has_error();
    }
    bool set_ema(float d) {
        if (!(d >= 0.f && d < 1.f)) {
            set_error("vit_trainer_set_ema: decay %g outside [0, 1)", (double)d);
            return false;
        }
        if (d == 0.f) {  // off; the arena stays for the next enabling, which seeds it again
            ema_on = false;
            return true;
        }
        if (!ema_on && !ema_seed()) return false;
        ema_set_decay(d);
        ema_on = true;
        return true;
    }
    bool ema_weights(bool on) {
        if (on == ema_view || (on && !ema_on)) {
            set_error(on ? (ema_view ? "vit_trainer_ema_weights: EMA weights already in use"
                                     : "vit_trainer_ema_weights: EMA is off")
                         : "vit_trainer_ema_weights: EMA weights not in use");
            return false;
        }
        ema_join();
        std::swap(params, ema);
        ema_view = on;
        refresh_bf16();  // the bf16 shadow, the transposed copies, the padded patch weight, the fp8 MX copies
        VIT_HIP(hipStreamSynchronize(s));
        return !has_error();
    }
    // false (with the error set) while the averaged weights are exchanged in
    bool ema_unlocked(const char* who) {
        if (!ema_view) return true;
        set_error("%s: EMA weights in use", who);
        return false;
    }

    // Momentum SGD (vit_trainer_set_sgd): a setting of step / train_step / sgd_chunk.  While
    // momentum > 0 they launch the OPT_SGDM kernels over sgd_buf (one fp32 arena in the layout of params,
    // allocated and zeroed by the first such step), with first = 1 while sgd_steps == 0: the early per-chunk
    // launches of a train_step see the count its step() then advances, so every chunk of one step agrees.
    vit_sgd_t sgd_hp{0.f, 0.f, 0.f, 0};
    float sgd_omd = 1.0f;  // (float)(1.0 - (double)dampening)
    float* sgd_buf = nullptr;
    long long sgd_steps = 0;
    bool sgdm_on() const { return sgd_hp.momentum > 0.f; }
    OptKind sgd_kind() const { return sgdm_on() ? OPT_SGDM : OPT_SGD; }
    // (cleared on s; s_comm's chunk launches wait for s: chunk_fan_in)
    bool ensure_sgd_buf() { return ensure_arena(sgd_buf, true); }
    bool set_sgd(float mu, float damp, float wd, int nesterov) {
        if (!sgd_valid(mu, damp, wd, nesterov)) return false;
        sgd_hp = vit_sgd_t{mu, damp, wd, nesterov ? 1 : 0};
        sgd_omd = (float)(1.0 - (double)damp);
        return true;
    }
    // torch.optim.SGD's argument rules, and no decay without a buffer; false with the error set
    static bool sgd_valid(float mu, float damp, float wd, int nesterov) {
        if (!(std::isfinite(mu) && mu >= 0.f && std::isfinite(damp) && std::isfinite(wd) && wd >= 0.f)) {
            set_error("vit_trainer_set_sgd: momentum %g / weight_decay %g is not finite and >= 0, or dampening %g is "
                      "not finite", (double)mu, (double)wd, (double)damp);
            return false;
        }
        if (nesterov && !(mu > 0.f && damp == 0.f)) {
            set_error("vit_trainer_set_sgd: nesterov needs momentum > 0 and dampening 0 (momentum %g, dampening %g)",
                      (double)mu, (double)damp);
            return false;
        }
        if (wd > 0.f && !(mu > 0.f)) {
            set_error("vit_trainer_set_sgd: weight_decay %g needs momentum > 0 (plain SGD has no decayed form)",
                      (double)wd);
            return false;
        }
        return true;
    }

    // An optional fp32 arena in the layout of params (adam_m, adam_v, sgd_buf, ema): allocated on first use
    // and, zero, cleared on s then.  false with the error set when the allocation fails.
    bool ensure_arena(float*& a, bool zero) {
        if (a) return true;
        a = alloc<float>(arena_elems);
        if (!a) return false;
        if (zero) VIT_HIP(hipMemsetAsync(a, 0, arena_elems * 4, s));
        return true;
    }
    bool ensure_adam() { return ensure_arena(adam_m, true) && ensure_arena(adam_v, true); }
    // Parameter groups (vit_trainer_set_param_groups): per-(tensor, layer) multipliers
    // of lr and weight decay.  grp_lr / grp_wd keep the setting in the canonical [20 * L] indexing
    // (ignored entries as 1); the device tables are per segment in arena order (common.h GroupTab).
    // Chunk boundaries are segment boundaries, so chunk c is the tile range
    // [grp_chunk_tile[c], grp_chunk_tile[c + 1]) of the same kernel (early SGD).
    bool groups_on = false;
    std::vector<float> grp_lr, grp_wd;
    std::vector<int> grp_seg_entry;  // segment s (arena order) -> canonical entry ti * L + l
    int grp_chunk_tile[VIT_MAX_LAYERS + 3]{};
    GroupTab grp_tab{};
    float *grp_dev_lr = nullptr, *grp_dev_wd = nullptr;
    bool group_used(int ti, int l) const { return layered(ti) ? true : l == 0; }
    // segments and tiles of the layout; the static device tables.  Once, on the first enabling.
    bool groups_enable() {
        if (grp_tab.tile0) return true;
        for (int ti = 0; ti < 20; ti++)
            for (int l = 0; l < L; l++)
                if (group_used(ti, l)) grp_seg_entry.push_back(ti * L + l);
        std::sort(grp_seg_entry.begin(), grp_seg_entry.end(), [&](int a, int b) { return off[a] < off[b]; });
        const int nseg = (int)grp_seg_entry.size();  // 12 L + 8
        std::vector<long long> start(nseg + 1);
        std::vector<int> tile0(nseg + 1);
        for (int sgi = 0; sgi < nseg; sgi++) start[sgi] = off[grp_seg_entry[sgi]];
        start[nseg] = arena_elems;
        tile0[0] = 0;
        for (int sgi = 0; sgi < nseg; sgi++)
            tile0[sgi + 1] = tile0[sgi] + (int)((start[sgi + 1] - start[sgi] + GROUP_TILE - 1) / GROUP_TILE);
        for (int c = 0, sgi = 0; c <= n_chunks; c++) {
            while (sgi < nseg && start[sgi] < chunk_off[c]) sgi++;
            if (start[sgi] != chunk_off[c]) {
                set_error("parameter groups: chunk %d does not start a segment", c);
                return false;
            }
            grp_chunk_tile[c] = tile0[sgi];
        }
        int* d_tile0 = alloc<int>(nseg + 1);
        long long* d_start = alloc<long long>(nseg + 1);
        grp_dev_lr = alloc<float>(nseg);
        grp_dev_wd = alloc<float>(nseg);
        if (!d_tile0 || !d_start || !grp_dev_lr || !grp_dev_wd) return false;
        VIT_HIP(hipMemcpyAsync(d_tile0, tile0.data(), (size_t)(nseg + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        VIT_HIP(hipMemcpyAsync(d_start, start.data(), (size_t)(nseg + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
        VIT_HIP(hipStreamSynchronize(s));
        if (has_error()) return false;
        grp_tab = GroupTab{d_tile0, d_start, grp_dev_lr, grp_dev_wd, nseg};
        return true;
    }
    // lr_mul / wd_mul canonical [20 * L], either NULL = ones, both NULL = off
    bool set_groups(const float* lr_mul, const float* wd_mul) {
        const int n = 20 * L;
        if (!lr_mul && !wd_mul) {
            groups_on = false;
            grp_lr.assign(n, 1.0f);
            grp_wd.assign(n, 1.0f);
            return true;
        }
        std::vector<float> nl(n, 1.0f), nw(n, 1.0f);
        for (int ti = 0; ti < 20; ti++)
            for (int l = 0; l < L; l++) {
                if (!group_used(ti, l)) continue;
                const int e = ti * L + l;
                const float a = lr_mul ? lr_mul[e] : 1.0f, b = wd_mul ? wd_mul[e] : 1.0f;
                if (!(std::isfinite(a) && a >= 0.f && std::isfinite(b) && b >= 0.f)) {
                    set_error("vit_trainer_set_param_groups: tensor %d layer %d: lr_mul %g / wd_mul %g is not "
                              "finite and >= 0", ti, l, (double)a, (double)b);
                    return false;
                }
                nl[e] = a;
                nw[e] = b;
            }
        if (!groups_enable()) return false;
        const int nseg = grp_tab.nseg;
        std::vector<float> sl(nseg), sw(nseg);
        for (int sgi = 0; sgi < nseg; sgi++) {
            sl[sgi] = nl[grp_seg_entry[sgi]];
            sw[sgi] = nw[grp_seg_entry[sgi]];
        }
        // on the trainer's stream, behind every step in flight (a step leaves s behind the side
        // streams' optimizer work); synchronous, so the host vectors may go
        VIT_HIP(hipMemcpyAsync(grp_dev_lr, sl.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, s));
        VIT_HIP(hipMemcpyAsync(grp_dev_wd, sw.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, s));
        VIT_HIP(hipStreamSynchronize(s));
        if (has_error()) return false;
        grp_lr.swap(nl);
        grp_wd.swap(nw);
        grp_dev_ones = false;
        groups_on = true;
        return true;
    }
    // AdamW update t = adam_t + 1 (llm.c's update, which the reference's m/v buffers —
    // train_vit.rs:73-74 — were allocated for; its optimizer_step :737 is SGD)
    void step_adamw(float lr, const vit_adamw_t& hp) {
        if (!step_begin(&hp, false)) return;
        OptimArgs a = optim_args(-1, lr, true, groups_on);
        a.hp = adamw_hp(lr, hp, adam_t);
        optimizer_launch(OPT_ADAMW, a, groups_on, s);
        step_finish(true);
    }
    // LAMB (vit_trainer_step_lamb): AdamW's state and direction, the step of every segment
    // scaled by its trust ratio.  Always the tiled range of the parameter-group tables (a ratio is per
    // segment), with all-ones multipliers while groups are off.  On the first step: the tables, the
    // segments' own lengths, a {sum p^2, sum u^2} slot per tile and a {|w|, |u|, r} record per segment.
    long long* lamb_len = nullptr;
    double2* lamb_slots = nullptr;
    float* lamb_rec = nullptr;
    long long lamb_steps = 0;
    bool grp_dev_ones = false;  // the device multiplier tables hold all ones (filled here, not by set_groups)
    bool lamb_enable() {
        if (lamb_rec) return true;
        if (!groups_enable()) return false;
        const int nseg = grp_tab.nseg;
        std::vector<long long> len(nseg);
        for (int sgi = 0; sgi < nseg; sgi++) {
            const int ti = grp_seg_entry[sgi] / L;
            len[sgi] = layered(ti) ? canon_size[ti] / L : canon_size[ti];
        }
        long long* d_len = alloc<long long>(nseg);
        if (!d_len) return false;
        VIT_HIP(hipMemcpyAsync(d_len, len.data(), (size_t)nseg * sizeof(long long), hipMemcpyHostToDevice, s));
        VIT_HIP(hipStreamSynchronize(s));
        if (has_error()) return false;
        double2* slots = alloc<double2>(grp_chunk_tile[n_chunks]);  // (every tile of the arena)
        float* rec = alloc<float>((long long)nseg * LAMB_REC);
        if (!slots || !rec) return false;
        lamb_len = d_len;
        lamb_slots = slots;
        lamb_rec = rec;
        return true;
    }
    void step_lamb(float lr, const vit_adamw_t& hp, int flags) {
        if (!step_begin(&hp, true)) return;
        lamb_steps += 1;
        LambArgs a{};
        a.o = optim_args(-1, lr, true, true);
        a.o.hp = adamw_hp(lr, hp, adam_t);
        a.seg_len = lamb_len;
        a.slots = lamb_slots;
        a.rec = lamb_rec;
        a.flags = flags;
        optimizer_launch(a, true, s);
        step_finish(true);
    }

    // What step, step_adamw (hp) and step_lamb (hp, lamb) share.  The begin: s behind the side streams and the
    // all-reduce, the optimizer state of the step allocated (false, with the error set, if it cannot be), for
    // AdamW / LAMB the counters advanced, then the clip record when clipping is on.  The finish: the EMA behind
    // an optimizer launch that did not fuse it (shadowless: the launch has an EMA form without a bf16 shadow),
    // and the transposed bf16 weights.
    bool step_begin(const vit_adamw_t* hp, bool lamb) {
        pre_side_wait();
        finish_allreduce();
        if (hp ? !ensure_adam() : (sgdm_on() && !ensure_sgd_buf())) return false;
        if (lamb) {
            if (!lamb_enable()) return false;
            if (!groups_on && !grp_dev_ones) {  // the bits of 1.0f into both tables, on the device
                VIT_HIP(hipMemsetD32Async((hipDeviceptr_t)grp_dev_lr, 0x3f800000, grp_tab.nseg, s));
                VIT_HIP(hipMemsetD32Async((hipDeviceptr_t)grp_dev_wd, 0x3f800000, grp_tab.nseg, s));
                grp_dev_ones = true;
            }
        }
        if (hp) {
            adam_t += 1;
            adam_hp = *hp;
            if (ema_on) ema_updates++;
        }
        tbeg(TC_SGD, 0);
        if (clip_on()) clip_norm();
        return true;
    }
    void step_finish(bool shadowless) {
        if (!ema_fuse(shadowless)) ema_behind(-1, s);
        tend();
        if (lowp()) refresh_transposed();
    }

    // The arguments of the optimizer launch over gradient chunk c (c < 0: the whole arena) from the
    // trainer's state: tiled, the chunk's tiles of the arena (the form of parameter groups, and LAMB's
    // always); its flat range otherwise.  rec is the record clip_norm() has written (the caller runs it
    // first).  adamw: m / v are the moments, the hyper-parameters the caller's (adamw_hp); otherwise an SGD
    // launch, which with momentum on gets the buffer and its setting here.
    OptimArgs optim_args(int c, float lr, bool adamw, bool tiled) const {
        const long long o = c < 0 || tiled ? 0 : chunk_off[c];
        OptimArgs a{};
        a.p = params + o;
        a.g = grads + o;
        if (lowp()) a.pbf = pbf + o;
        a.hp.lr = lr;
        if (clip_on()) a.rec = clip_rec;
        if (ema_fuse(adamw || sgdm_on())) a.ema = EmaArg{ema + o, ema_d, ema_omd};
        if (adamw) {
            a.m = adam_m + o;
            a.v = adam_v + o;
        } else if (sgdm_on()) {
            a.m = sgd_buf + o;
            a.hp.wd = sgd_hp.weight_decay;
            a.hp.mu = sgd_hp.momentum;
            a.hp.omd = sgd_omd;
            a.hp.nesterov = sgd_hp.nesterov;
            a.hp.first = sgd_steps == 0;
        }
        if (tiled) {
            a.gt = grp_tab;
            a.tile_begin = c < 0 ? 0 : grp_chunk_tile[c];
            a.ntiles = grp_chunk_tile[c < 0 ? n_chunks : c + 1] - a.tile_begin;
        } else {
            a.n = c < 0 ? arena_elems : chunk_off[c + 1] - chunk_off[c];
        }
        return a;
    }

    void step(float lr) {
        if (ema_on) ema_updates++;
        if (early_done) {  // every chunk already updated on s_comm (train_step with early SGD)
            early_done = false;
            pre_side_wait();
            order(comm_done, s_comm, s);
            if (sgdm_on()) sgd_steps++;
            refresh_transposed();
            return;
        }
        if (!step_begin(nullptr, false)) return;
        optimizer_launch(sgd_kind(), optim_args(-1, lr, false, groups_on), groups_on, s);
        if (sgdm_on()) sgd_steps++;
        step_finish(sgdm_on());
    }
};

__global__ void add_k(float* o, const float* a, const float* b, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        o[i] = a[i] + b[i];
}
__global__ void gelu_k(float* o, const float* a, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        o[i] = gelu_f(a[i]);
}
__global__ void gelu_bwd_k2(float* d, const float* x, const float* g, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        d[i] += gelu_grad_f(x[i]) * g[i];
}
__global__ void resbwd_k(float* d1, float* d2, const float* g, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        d1[i] += g[i];
        d2[i] += g[i];
    }
}
// stochastic depth, fp32 mode: the residual add and its backward with the branch scaled
// per row (rs[i / C]); every product rounded to fp32 on its own
__global__ void add_rs_k(float* o, const float* a, const float* b, const float* rs, long long n, int C) {
#pragma clang fp contract(off)
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float y = rs[i / C] * b[i];
        o[i] = a[i] + y;
    }
}
__global__ void resbwd_rs_k(float* d1, float* d2, const float* g, const float* rs, long long n, int C) {
#pragma clang fp contract(off)
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float y = rs[i / C] * g[i];
        d1[i] += g[i];
        d2[i] += y;
    }
}
void Trainer::add_rs(float* out, const float* a, const float* b, const float* rs, long long n) {
    add_rs_k<<<grid_for(n, 256), 256, 0, s>>>(out, a, b, rs, n, C);
    after_launch("residual_forward_rowscale");
}
void Trainer::res_bwd_rs(float* d1, float* d2, const float* dout, const float* rs, long long n) {
    resbwd_rs_k<<<grid_for(n, 256), 256, 0, s>>>(d1, d2, dout, rs, n, C);
    after_launch("residual_backward_rowscale");
}
void Trainer::add(float* out, const float* a, const float* b, long long n) {
    add_k<<<grid_for(n, 256), 256, 0, s>>>(out, a, b, n);
    after_launch("residual_forward");
}
void Trainer::gelu(float* out, const float* in, long long n) {
    gelu_k<<<grid_for(n, 256), 256, 0, s>>>(out, in, n);
    after_launch("gelu_forward");
}
void Trainer::gelu_bwd(float* dinp, const float* in, const float* dout, long long n) {
    gelu_bwd_k2<<<grid_for(n, 256), 256, 0, s>>>(dinp, in, dout, n);
    after_launch("gelu_backward");
}
void Trainer::res_bwd(float* d1, float* d2, const float* dout, long long n) {
    resbwd_k<<<grid_for(n, 256), 256, 0, s>>>(d1, d2, dout, n);
    after_launch("residual_backward");
}

}  // namespace vit

// ============================================================================ C ABI
struct vit_trainer {
    vit::Trainer t;
};
using vit::set_error;

extern "C" {
vit_trainer_t* vit_trainer_create(const vit_config_t* cfg, int batch, int precision, int device) {
    auto* h = new vit_trainer();
    if (!h->t.init(cfg, batch, precision, device)) {
        h->t.destroy();
        delete h;
        return nullptr;
    }
    return h;
}
void vit_trainer_destroy(vit_trainer_t* h) {
    if (!h) return;
    h->t.destroy();
    delete h;
}
long long vit_trainer_num_params(const vit_trainer_t* h) { return h->t.n_params; }
long long vit_trainer_device_bytes(const vit_trainer_t* h) { return (long long)h->t.dev_bytes; }
int vit_trainer_set_params(vit_trainer_t* h, const float* hp) {
    if (!h->t.ema_unlocked("vit_trainer_set_params")) return 1;
    h->t.canon_to_device(hp, h->t.params);
    h->t.refresh_bf16();
    VIT_HIP(hipStreamSynchronize(h->t.s));
    return vit::has_error();
}
int vit_trainer_get_params(vit_trainer_t* h, float* hp) {
    h->t.device_to_canon(h->t.params, hp);
    return vit::has_error();
}
int vit_trainer_get_grads(vit_trainer_t* h, float* hg) {
    VIT_HIP(hipStreamSynchronize(h->t.s_comm));
    h->t.device_to_canon(h->t.grads, hg);
    return vit::has_error();
}
static bool labels_ok(const int* lab, int n, int nc) {
    for (int i = 0; i < n; i++)
        if (lab[i] < 0 || lab[i] >= nc) {
            set_error("label %d of the batch is %d, outside [0, %d)", i, lab[i], nc);
            return false;
        }
    return true;
}
int vit_trainer_set_batch(vit_trainer_t* h, const float* px, const int* lab) {
    auto& t = h->t;
    if (lab && !labels_ok(lab, t.B, t.NC)) return 1;
    VIT_HIP(hipMemcpyAsync(t.pixels, px, (size_t)t.B * 3 * t.cfg.img * t.cfg.img * 4, hipMemcpyHostToDevice, t.s));
    t.has_targets = lab != nullptr;
    t.mixed = false;
    t.erased = false;
    if (lab) VIT_HIP(hipMemcpyAsync(t.labels, lab, (size_t)t.B * 4, hipMemcpyHostToDevice, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    return vit::has_error();
}
int vit_trainer_set_batch_device(vit_trainer_t* h, const float* px, const int* lab) {
    auto& t = h->t;
    VIT_HIP(hipMemcpyAsync(t.pixels, px, (size_t)t.B * 3 * t.cfg.img * t.cfg.img * 4, hipMemcpyDeviceToDevice, t.s));
    t.has_targets = lab != nullptr;
    t.mixed = false;
    t.erased = false;
    if (lab) VIT_HIP(hipMemcpyAsync(t.labels, lab, (size_t)t.B * 4, hipMemcpyDeviceToDevice, t.s));
    return vit::has_error();
}
int vit_trainer_set_label_smoothing(vit_trainer_t* h, float eps) {
    if (!h || !(eps >= 0.f && eps < 1.f)) {
        set_error("vit_trainer_set_label_smoothing: eps %g outside [0, 1)", (double)eps);
        return 1;
    }
    h->t.smooth_eps = eps;
    return 0;
}
int vit_trainer_mix_batch(vit_trainer_t* h, int mode, float lam, int x0, int y0, int x1, int y1) {
    if (!h) {
        set_error("vit_trainer_mix_batch: null trainer");
        return 1;
    }
    auto& t = h->t;
    const int img = t.cfg.img;
    if (mode == VIT_MIX_NONE) return 0;
    if (mode != VIT_MIX_MIXUP && mode != VIT_MIX_CUTMIX) {
        set_error("vit_trainer_mix_batch: unknown mode %d", mode);
        return 1;
    }
    if (mode == VIT_MIX_MIXUP && !(lam >= 0.f && lam <= 1.f)) {
        set_error("vit_trainer_mix_batch: mixup lam %g outside [0, 1]", (double)lam);
        return 1;
    }
    if (mode == VIT_MIX_CUTMIX && (x0 < 0 || y0 < 0 || x1 > img || y1 > img || x0 > x1 || y0 > y1)) {
        set_error("vit_trainer_mix_batch: box [%d,%d) x [%d,%d) outside the %d x %d image", x0, x1, y0, y1,
                  img, img);
        return 1;
    }
    if (!t.has_targets) {
        set_error("vit_trainer_mix_batch: the batch has no labels");
        return 1;
    }
    if (t.mixed) {
        set_error("vit_trainer_mix_batch: the batch is already mixed");
        return 1;
    }
    if (!t.labels_b) {
        t.labels_b = t.alloc<int>(t.B);
        if (!t.labels_b) return 1;
    }
    if (mode == VIT_MIX_MIXUP) {
        vit::mixup_batch(t.pixels, t.labels_b, t.labels, t.B, img, lam, t.s);
    } else {
        const double area = (double)(x1 - x0) * (double)(y1 - y0);
        lam = (float)(1.0 - area / ((double)img * (double)img));
        vit::cutmix_batch(t.pixels, t.labels_b, t.labels, t.B, img, x0, y0, x1, y1, t.s);
    }
    if (vit::has_error()) return 1;
    t.mixed = true;
    t.mix_lam = lam;
    return 0;
}
int vit_trainer_erase_batch(vit_trainer_t* h, const int* host_boxes, int max_count, int mode, unsigned long long seed,
                            const long long* host_keys) {
    if (!h) {
        set_error("vit_trainer_erase_batch: null trainer");
        return 1;
    }
    auto& t = h->t;
    vit::erase::Plan p;
    if (!vit::erase::prepare(host_boxes, t.B, t.cfg.img, max_count, mode, seed, host_keys, "vit_trainer_erase_batch", p))
        return 1;
    if (t.mixed) {
        set_error("vit_trainer_erase_batch: the batch is already mixed");
        return 1;
    }
    if (t.erased) {
        set_error("vit_trainer_erase_batch: the batch is already erased");
        return 1;
    }
    if (!p.list.empty() && !t.erase_list) {
        t.erase_list = t.alloc<char>((long long)vit::erase::list_bytes(t.B));
        if (!t.erase_list) return 1;
    }
    if (!vit::erase::enqueue(p, t.pixels, t.erase_list, t.erase_stage, t.s)) return 1;
    t.erased = true;
    return 0;
}
int vit_trainer_get_pixels(vit_trainer_t* h, float* host) {
    auto& t = h->t;
    VIT_HIP(hipMemcpyAsync(host, t.pixels, (size_t)t.B * 3 * t.cfg.img * t.cfg.img * 4, hipMemcpyDeviceToHost, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    return vit::has_error();
}
int vit_trainer_forward(vit_trainer_t* h, int b_global) {
    auto& t = h->t;
    t.b_global = b_global > 0 ? b_global : t.B;
    t.dp_begin(t.has_targets);
    if (t.lowp()) t.forward_bf16(); else t.forward_f32();
    t.dp_fwd = false;
    return vit::has_error();
}
int vit_trainer_set_drop_path(vit_trainer_t* h, const float* host_scales) {
    if (!h) {
        set_error("vit_trainer_set_drop_path: null trainer");
        return 1;
    }
    return h->t.set_drop_path(host_scales) ? 0 : 1;
}
// host-only: the project's counter-form splitmix64 (loader.hip, augment.hip), tag "droppath"
static unsigned long long dp_sm64(unsigned long long seed, unsigned long long i) {
    unsigned long long z = seed + (i + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
int vit_drop_path_draw(unsigned long long seed, long long key, int num_layers, int batch, float rate, int linear,
                       float* out) {
    if (!out || num_layers < 1 || batch < 1 || !(rate >= 0.f && rate < 1.f)) {
        set_error("vit_drop_path_draw: bad arguments (num_layers %d, batch %d, rate %g of [0, 1))", num_layers, batch,
                  (double)rate);
        return 1;
    }
    const unsigned long long s = seed ^ dp_sm64(0x64726f7070617468ULL, (unsigned long long)key);
    for (int l = 0; l < num_layers; l++) {
        const float p = linear && num_layers > 1 ? (float)((double)rate * l / (num_layers - 1)) : rate;
        const float keep_scale = 1.0f / (1.0f - p);
        for (int br = 0; br < 2; br++)
            for (int b = 0; b < batch; b++) {
                const unsigned long long pos = (unsigned long long)(2 * l + br) * (unsigned long long)batch + b;
                const float u = (float)(dp_sm64(s, pos) >> 40) * (1.0f / 16777216.0f);
                out[((size_t)l * 2 + br) * batch + b] = u >= p ? keep_scale : 0.0f;
            }
    }
    return 0;
}
int vit_trainer_get_drop_path(vit_trainer_t* h, float* out, int* used) {
    if (!h) {
        set_error("vit_trainer_get_drop_path: null trainer");
        return 1;
    }
    auto& t = h->t;
    if (used) *used = t.dp_last_used ? 1 : 0;
    if (out && t.dp_last_used) memcpy(out, t.dp_used.data(), t.dp_used.size() * sizeof(float));
    return 0;
}
int vit_trainer_zero_grad(vit_trainer_t* h) {
    auto& t = h->t;
    if (!t.ema_unlocked("vit_trainer_zero_grad")) return 1;
    t.clip_parts_valid = false;
    // the previous step's all-reduce must be done with the arena before it is cleared
    if (t.comm) {
        t.order(t.comm_done, t.s_comm, t.s);
    }
    if (t.pre_side_on()) {  // on s2 beside the forward; the backward waits for it
        hipStream_t zs = t.pre_side_begin();
        VIT_HIP(hipMemsetAsync(t.grads, 0, t.arena_elems * 4, zs));
        t.pre_side_end();
    } else {
        VIT_HIP(hipMemsetAsync(t.grads, 0, t.arena_elems * 4, t.s));
    }
    return vit::has_error();
}
int vit_trainer_backward(vit_trainer_t* h) {
    auto& t = h->t;
    if (!t.ema_unlocked("vit_trainer_backward")) return 1;
    if (!t.has_targets) {
        set_error("vit_trainer_backward: the batch has no targets (forward-only batch)");
        return 1;
    }
    t.clip_parts_valid = false;
    // gradient accumulation: this is backward acc_k of its window; only the one that completes it (or any
    // backward while accumulation is off) has consumers in chunk_done
    t.acc_k = t.acc_next();
    const bool final_bwd = t.acc_k == 0 || t.acc_k == t.acc_steps;
    if (t.acc_k && !t.ensure_arena(t.acc, false)) return 1;
    t.clip_live = t.clip_on() && !t.early_on && t.clip_overlap_on() && final_bwd;
    t.acc_chunked = t.acc_k && (t.acc_overlap_on() ||
                                (final_bwd && (t.early_on || t.clip_live || (t.comm && t.overlap))));
    if (t.lowp()) t.backward_bf16(); else t.backward_f32();
    if (t.acc_k && !t.acc_chunked) t.acc_range(0, t.arena_elems, t.s);  // the plain form: every writer has joined s
    if (t.acc_comm_busy) {  // s, and through it every later writer and reader of either arena, behind the sums
        t.order(t.comm_done, t.s_comm, t.s);
        t.acc_comm_busy = false;
    }
    if (t.acc_k && !vit::has_error()) t.acc_done = t.acc_k;
    t.acc_k = 0;
    t.acc_chunked = false;
    t.clip_parts_valid = t.clip_live && !vit::has_error();
    t.clip_live = false;
    return vit::has_error();
}
int vit_trainer_step(vit_trainer_t* h, float lr) {
    if (!h->t.ema_unlocked("vit_trainer_step") || !h->t.acc_closed("vit_trainer_step")) return 1;
    h->t.step(lr);
    h->t.acc_done = 0;
    return vit::has_error();
}
int vit_trainer_train_step(vit_trainer_t* h, float lr, int b_global) {
    auto& t = h->t;
    if (!t.ema_unlocked("vit_trainer_train_step")) return 1;
    vit_trainer_zero_grad(h);
    vit_trainer_forward(h, b_global);
    // the fused step knows lr before the backward: SGD per finished chunk (Trainer::early_sgd)
    // (not under gradient clipping: no parameter may change before the global norm exists)
    // (under gradient accumulation only in the call that completes a window: the others update nothing)
    const int k = t.acc_next();
    const bool closes = k == 0 || k == t.acc_steps;
    t.early_on = t.early_sgd_on() && t.lowp() && !t.comm && t.two_streams && !t.timing && t.s2 && t.has_targets &&
                 !t.clip_on() && closes;
    t.early_lr = lr;
    if (t.early_on && t.sgdm_on() && !t.ensure_sgd_buf()) t.early_on = false;  // (the error is set: step() reports it)
    vit_trainer_backward(h);
    t.early_done = t.early_on && !vit::has_error();
    t.early_on = false;
    if (!closes) return vit::has_error();  // a micro-step inside the window: accumulated, no update
    vit_trainer_step(h, lr);
    return vit::has_error();
}
int vit_trainer_set_grad_accum(vit_trainer_t* h, int steps) {
    if (!h || steps < 1) {
        set_error("vit_trainer_set_grad_accum: %s", h ? "steps must be >= 1" : "null trainer");
        return 1;
    }
    auto& t = h->t;
    VIT_HIP(hipDeviceSynchronize());  // the sums in flight read the count
    t.acc_steps = steps;
    t.acc_done = 0;  // any call abandons an open window
    return vit::has_error();
}
int vit_trainer_get_grad_accum_info(vit_trainer_t* h, int* steps, int* done) {
    if (!h) {
        set_error("vit_trainer_get_grad_accum_info: null trainer");
        return 1;
    }
    if (steps) *steps = h->t.acc_steps;
    if (done) *done = h->t.acc_done;
    return 0;
}
int vit_trainer_get_grad_accum(vit_trainer_t* h, float* host) {
    if (!h || !host) {
        set_error("vit_trainer_get_grad_accum: null argument");
        return 1;
    }
    auto& t = h->t;
    if (!t.acc_open()) {
        set_error("vit_trainer_get_grad_accum: no open window (micro-step %d of %d)", t.acc_done, t.acc_steps);
        return 1;
    }
    t.device_to_canon(t.acc, host);  // on s, which every backward leaves behind its sums
    return vit::has_error();
}
int vit_trainer_set_batch_jpeg(vit_trainer_t* h, vit_jpeg_loader_t* l, const float* mean3, const float* std3) {
    if (!h || !l || !mean3 || !std3) {
        set_error("vit_trainer_set_batch_jpeg: null argument");
        return 1;
    }
    return h->t.set_batch_jpeg(l, mean3, std3) ? 0 : 1;
}
int vit_trainer_set_batch_u8(vit_trainer_t* h, const unsigned char* images, const int* labels,
                             const float* mean3, const float* std3) {
    if (!h || !images || !mean3 || !std3) {
        set_error("vit_trainer_set_batch_u8: null argument");
        return 1;
    }
    if (labels && !labels_ok(labels, h->t.B, h->t.NC)) return 1;
    return h->t.set_batch_u8(images, labels, mean3, std3) ? 0 : 1;
}
int vit_trainer_set_augment_plan(vit_trainer_t* h, const vit_aug_op_t* host_plan, int depth,
                                 const unsigned char* fill3) {
    if (!h) {
        set_error("vit_trainer_set_augment_plan: null trainer");
        return 1;
    }
    return h->t.set_augment_plan(host_plan, depth, fill3) ? 0 : 1;
}
int vit_trainer_step_adamw(vit_trainer_t* h, float lr, float beta1, float beta2, float eps,
                           float weight_decay) {
    if (!h->t.ema_unlocked("vit_trainer_step_adamw") || !h->t.acc_closed("vit_trainer_step_adamw")) return 1;
    h->t.step_adamw(lr, vit_adamw_t{beta1, beta2, eps, weight_decay});
    h->t.acc_done = 0;
    return vit::has_error();
}
int vit_trainer_step_lamb(vit_trainer_t* h, float lr, float beta1, float beta2, float eps, float weight_decay,
                          int flags) {
    if (!h) {
        set_error("vit_trainer_step_lamb: null trainer");
        return 1;
    }
    if (!h->t.ema_unlocked("vit_trainer_step_lamb") || !h->t.acc_closed("vit_trainer_step_lamb")) return 1;
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f)) {
        set_error("vit_trainer_step_lamb: beta1 %g / beta2 %g outside [0, 1)", (double)beta1, (double)beta2);
        return 1;
    }
    if (!(std::isfinite(eps) && eps >= 0.f && std::isfinite(weight_decay) && weight_decay >= 0.f)) {
        set_error("vit_trainer_step_lamb: eps %g / weight_decay %g is not finite and >= 0", (double)eps,
                  (double)weight_decay);
        return 1;
    }
    if (flags & ~(VIT_LAMB_ALWAYS_ADAPT | VIT_LAMB_TRUST_CLIP)) {
        set_error("vit_trainer_step_lamb: unknown flag bits 0x%x", flags);
        return 1;
    }
    h->t.step_lamb(lr, vit_adamw_t{beta1, beta2, eps, weight_decay}, flags);
    h->t.acc_done = 0;
    return vit::has_error();
}
int vit_trainer_get_lamb_info(vit_trainer_t* h, float* w_norm, float* u_norm, float* ratio, long long* steps) {
    if (!h) {
        set_error("vit_trainer_get_lamb_info: null trainer");
        return 1;
    }
    auto& t = h->t;
    if (steps) *steps = t.lamb_steps;
    if (!t.lamb_steps) {
        set_error("vit_trainer_get_lamb_info: no LAMB step has run");
        return 1;
    }
    const int nseg = t.grp_tab.nseg;
    std::vector<float> rec((size_t)nseg * vit::LAMB_REC);
    VIT_HIP(hipMemcpyAsync(rec.data(), t.lamb_rec, rec.size() * 4, hipMemcpyDeviceToHost, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    if (vit::has_error()) return 1;
    float* out[vit::LAMB_REC] = {w_norm, u_norm, ratio};
    for (int k = 0; k < vit::LAMB_REC; k++) {
        if (!out[k]) continue;
        for (int e = 0; e < 20 * t.L; e++) out[k][e] = k == 2 ? 1.0f : 0.0f;
        for (int sgi = 0; sgi < nseg; sgi++) out[k][t.grp_seg_entry[sgi]] = rec[(size_t)sgi * vit::LAMB_REC + k];
    }
    return 0;
}
int vit_trainer_set_grad_clip(vit_trainer_t* h, float max_norm) {
    if (!h || !(max_norm >= 0.f)) {
        set_error("vit_trainer_set_grad_clip: max_norm %g is not >= 0", (double)max_norm);
        return 1;
    }
    auto& t = h->t;
    if (max_norm > 0.f && !t.clip_enable()) return 1;
    if (!(max_norm > 0.f)) t.clip_parts_valid = false;
    t.clip_max = max_norm;
    return 0;
}
float vit_trainer_grad_norm(vit_trainer_t* h) {
    auto& t = h->t;
    if (!t.clip_have_norm) return -1.0f;
    ClipRec r{};
    VIT_HIP(hipMemcpyAsync(&r, t.clip_rec, sizeof(r), hipMemcpyDeviceToHost, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    return r.norm;
}
int vit_trainer_set_param_groups(vit_trainer_t* h, const float* lr_mul, const float* wd_mul) {
    if (!h) {
        set_error("vit_trainer_set_param_groups: null trainer");
        return 1;
    }
    return h->t.set_groups(lr_mul, wd_mul) ? 0 : 1;
}
int vit_trainer_get_param_groups(vit_trainer_t* h, float* lr_mul, float* wd_mul, int* on) {
    if (!h) {
        set_error("vit_trainer_get_param_groups: null trainer");
        return 1;
    }
    auto& t = h->t;
    const size_t n = (size_t)20 * t.L;
    for (size_t e = 0; e < n; e++) {
        if (lr_mul) lr_mul[e] = t.grp_lr.empty() ? 1.0f : t.grp_lr[e];
        if (wd_mul) wd_mul[e] = t.grp_wd.empty() ? 1.0f : t.grp_wd[e];
    }
    if (on) *on = t.groups_on ? 1 : 0;
    return 0;
}
int vit_trainer_set_ema(vit_trainer_t* h, float decay) {
    if (!h) {
        set_error("vit_trainer_set_ema: null trainer");
        return 1;
    }
    if (!h->t.ema_unlocked("vit_trainer_set_ema")) return 1;
    return h->t.set_ema(decay) ? 0 : 1;
}
int vit_trainer_get_ema_info(vit_trainer_t* h, float* decay, long long* updates, int* on) {
    if (!h) {
        set_error("vit_trainer_get_ema_info: null trainer");
        return 1;
    }
    auto& t = h->t;
    if (decay) *decay = t.ema_on ? t.ema_d : 0.f;
    if (updates) *updates = t.ema_updates;
    if (on) *on = t.ema_on ? 1 : 0;
    return 0;
}
int vit_trainer_get_ema(vit_trainer_t* h, float* host) {
    if (!h || !host || !h->t.ema_on) {
        set_error("vit_trainer_get_ema: %s", !h || !host ? "null argument" : "EMA is off");
        return 1;
    }
    auto& t = h->t;
    t.ema_join();
    t.device_to_canon(t.ema_view ? t.params : t.ema, host);  // (exchanged in: `params` is the average)
    return vit::has_error();
}
int vit_trainer_set_ema_params(vit_trainer_t* h, const float* host) {
    if (!h || !host || !h->t.ema_on) {
        set_error("vit_trainer_set_ema_params: %s", !h || !host ? "null argument" : "EMA is off");
        return 1;
    }
    auto& t = h->t;
    if (!t.ema_unlocked("vit_trainer_set_ema_params")) return 1;
    t.ema_join();
    t.canon_to_device(host, t.ema);
    return vit::has_error();
}
int vit_trainer_ema_weights(vit_trainer_t* h, int on) {
    if (!h) {
        set_error("vit_trainer_ema_weights: null trainer");
        return 1;
    }
    return h->t.ema_weights(on != 0) ? 0 : 1;
}
int vit_trainer_set_sgd(vit_trainer_t* h, float momentum, float dampening, float weight_decay, int nesterov) {
    if (!h) {
        set_error("vit_trainer_set_sgd: null trainer");
        return 1;
    }
    if (!h->t.ema_unlocked("vit_trainer_set_sgd")) return 1;
    return h->t.set_sgd(momentum, dampening, weight_decay, nesterov) ? 0 : 1;
}
int vit_trainer_get_sgd_info(vit_trainer_t* h, float* momentum, float* dampening, float* weight_decay, int* nesterov,
                             long long* steps) {
    if (!h) {
        set_error("vit_trainer_get_sgd_info: null trainer");
        return 1;
    }
    auto& t = h->t;
    if (momentum) *momentum = t.sgd_hp.momentum;
    if (dampening) *dampening = t.sgd_hp.dampening;
    if (weight_decay) *weight_decay = t.sgd_hp.weight_decay;
    if (nesterov) *nesterov = t.sgd_hp.nesterov;
    if (steps) *steps = t.sgd_steps;
    return 0;
}
int vit_trainer_get_momentum(vit_trainer_t* h, float* host) {
    if (!h || !host || !h->t.sgd_buf || !h->t.sgd_steps) {
        set_error("vit_trainer_get_momentum: %s", !h || !host ? "null argument" : "no momentum step has run");
        return 1;
    }
    VIT_HIP(hipDeviceSynchronize());
    h->t.device_to_canon(h->t.sgd_buf, host);
    return vit::has_error();
}
int vit_trainer_get_adamw_state(vit_trainer_t* h, float* m, float* v, int* step) {
    auto& t = h->t;
    if (step) *step = t.adam_t;
    if (!t.adam_m) {
        set_error("vit_trainer_get_adamw_state: no AdamW step has run");
        return 1;
    }
    VIT_HIP(hipDeviceSynchronize());
    if (m) t.device_to_canon(t.adam_m, m);
    if (v) t.device_to_canon(t.adam_v, v);
    return vit::has_error();
}
int vit_trainer_eval(vit_trainer_t* h, int* host_pred, int* host_correct) {
    auto& t = h->t;
    if (host_correct) *host_correct = -1;
    t.b_global = t.B;
    t.dp_begin(false);  // eval never drops (a pending table stays pending)
    if (t.lowp()) t.forward_bf16(); else t.forward_f32();
    VIT_HIP(hipMemsetAsync(t.preds + t.B, 0, 4, t.s));
    vit::argmax_rows_k<<<cdiv(t.B, 4), 256, 0, t.s>>>(t.preds, t.preds + t.B, t.logits,
                                                 t.has_targets ? t.labels : nullptr, t.B, t.NC);
    vit::after_launch("argmax_rows");
    std::vector<int> out(t.B + 1);
    VIT_HIP(hipMemcpyAsync(out.data(), t.preds, (size_t)(t.B + 1) * 4, hipMemcpyDeviceToHost, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    if (vit::has_error()) return 1;
    if (host_pred) memcpy(host_pred, out.data(), (size_t)t.B * 4);
    if (host_correct && t.has_targets) *host_correct = out[t.B];
    return 0;
}
// Save and load go through the one writer and the one reader of checkpoint.cpp: a section per optional
// arena.
int vit_trainer_save_checkpoint(vit_trainer_t* h, const char* path) {
    using namespace vit::ckpt;
    auto& t = h->t;
    if (!t.ema_unlocked("vit_trainer_save_checkpoint") || !t.acc_closed("vit_trainer_save_checkpoint")) return 1;
    VIT_HIP(hipDeviceSynchronize());
    if (vit::has_error()) return 1;
    // the arenas that exist, in file order: params; m, v once an AdamW or LAMB step has run; the EMA while it
    // is on; the momentum buffer once a momentum step has run
    const float* dev[SEC_COUNT] = {t.params, t.adam_m, t.adam_m ? t.adam_v : nullptr, t.ema_on ? t.ema : nullptr,
                                   t.sgd_buf && t.sgd_steps ? t.sgd_buf : nullptr};
    std::vector<float> host[SEC_COUNT];
    const float* sec[SEC_COUNT] = {};
    for (int k = 0; k < SEC_COUNT; k++) {
        if (!dev[k]) continue;
        host[k].resize((size_t)t.n_params);
        t.device_to_canon(dev[k], host[k].data());
        sec[k] = host[k].data();
    }
    if (vit::has_error()) return 1;
    Header hd;
    hd.cfg = t.cfg;
    hd.step = t.adam_t;
    hd.adamw = t.adam_hp;
    hd.ema_decay = t.ema_d;
    hd.ema_updates = t.ema_updates;
    hd.momentum_steps = t.sgd_steps;
    hd.sgd = t.sgd_hp;
    return vit::ckpt::write(path, hd, sec);
}
int vit_trainer_load_checkpoint(vit_trainer_t* h, const char* path) {
    using namespace vit::ckpt;
    auto& t = h->t;
    if (!t.ema_unlocked("vit_trainer_load_checkpoint")) return 1;
    Reader r;
    if (r.open(path) || r.require_config(&t.cfg)) return 1;
    const Header& hd = r.header();
    if (hd.has(SEC_EMA) && !(hd.ema_decay > 0.f && hd.ema_decay < 1.f)) {
        set_error("checkpoint %s: EMA decay %g outside (0, 1)", path, (double)hd.ema_decay);
        return 1;
    }
    const vit_sgd_t& sg = hd.sgd;
    if (hd.has(SEC_MOMENTUM) &&
        (hd.momentum_steps < 0 || !vit::Trainer::sgd_valid(sg.momentum, sg.dampening, sg.weight_decay, sg.nesterov))) {
        set_error("checkpoint %s: invalid momentum-SGD setting in the header", path);
        return 1;
    }
    // every present section into host memory before the device is touched: a failing load changes nothing
    std::vector<float> host[SEC_COUNT];
    for (int k = 0; k < SEC_COUNT; k++) {
        if (!hd.has((Section)k)) continue;
        host[k].resize((size_t)t.n_params);
        if (r.read((Section)k, host[k].data())) return 1;
    }
    VIT_HIP(hipDeviceSynchronize());
    t.acc_done = 0;  // an open accumulation window belongs to the parameters that are replaced here
    t.canon_to_device(host[SEC_PARAMS].data(), t.params);
    t.refresh_bf16();
    if (hd.has(SEC_M)) {
        if (!t.ensure_adam()) return 1;
        t.canon_to_device(host[SEC_M].data(), t.adam_m);
        t.canon_to_device(host[SEC_V].data(), t.adam_v);
        t.adam_t = hd.step;
        t.adam_hp = hd.adamw;
    } else if (t.adam_m) {  // a parameters-only file restarts the optimizer
        VIT_HIP(hipMemsetAsync(t.adam_m, 0, t.arena_elems * 4, t.s));
        VIT_HIP(hipMemsetAsync(t.adam_v, 0, t.arena_elems * 4, t.s));
        t.adam_t = 0;
    }
    if (hd.has(SEC_MOMENTUM)) {  // the file's buffer, count and setting
        if (!t.ensure_sgd_buf()) return 1;
        t.canon_to_device(host[SEC_MOMENTUM].data(), t.sgd_buf);
        t.sgd_steps = hd.momentum_steps;
        t.set_sgd(sg.momentum, sg.dampening, sg.weight_decay, sg.nesterov);
    } else {  // a file without one: the next momentum step seeds the buffer again; the setting stays
        t.sgd_steps = 0;
    }
    if (hd.has(SEC_EMA)) {  // the file's average, decay and count; EMA on
        if (!t.ensure_arena(t.ema, false)) return 1;
        t.canon_to_device(host[SEC_EMA].data(), t.ema);
        t.ema_set_decay(hd.ema_decay);
        t.ema_updates = hd.ema_updates;
        t.ema_on = true;
    } else if (t.ema_on) {  // a file without one restarts the average from the loaded parameters
        if (!t.ema_seed()) return 1;
    }
    VIT_HIP(hipStreamSynchronize(t.s));
    return vit::has_error();
}
float vit_trainer_mean_loss(vit_trainer_t* h) {
    auto& t = h->t;
    if (!t.has_targets) return -1.0f;  // train_vit.rs:264-266
    std::vector<float> l(t.B);
    VIT_HIP(hipMemcpyAsync(l.data(), t.losses, t.B * 4, hipMemcpyDeviceToHost, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    float m = 0.f;  // train_vit.rs:258-263
    for (float v : l) m += v;
    return m / (float)t.B;
}
int vit_trainer_get_logits(vit_trainer_t* h, float* out) {
    auto& t = h->t;
    VIT_HIP(hipMemcpyAsync(out, t.logits, (size_t)t.B * t.NC * 4, hipMemcpyDeviceToHost, t.s));
    VIT_HIP(hipStreamSynchronize(t.s));
    return vit::has_error();
}
int vit_trainer_sync(vit_trainer_t* h) {
    h->t.pre_side_wait();
    VIT_HIP(hipStreamSynchronize(h->t.s_comm));
    VIT_HIP(hipStreamSynchronize(h->t.s));
    return vit::has_error();
}
void* vit_trainer_stream(vit_trainer_t* h) { return (void*)h->t.s; }

int vit_layout_query(const vit_config_t* cfg, long long* tensor_off, long long* chunk_off, long long* arena_elems) {
    if (!cfg || cfg->num_layers < 1 || cfg->num_layers > VIT_MAX_LAYERS || cfg->patch < 1 || cfg->img < cfg->patch ||
        cfg->channels < 1 || cfg->num_classes < 1) {
        set_error("vit_layout_query: bad config");
        return -1;
    }
    const int L = cfg->num_layers, np = (cfg->img / cfg->patch) * (cfg->img / cfg->patch);
    long long canon[20], n_params = 0, co[VIT_MAX_LAYERS + 3], arena = 0;
    std::vector<long long> off;
    int n_chunks = 0;
    vit::compute_layout(cfg->channels, L, np + 1, cfg->in_ch * cfg->patch * cfg->patch, cfg->num_classes, canon,
                        n_params, off, co, n_chunks, arena);
    if (tensor_off) memcpy(tensor_off, off.data(), off.size() * sizeof(long long));
    if (chunk_off) memcpy(chunk_off, co, (size_t)(n_chunks + 1) * sizeof(long long));
    if (arena_elems) *arena_elems = arena;
    return n_chunks;
}
int vit_dp_unique_id_size(void) { return (int)sizeof(ncclUniqueId); }
int vit_dp_get_unique_id(char* out) {
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) {
        set_error("ncclGetUniqueId: %s", ncclGetErrorString(r));
        return 1;
    }
    memcpy(out, &id, sizeof(id));
    return 0;
}
int vit_trainer_dp_init(vit_trainer_t* h, int rank, int world, const char* uid, int overlap) {
    auto& t = h->t;
    t.rank = rank;
    t.world = world;
    t.overlap = overlap;
    if (world < 1 || rank < 0 || rank >= world) {
        set_error("vit_trainer_dp_init: bad rank %d / world %d", rank, world);
        return 1;
    }
    ncclUniqueId id;
    memcpy(&id, uid, sizeof(id));
    VIT_HIP(hipSetDevice(t.device));
    ncclResult_t r = ncclCommInitRank(&t.comm, world, id, rank);
    if (r != ncclSuccess) {
        set_error("ncclCommInitRank(rank %d/%d): %s", rank, world, ncclGetErrorString(r));
        t.comm = nullptr;
        return 1;
    }
    return 0;
}
int vit_trainer_get_dp_snapshot(vit_trainer_t* h, float* host) {
    auto& t = h->t;
    if (!t.dp_probe_on) {
        set_error("vit_trainer_get_dp_snapshot: option dp_probe is off");
        return 1;
    }
    VIT_HIP(hipStreamSynchronize(t.s_comm));
    t.device_to_canon(t.dp_snap, host);
    return vit::has_error();
}
int vit_trainer_dp_ranks(vit_trainer_t* h) {
    if (!h->t.comm) return 0;
    int n = 0;
    ncclResult_t r = ncclCommCount(h->t.comm, &n);
    if (r != ncclSuccess) {
        set_error("ncclCommCount: %s", ncclGetErrorString(r));
        return -1;
    }
    return n;
}
int vit_trainer_set_concurrency(vit_trainer_t* h, int on) {
    auto& t = h->t;
    VIT_HIP(hipStreamSynchronize(t.s2));
    for (int k = 0; k < vit::Trainer::MAXMB; k++) if (t.ms[k]) VIT_HIP(hipStreamSynchronize(t.ms[k]));
    t.two_streams = on != 0;
    t.nmb = t.pick_nmb(t.mb_want);
    t.lc_dirty = true;
    t.lc_d1_clean = false;
    return vit::has_error();
}
int vit_trainer_set_option(vit_trainer_t* h, const char* name, int value) {
    auto& t = h->t;
    VIT_HIP(hipDeviceSynchronize());
    t.lc_dirty = true;  // (last_cls: the next forward redoes its clears for the new settings)
    t.lc_d1_clean = false;
    const std::string n = name ? name : "";
    if (n == "microbatch") {
        t.mb_want = value;
        t.nmb = t.pick_nmb(value);
    } else if (n == "ema_fused") {  // 0: EMA as ema_update launches behind the un-fused optimizer kernels (A/B)
        t.ema_fused = value != 0;
    } else if (n == "early_sgd") {  // one GPU: SGD per finished gradient chunk inside train_step (default: fp8 mode only)
        t.early_sgd = value < 0 ? -1 : value != 0;
    } else if (n == "accum_overlap") {  // gradient accumulation: the sums per chunk beside the backward (1), one pass behind it (0), auto (-1)
        t.acc_overlap = value < 0 ? -1 : value != 0;
    } else if (n == "clip_overlap") {  // gradient clipping: partial sums per chunk beside the backward (1), at step time (0), auto (-1)
        t.clip_overlap = value < 0 ? -1 : value != 0;
    } else if (n == "last_cls") {  // bf16: the last block's row-wise ops after attention on the CLS rows only (default 1)
        t.last_cls = value != 0;
    } else if (n == "last_cls_bwd") {  // bf16, with last_cls: the last block's weight gradients on the CLS K-steps (1) and its fcproj dgrad on the CLS rows (2, default)
        t.lc_bwd = value < 0 ? 0 : value;
    } else if (n == "dp_probe") {
        if (value && !t.dp_snap) {  // allocated once, kept until destroy
            t.dp_snap = t.alloc<float>(t.arena_elems);
            if (t.dp_snap) VIT_HIP(hipMemset(t.dp_snap, 0, t.arena_elems * 4));
        }
        t.dp_probe_on = value != 0 && t.dp_snap != nullptr;
    } else {
        set_error("vit_trainer_set_option: unknown option '%s'", n.c_str());
        return 1;
    }
    return vit::has_error();
}
int vit_trainer_set_timing(vit_trainer_t* h, int on) {
    h->t.timing = on != 0;
    return 0;
}
int vit_trainer_timing(vit_trainer_t* h, const char** names, double* ms, long long* calls,
                       double* flops, int max) {
    auto& t = h->t;
    t.collect();
    int n = 0;
    for (int c = 0; c < vit::TC_COUNT && n < max; c++) {
        if (!t.t_calls[c]) continue;
        names[n] = vit::kTimerNames[c];
        ms[n] = t.t_ms[c];
        calls[n] = t.t_calls[c];
        flops[n] = t.t_flops[c];
        n++;
    }
    return n;
}
void vit_trainer_timing_reset(vit_trainer_t* h) {
    auto& t = h->t;
    t.collect();
    for (int c = 0; c < vit::TC_COUNT; c++) {
        t.t_ms[c] = 0;
        t.t_calls[c] = 0;
        t.t_flops[c] = 0;
    }
}
}  // extern "C"
