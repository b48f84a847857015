// ops_internal.h — stream-explicit launchers shared by the C-ABI ops and the trainer.
#pragma once
#include "common.h"
#include "gemm.h"
#include "../../include/vit_ops.h"

namespace vit {
int grid_for(long long n, int threads);
void ln_forward_f32(float* out, float* mean, float* rstd, const float* inp, const float* w,
                    const float* b, long long rows, int C, hipStream_t s);
// row_stride: logical row r is row r * row_stride of out / inp / mean / rstd (the trainer's last block
// normalises only the CLS row of each image, in place: stride T)
void ln_forward_bf16(bf16_t* out, float* mean, float* rstd, const float* inp, const float* w,
                     const float* b, long long rows, int C, hipStream_t s, long long row_stride = 1);
// dinp += LN_dinp(dout); dw / db += the column sums, in a fixed order through per-block partial
// rows in ws (nullptr = thread workspace; ln_bwd_blocks(rows) * 2C floats)
void ln_backward_f32(float* dinp, float* dw, float* db, const float* dout, const float* inp,
                     const float* w, const float* mean, const float* rstd, long long rows, int C,
                     hipStream_t s, float* ws = nullptr);
// the trainer's residual-gradient stream in "bf16 + lo8" form (common.h lo8_*: a bf16 plane, the
// GEMM operand, and a byte plane of the rounding residual; lo planes nullable = plain bf16):
// dres_out = dres_in + LN_dinp(dout); dres_colsum / dw / db as above, taken in fp32 before the
// rounding; part != null: per-block partial rows [ln_bwd_blocks(rows)][2C or 3C] (dw | db |
// dres_colsum) instead of atomics, summed later in a fixed order (else reduced into dw / db / dres_colsum)
struct LnbArgs {
    bf16_t* dres_out = nullptr;
    uint8_t* lo_out = nullptr;
    const bf16_t* dres_in = nullptr;
    const uint8_t* lo_in = nullptr;
    float *dw = nullptr, *db = nullptr, *dres_colsum = nullptr, *part = nullptr;
    const bf16_t* dout = nullptr;
    const float *inp = nullptr, *w = nullptr, *mean = nullptr, *rstd = nullptr;
    long long rows = 0;
    int C = 0;
    // stochastic depth (both or neither): dres_out is also the upstream gradient of a residual
    // branch scaled per row in the forward: dres_scaled = bf16(fl32(row_scale[r] * dres_out)) (a bf16 plane
    // of its own, the branch's GEMM operand) and dres_colsum sums those fp32 products; dres_out / lo_out
    // (the pass-through gradient) keep the bits of the plain form
    bf16_t* dres_scaled = nullptr;
    const float* row_scale = nullptr;
    // fp8 (any of qr / slr / qc / slc set; gemm_fp8.hip, C a multiple of 256 up to 1280: ln_backward_mx_supported):
    // plus both MX forms of dres_out's bf16 plane, as quantize_mx_rowcol_bf16 writes them.  scratch:
    // ln_backward_mx_scratch_bytes(C) (nullptr: the thread workspace; a caller with work in flight on other
    // streams passes its own)
    uint8_t *qr = nullptr, *slr = nullptr, *qc = nullptr, *slc = nullptr;
    long long ldqc = 0, tok_off = 0, ntok = 0;
    uint8_t* scratch = nullptr;
    bool mx() const { return qr || slr || qc || slc; }
};
// the plain, row-scaled or MX kernel by which optional parts are set (false + set_error on a bad call)
bool ln_backward_stream(const LnbArgs& a, hipStream_t s);
bool ln_backward_stream_mx(const LnbArgs& a, hipStream_t s);  // gemm_fp8.hip: the MX form's kernel, for the launcher
int ln_bwd_blocks(long long rows);
void convert_f2bf(bf16_t* out, const float* inp, long long n, hipStream_t s);
// e = ema_blend(e, p) over n elements on s (the body of ema_update, include/vit_ops.h; common.h ema_blend)
void ema_update_on(float* e, const float* p, long long n, float d, float omd, hipStream_t s);
// out = fl32(a + b) over n elements on s (the body of grad_accumulate, include/vit_ops.h); out may be a or b
void grad_accumulate_on(float* out, const float* a, const float* b, long long n, hipStream_t s);
// sum of squares in double, deterministic (the body of grad_sumsq, include/vit_ops.h):
// sumsq_partials writes sumsq_blocks(n) per-workgroup partial sums (a function of n alone; 0 for
// n <= 0, then nothing is launched) to slots; sumsq_finish / clip_finish sum nslots of them in slot
// order with one workgroup into out[0] / into the clip record {S, norm, c} for max_norm
int sumsq_blocks(long long n);
void sumsq_partials(double* slots, const float* x, long long n, hipStream_t s);
void sumsq_finish(double* out, const double* slots, int nslots, hipStream_t s);
void clip_finish(ClipRec* rec, const double* slots, int nslots, float max_norm, hipStream_t s);
void softmax_rows(float* probs, const float* logits, long long rows, int V, hipStream_t s);
void ce_forward(float* losses, const float* probs, const int* targets, long long rows, int V,
                hipStream_t s);
void ce_backward(float* dlogits, const float* dlosses, const float* probs, const int* targets,
                 long long rows, int V, hipStream_t s);
// soft targets t = (1-eps) (lam 1[ta] + (1-lam) 1[tb]) + eps/V (tb nullable = ta): probs (the bits
// softmax_rows writes) and losses = lse(z) - t.z in one kernel (losses nullable = softmax_rows);
// dlogits += (probs - t) * dlosses
void softmax_ce_soft(float* probs, float* losses, const float* logits, const int* ta, const int* tb,
                     float lam, float eps, long long rows, int V, hipStream_t s);
void ce_soft_backward(float* dlogits, const float* dlosses, const float* probs, const int* ta,
                      const int* tb, float lam, float eps, long long rows, int V, hipStream_t s);
// batch mixing in place on px [B,3,IMG,IMG], image i with image B-1-i (the middle image of an odd B
// is left as it is); both also write labels_b[r] = labels[B-1-r] when they launch.
// mixup: x_i' = rn(rn(lam x_i) + rn((1-lam) x_j));  cutmix: the box [x0,x1) x [y0,y1) of every
// channel plane is swapped (the caller checks it lies inside the image; an empty box launches nothing)
void mixup_batch(float* px, int* labels_b, const int* labels, int B, int IMG, float lam, hipStream_t s);
void cutmix_batch(float* px, int* labels_b, const int* labels, int B, int IMG, int x0, int y0, int x1,
                  int y1, hipStream_t s);
void im2col_f32(float* out, const float* px, int B, int IMG, int P, hipStream_t s);
void im2col_bf16(bf16_t* out, const float* px, int B, int IMG, int P, hipStream_t s);
// rows padded to KPP columns (zeros past 3*P*P; KPP % 8 == 0): the bf16 GEMM operand of a patch
// whose 3*P*P is not a multiple of 8 (ViT-H/14: 588 -> 640)
void im2col_pad_bf16(bf16_t* out, const float* px, int B, int IMG, int P, int KPP, hipStream_t s);
void patch_assemble(float* enc, const float* emb, const float* cls, const float* wpe, int B,
                    int NP, int C, hipStream_t s);
// out[c][r] = in[r][c] for `count` R x Cc bf16 matrices `stride` elements apart (in and out)
void transpose_bf16(bf16_t* out, const bf16_t* in, int R, int Cc, int count, long long stride,
                    hipStream_t s);
void patch_gather_f32(float* out, const float* denc, int B, int NP, int C, hipStream_t s);
void patch_gather_bf16(bf16_t* out, const float* denc, int B, int NP, int C, hipStream_t s);
void patch_gather_bf16(bf16_t* out, const bf16_t* denc, int B, int NP, int C, hipStream_t s);
// dcls += sum_b denc[b,0];  dwpe[t] += sum_b denc[b,t];  dpb += sum_{b,t>0} denc[b,t] — fixed order
// (no atomics); ws (nullable = thread workspace): T*C floats of per-position sums
void patch_small_grads(float* dcls, float* dwpe, float* dpb, const float* denc, int B, int T,
                       int C, hipStream_t s, float* ws = nullptr);
// part (nullable): PSG_CHUNKS * T * C floats of per-image-chunk partial sums (the chunked form)
constexpr int PSG_CHUNKS = 16;
void patch_small_grads(float* dcls, float* dwpe, float* dpb, const bf16_t* denc, const uint8_t* lo, int B, int T,
                       int C, hipStream_t s, float* ws = nullptr, float* part = nullptr);
// attention.hip
void attn_forward_f32(float* out, float* preatt, float* att, const float* inp, int B, int T, int C,
                      int NH, hipStream_t s);
void attn_backward_f32(float* dinp, float* dpreatt, float* datt, const float* dout,
                       const float* inp, const float* att, int B, int T, int C, int NH,
                       hipStream_t s);
bool attn_fused_supported(int T, int C, int NH);
bool attn_generic_supported(int T, int C, int NH);  // VALU bf16 kernels (other head sizes, T > 256)
void attn_forward_fused(bf16_t* out, float* lse, const bf16_t* qkv, int B, int T, int C, int NH,
                        hipStream_t s);
// dqkv_colsum (nullable, [3C]) += column sums of dqkv (the qkv bias gradient, fused, fixed order);
// colsum_store: dqkv_colsum = the sums instead (a per-micro-batch partial row the trainer reduces)
// floats of the workspace attn_backward_fused needs (generic delta rows / fused column-sum partials)
size_t attn_backward_ws_floats(int B, int T, int C, int NH);
void attn_backward_fused(bf16_t* dqkv, const bf16_t* dout, const bf16_t* qkv, const bf16_t* out,
                         const float* lse, int B, int T, int C, int NH, hipStream_t s,
                         float* dqkv_colsum = nullptr, float* ws = nullptr, bool colsum_store = false);
// ws (nullable = thread workspace): B*NH*192 floats — per-(b,h) bias partial sums
}  // namespace vit
