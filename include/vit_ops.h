/*
 * vit_ops.h — C ABI of libvit_hip.so: the reference's layer ops as MI355X (gfx950) HIP kernels.
 *
 * Drop-in boundary.  The reference's layer ops are the free functions of
 * /root/reference/train_vit.rs:376-670 (raw *mut f32 / *const f32 + c_int dims).  Each symbol
 * below keeps the reference's name, argument order (outputs, inputs/weights, dims) and write
 * semantics, with DEVICE pointers:
 *   - forward ops OVERWRITE their outputs; backward ops ACCUMULATE (+=) into dinp/dweight/dbias
 *     (train_vit.rs:524-525, 538, 549, 552, 578-579, 587, 595-596, 626-633, 650);
 *   - a NULL bias means "no bias" (train_vit.rs:388, 548);
 *   - the caller owns every buffer (ops never allocate caller-visible memory);
 *   - ops are enqueued on the calling thread's stream (vit_set_stream); with VIT_SYNC=1 in the
 *     environment every op synchronises before returning, restoring the reference's
 *     synchronous semantics;
 *   - the reference ops return () and have no error channel: failures (bad shapes, HIP errors)
 *     set a sticky thread-local error read with vit_last_error().
 * Semantic fixes relative to the reference text (SURVEY.md §8a defect register) are applied:
 * D1 offsets by T, D2 full normalisation, D3 non-causal attention, D4 GELU derivative,
 * D5 LN backward, D6 -log p loss, D7 patch embedding, D10 64-bit offsets.
 * Activation layouts are the reference's: qkv [B,T,3C] (Q|K|V, head h at h*hs),
 * preatt/att [B,T,NH,T] (row index bth = (b*T+t)*NH+h, train_vit.rs:406-410).
 */
#ifndef VIT_OPS_H
#define VIT_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ context */
int vit_init(int device);                 /* select device; 0 on success */
void vit_set_stream(void* hip_stream);    /* hipStream_t; NULL = default stream */
void* vit_get_stream(void);
int vit_sync(void);                        /* hipStreamSynchronize(current stream) */
int vit_last_error(const char** msg);      /* 0 = no error; sticky until vit_clear_error */
void vit_clear_error(void);
/* device memory helpers for hosts without their own device allocator (ctypes tests, C hosts) */
void* vit_malloc(size_t bytes);
void vit_free(void* p);
int vit_memcpy_h2d(void* dst, const void* src, size_t bytes);
int vit_memcpy_d2h(void* dst, const void* src, size_t bytes);
int vit_memcpy_d2d(void* dst, const void* src, size_t bytes);
int vit_memset(void* dst, int value, size_t bytes);
/* launch counters: how many launches of each kernel family ran since the last reset (process-wide,
 * every thread and stream).  GEMM families are indexed base + epilogue (epi < 16, gemm.h Epi; 12 = the
 * row-scaled residual epilogue of gemm_bf16_fused_rowscale). */
enum {
    VIT_HIT_GEMM_128 = 0,            /* bf16 128x128 register-staged (small / ragged shapes) */
    VIT_HIT_GEMM_256x256 = 16,       /* bf16 256x256 LDS-DMA engine, one workgroup per CU */
    VIT_HIT_GEMM_256x128 = 32,       /* bf16 256x128 LDS-DMA engine, two workgroups per CU */
    VIT_HIT_GEMM_FP8 = 48,           /* MXFP8 256x256 engine */
    VIT_HIT_GEMM_F32 = 64,           /* fp32 MFMA (parity path) */
    VIT_HIT_SPLITK_REDUCE = 80,      /* split-K slab reduction (separate launch) */
    VIT_HIT_ATTN_FWD_MFMA = 81,      /* fused MFMA attention forward */
    VIT_HIT_ATTN_BWD_PERSISTENT = 82,/* persistent one-pass MFMA attention backward */
    VIT_HIT_ATTN_BWD_ONEPASS = 83,   /* one-pass backward, one workgroup per (b,h) */
    VIT_HIT_ATTN_BWD_PAIR = 84,      /* paired-role backward */
    VIT_HIT_ATTN_GENERIC = 85,       /* generic VALU attention (T past the MFMA kernels' LDS) */
    VIT_HIT_ATTN_BWD_XKEY = 86,      /* one-pass backward + the last key's side path (T = 32k + 1) */
    VIT_HIT_QUANT_ROWCOL = 87,       /* fused row + column MX quantization */
    VIT_HIT_GEMM_PP = 88,            /* bf16 two-group ping-pong 192x256 engine (variant 11; also counted as 256x256 + epi) */
    VIT_HIT_LN_MX = 89,              /* LayerNorm forward straight into the row + column MX forms (fp8) */
    VIT_HIT_LNB_MX = 90,             /* LayerNorm backward (residual-gradient stream) + both MX forms (fp8) */
    VIT_HIT_AUGMENT = 91,            /* RandAugment on the uint8 batch: + 0 statistics / LUT, 1 in-place apply,
                                        2 out-of-place apply (sharpness, affine), 3 copy back */
    VIT_HIT_EMA = 95,                /* a launch that advances an EMA of the weights: an optimizer kernel's EMA
                                        instantiation (vit_trainer_set_ema) or ema_update */
    VIT_HIT_ERASE = 96,              /* random erasing on the fp32 batch (vit_random_erase_f32, vit_trainer_erase_batch):
                                        one launch per call that has a non-empty box.  A family of its own: the mix
                                        kernels of vit_trainer_mix_batch are in no family */
    VIT_HIT_SGDM = 97,               /* momentum SGD: every momentum instantiation of the optimizer kernels
                                        (vit_trainer_set_sgd) and sgd_momentum_step */
    VIT_HIT_ACCUM = 98,              /* gradient accumulation: a launch of grad_accumulate's kernel (the op, or the
                                        trainer's sums under vit_trainer_set_grad_accum; its first copy is not one) */
    VIT_HIT_COUNT = 99
};
int vit_kernel_hits(long long* out, int n); /* copies min(n, VIT_HIT_COUNT); returns VIT_HIT_COUNT */
void vit_kernel_hits_reset(void);
/* events for per-kernel timing on the current stream */
void* vit_event_create(void);
void vit_event_destroy(void* ev);
int vit_event_record(void* ev);
float vit_event_elapsed_ms(void* start, void* stop);

/* ------------------------------------------------------------------ reference ops (fp32) */
/* train_vit.rs:376 */
void residual_forward(float* out, const float* inp1, const float* inp2, int N);
/* train_vit.rs:384 — out[BT,OC] = inp[BT,C] . weight[OC,C]^T + bias */
void matmul_forward(float* out, const float* inp, const float* weight, const float* bias,
                    int B, int T, int C, int OC);
/* train_vit.rs:400 (+ attention.rs:1) — preatt/att [B,T,NH,T] are materialised like the
 * reference; either may be NULL (fused use: the scores are then not stored) */
void attention_forward(float* out, float* preatt, float* att, const float* inp,
                       int B, int T, int C, int NH);
/* train_vit.rs:453 */
void layernorm_forward(float* out, float* mean, float* rstd, const float* inp,
                       const float* weight, const float* bias, int B, int T, int C);
/* train_vit.rs:482 */
void gelu_forward(float* out, const float* inp, int N);
/* train_vit.rs:493 */
void softmax_forward(float* probs, const float* logits, int B, int T, int V);
/* rusty_vit.rs:836 (called train_vit.rs:256), D6: losses = -log probs[target] */
void crossentropy_forward(float* losses, const float* probs, const int* targets,
                          int B, int T, int V);
/* train_vit.rs:521 (+=) */
void residual_backward(float* dinp1, float* dinp2, const float* dout, int N);
/* train_vit.rs:530 (+=); dinp NULL skips the input gradient, dbias NULL skips the bias */
void matmul_backward(float* dinp, float* dweight, float* dbias, const float* dout,
                     const float* inp, const float* weight, int B, int T, int C, int OC);
/* train_vit.rs:559 (+=); dpreatt/datt: accumulated [B,T,NH,T] scratch, NULL = internal */
void attention_backward(float* dinp, float* dpreatt, float* datt, const float* dout,
                        const float* inp, const float* att, int B, int T, int C, int NH);
/* train_vit.rs:603 (+=) */
void layernorm_backward(float* dinp, float* dweight, float* dbias, const float* dout,
                        const float* inp, const float* weight, const float* mean,
                        const float* rstd, int B, int T, int C);
/* train_vit.rs:639 (+=), D4 */
void gelu_backward(float* dinp, const float* inp, const float* dout, int N);
/* undefined in the reference, called train_vit.rs:293 (+=): dlogits += (p - 1[tgt]) * dloss */
void crossentropy_softmax_backward(float* dlogits, const float* dlosses, const float* probs,
                                   const int* targets, int B, int T, int V);
/* soft-target loss (no reference counterpart; label smoothing / mixup / cutmix).  Row r has the
 * target distribution t = (1-eps) (lam 1[ta[r]] + (1-lam) 1[tb[r]]) + eps/V; tb NULL = ta.
 * forward: softmax and loss in one kernel: probs = the bits softmax_forward writes,
 *          losses[r] = lse(z) - sum_k t_k z_k, from the logits (finite where a probability
 *          underflows); an out-of-range label gives NaN in that row; losses NULL = softmax_forward.
 * backward (+=): dlogits += (probs - t) * dlosses[r] */
void softmax_crossentropy_soft_forward(float* probs, float* losses, const float* logits,
                                       const int* ta, const int* tb, float lam, float eps,
                                       int B, int T, int V);
void crossentropy_soft_softmax_backward(float* dlogits, const float* dlosses, const float* probs,
                                        const int* ta, const int* tb, float lam, float eps,
                                        int B, int T, int V);
/* ViT replacement of encoder_forward (train_vit.rs:196): pixels [B,3,IMG,IMG] ->
 * encoded [B,T,C], row 0 = cls + wpe[0], row 1+p = patch_p . patch_w^T + patch_b + wpe[1+p] */
void patch_embed_forward(float* encoded, const float* pixels, const float* patch_w,
                         const float* patch_b, const float* cls, const float* wpe,
                         int B, int IMG, int P, int C);
/* ViT replacement of encoder_backward (train_vit.rs:371), (+=), no pixel gradient */
void patch_embed_backward(float* dpatch_w, float* dpatch_b, float* dcls, float* dwpe,
                          const float* dencoded, const float* pixels, int B, int IMG, int P,
                          int C);
/* optimizer_step (train_vit.rs:737): params -= lr * grads */
void sgd_step(float* params, const float* grads, long long n, float lr);
/* torch.optim.SGD's update with momentum, dampening, Nesterov and coupled weight decay (vit_trainer.h
 * vit_trainer_set_sgd), per element, every operation rounded to fp32 on its own (no FMA), with
 * omd = (float)(1.0 - (double)dampening):
 *     g2 = weight_decay != 0 ? g + weight_decay * p : g
 *     b' = first ? g2 : momentum * b + omd * g2      (first: buf is seeded with g2's bits, its old values ignored)
 *     d  = nesterov ? g2 + momentum * b' : b'
 *     p' = p - lr * d
 * Device pointers, any n >= 0, any 4-byte alignment: the scalar form of the element function the trainer's
 * momentum kernels run.  Every value must be finite, momentum and weight_decay >= 0, and nesterov needs
 * momentum > 0 and dampening == 0 (torch's rule).  No reference counterpart: the reference's SGD is sgd_step. */
void sgd_momentum_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening,
                       float weight_decay, int nesterov, int first);
/* out[0] = sum_i x[i]^2: every square and every sum in double; device pointers; any n >= 0
 * (n == 0 gives 0).  No reference counterpart: the reduction behind the trainer's global-norm
 * gradient clipping (vit_trainer_set_grad_clip), which runs this kernel body per gradient chunk.
 * Deterministic: per-workgroup partial sums (their number a function of n alone) combined in a
 * fixed order, no floating-point atomics: two calls on the same buffer give the same bits. */
void grad_sumsq(double* out, const float* x, long long n);
/* ema[i] = fl32( fl32(decay * ema[i]) + fl32(omd * params[i]) ) for i < n, omd = (float)(1.0 - (double)decay):
 * numpy's fp32 `decay * ema + omd * params`, each product and the sum rounded on its own (no FMA).  Device
 * pointers, any n >= 0; 16-byte accesses over n / 4 float4s when both pointers are 16-byte aligned and a
 * scalar tail for n % 4 (all scalar otherwise).  No reference counterpart: the update the trainer's optimizer
 * kernels fuse for vit_trainer_set_ema, stand-alone; fp32-mode SGD launches it. */
void ema_update(float* ema, const float* params, long long n, float decay);
/* out[i] = fl32(a[i] + b[i]) for i < n: one fp32 addition per element, numpy's fp32 `a + b`.  Device pointers,
 * any n >= 0 (n == 0 launches nothing), any 4-byte alignment.  out may be exactly a or exactly b (an in-place
 * sum); any other overlap of out with an input is an error.  16-byte accesses over n / 4 float4s when all three
 * pointers are 16-byte aligned and a scalar tail for n % 4 (all scalar otherwise): the same values either way.
 * No atomics.  No reference counterpart: the summing pass of the trainer's gradient accumulation
 * (vit_trainer_set_grad_accum), stand-alone. */
void grad_accumulate(float* out, const float* a, const float* b, long long n);
/* One LAMB step (vit_trainer.h vit_trainer_step_lamb) of one tensor as one segment: m, v
 * advanced as AdamW's step t does, u = mh / (sqrt(vh) + eps) + weight_decay * p, the norms of p and u in double
 * (fixed order), r = |p| / |u| where the tensor is adapted (weight_decay != 0, or flags & 1 = always adapt) and
 * both norms are positive, else 1; flags & 2 caps r at 1; p -= (lr * r) * u.  Device pointers, any n >= 1, any
 * 4-byte alignment; the element functions and the order of the sums per 4096-element tile are the trainer's.
 * info (device, nullable) receives {|p|, |u|, r}.  t >= 1.  No reference counterpart: the reference trains
 * with SGD only. */
void lamb_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int t, int flags, float* info);

/* ------------------------------------------------------------------ bf16 fast path
 * Build-side extensions with the same conventions; bf16 storage as raw uint16_t, fp32
 * accumulate; LN statistics, biases, residual stream and gradients stay fp32.           */
/* out_bf16[BT,OC] = inp . W^T + bias */
void matmul_forward_bf16(uint16_t* out, const uint16_t* inp, const uint16_t* weight,
                         const float* bias, int B, int T, int C, int OC);
/* dinp_f32 += dout . W (NULL skips);  dweight_f32 += dout^T . inp (split-K, atomics) */
void matmul_backward_bf16(float* dinp, float* dweight, float* dbias, const uint16_t* dout,
                          const uint16_t* inp, const uint16_t* weight, int B, int T, int C,
                          int OC);
/* fused attention: out_bf16 [B,T,C], lse [B,NH,T] (log2 domain), no T x T HBM traffic.
 * Head sizes 32/64/80/96/128 run the MFMA kernels while the head's operands fit the LDS
 * (T <= 320; <= 288 at head size 128), e.g. ViT-B/16 (hs 64, T 197) and ViT-H/14 (hs 80,
 * T 257); longer sequences run generic VALU kernels with the same outputs; other shapes set
 * vit_last_error.  vit_attention_kernel_kind: 1 = MFMA, 2 = generic, 0 = unsupported. */
int vit_attention_kernel_kind(int T, int C, int NH);
void attention_forward_fused_bf16(uint16_t* out, float* lse, const uint16_t* inp,
                                  int B, int T, int C, int NH);
/* dinp_bf16 [B,T,3C] is OVERWRITTEN (it is produced whole); recomputes P from lse */
void attention_backward_fused_bf16(uint16_t* dinp, const uint16_t* dout, const uint16_t* inp,
                                   const uint16_t* out, const float* lse, int B, int T, int C,
                                   int NH);
/* As attention_backward_fused_bf16, plus the fused qkv-bias gradient the trainer uses:
 * dqkv_bias[j] += sum over the B*T rows of dinp[row][j] (fp32 sums of the unrounded values,
 * deterministic order), j < 3C.  dqkv_bias may be NULL. */
void attention_backward_fused_bf16_ex(uint16_t* dinp, const uint16_t* dout, const uint16_t* inp,
                                      const uint16_t* out, const float* lse, int B, int T, int C, int NH,
                                      float* dqkv_bias);
void layernorm_forward_bf16(uint16_t* out, float* mean, float* rstd, const float* inp,
                            const float* weight, const float* bias, int B, int T, int C);
/* train_vit.rs:603 with the LN-output gradient in bf16 (as the trainer's dgrad GEMMs write it):
 * dinp, dweight, dbias (fp32) += */
void layernorm_backward_bf16(float* dinp, float* dweight, float* dbias, const uint16_t* dout,
                             const float* inp, const float* weight, const float* mean,
                             const float* rstd, int B, int T, int C);
/* train_vit.rs:482 / :639 (D4) in the form the fused GEMM epilogues use (logistic tanh, raw
 * v_exp / v_rcp): out_bf16 = gelu(inp_bf16); dinp_f32 += gelu'(inp_bf16) * dout_bf16 */
void gelu_forward_bf16(uint16_t* out, const uint16_t* inp, int N);
void gelu_backward_bf16(float* dinp, const uint16_t* inp, const uint16_t* dout, int N);
/* generic bf16 GEMM (the engine under matmul_*_bf16), for tests and tools:
 * C[M,N] (epilogue)= A . B with A(m,k) = a_kcontig ? A[m*lda+k] : A[k*lda+m],
 * B(k,n) = b_kcontig ? B[n*ldb+k] : B[k*ldb+n].  epi: 0 f32 store, 1 f32 +=, 2 f32 atomic +=
 * (split-K), 3 bf16 store; bias (nullable) is added for 0/1/3; dbias (nullable, epi 2 with an
 * M-contig A) receives the row sums of A. */
void gemm_bf16_ex(void* C, long long ldc, const uint16_t* A, long long lda, int a_kcontig,
                  const uint16_t* B, long long ldb, int b_kcontig, const float* bias,
                  float* dbias, int M, int N, int K, int epi, int splitk);
/* gemm_bf16_ex (no bias / dbias) with the caller's promise that rows k of an M-contiguous A with
 * k % k_period != 0 are exact zeros (k_period 0: none).  The split-K weight-gradient engine
 * (epi 2, M-contiguous A, N-contiguous B, K % 32 == 0, M >= 256, N >= 128) then skips the 32-row
 * K-steps that hold no row i * k_period when k_period > 32; the result has the bits of the dense
 * call.  Every other engine and period runs dense. */
void gemm_bf16_kperiod(void* C, long long ldc, const uint16_t* A, long long lda, int a_kcontig,
                       const uint16_t* B, long long ldb, int b_kcontig, int M, int N, int K, int epi,
                       int splitk, int k_period);
/* the fused epilogues of the trainer's GEMMs: epi 4 C = pre = acc + bias, C2 = gelu(pre)
 * (both bf16); 5 C_f32 = acc + bias + aux_f32; 6 C_bf16 = acc * gelu'(aux_bf16) and, when
 * colsum_out is not NULL, colsum_out[n] += sum_m C[m][n]; 0 / 3 as gemm_bf16_ex.  The pair the
 * trainer uses for the MLP (fc forward -> fcproj dgrad): epi 8 C = gelu'(pre), C2 = gelu(pre)
 * (both bf16, pre = acc + bias, one sigmoid for both); 9 C_bf16 = acc * aux_bf16 (aux = the
 * stored gelu') with the colsum_out of epi 6. */
void gemm_bf16_fused(void* C, void* C2, long long ldc, const void* aux, long long ldaux,
                     const uint16_t* A, long long lda, int a_kcontig, const uint16_t* B,
                     long long ldb, int b_kcontig, const float* bias, float* colsum_out, int M,
                     int N, int K, int epi);
/* gemm_bf16_fused on a strided selection of rows (lda / ldc / ldaux = a multiple of the dense pitch).
 * rows_gathered: the call keeps the 256x256 engine of the dense tensor's other GEMMs for any M >= 1
 * (N >= 256, K % 64 == 0, K-contiguous A).  colsum_row_period = p > 0 (epi 6 / 9 of such a call, p >= 128,
 * N % 8 == 0; an error otherwise): output row m is row m * p of a dense tensor whose other rows are
 * exact zeros, and colsum_out receives what the dense M * p row call would add, bit for bit. */
void gemm_bf16_fused_rows(void* C, void* C2, long long ldc, const void* aux, long long ldaux,
                          const uint16_t* A, long long lda, int a_kcontig, const uint16_t* B,
                          long long ldb, int b_kcontig, const float* bias, float* colsum_out, int M,
                          int N, int K, int epi, int rows_gathered, int colsum_row_period);
/* gemm_bf16_fused_rows with epi 12, the row-scaled residual epilogue of stochastic depth
 * (vit_trainer_set_drop_path): C_f32[m][n] = aux_f32[m*ldaux + n] + fl32(row_scale[m * ld_row_scale] *
 * (acc + bias[n])), the product rounded to fp32 on its own (no FMA), so row_scale == 1 gives the bits of
 * epi 5 and row_scale == 0 gives C == aux.  row_scale: fp32 device pointer; a row-gathered call passes the
 * dense per-row table with ld_row_scale = the rows' stride.  colsum_out must be NULL and
 * colsum_row_period 0 (the epilogue sums no columns); C2 is unused.  Runs on the 128x128 engine and both
 * 256x256 forms; the ping-pong engine of variant 11 declines it (the call then takes the default engine). */
void gemm_bf16_fused_rowscale(void* C, void* C2, long long ldc, const void* aux, long long ldaux,
                              const uint16_t* A, long long lda, int a_kcontig, const uint16_t* B,
                              long long ldb, int b_kcontig, const float* bias, float* colsum_out, int M,
                              int N, int K, int epi, int rows_gathered, int colsum_row_period,
                              const float* row_scale, long long ld_row_scale);
/* ------------------------------------------------------------------ fp8 (MXFP8) GEMM path
 * OCP fp8 e4m3 operands with one E8M0 scale per 32 consecutive k-elements of a row (OCP MX block
 * scaling) on v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulate: the fp8 mode's forward and
 * input-gradient GEMMs (matmul_forward, train_vit.rs:384; dinp of matmul_backward, :530-541).
 * Scales use the lane-native layout [K/64][Rpad/32][64] bytes (Rpad = rows rounded up to 256;
 * byte h*32 + r of row group g at step s scales row 32g + r, k-block 2s + h): mx_scale_size
 * bytes per operand.  quantize_mx_*: x [R][K] (row stride ldx elements, K % 64 == 0) -> q [R][K]
 * e4m3 (row stride ldq bytes) + scales; scale 2^X with X = ceil(log2(amax / 448)) per block,
 * x * 2^-X rounded to nearest even.  gemm_fp8_fused: C = A . B^T with A [M][K], B [N][K]
 * (K-contiguous bytes) and the epilogues of gemm_bf16_fused (epi 0, 1, 2, 3, 4, 5, 6, 8, 9; epi 2 =
 * C += A . B^T through K-split fp32 slabs and a fixed-order reduce: the fp8 weight gradient of
 * matmul_backward, train_vit.rs:543-555, with A / B from quantize_mx_cols_bf16_ex). */
long long mx_scale_size(long long rows, int K);
void quantize_mx_bf16_ex(uint8_t* q, uint8_t* scales, const uint16_t* x, long long R, int K,
                         long long ldx, long long ldq);
void quantize_mx_f32_ex(uint8_t* q, uint8_t* scales, const float* x, long long R, int K,
                        long long ldx, long long ldq);
/* column-wise MX (blocks of 32 consecutive ROWS of x: the token axis a weight gradient reduces
 * over): x [R][C] bf16 (row stride ldx, C % 64 == 0) -> q [C][Kp] e4m3, Kp = mx_cols_padded(R)
 * (R rounded up to 64, padding tokens zero) + scales (mx_scale_size(C, Kp) bytes); equal, byte for
 * byte, to quantize_mx_bf16_ex of the zero-padded transpose. */
long long mx_cols_padded(long long R);
void quantize_mx_cols_bf16_ex(uint8_t* q, uint8_t* scales, const uint16_t* x, long long R, int C,
                              long long ldx);
/* both forms in one read of x [R][C] (row stride ldx): qr [R][C] + scales_r exactly as
 * quantize_mx_bf16_ex(qr, scales_r, x, R, C, ldx, C), and the column form of tokens
 * [tok_off, tok_off + ntok) of a [C][ldqc] matrix + scales_c (mx_scale_size(C, ldqc) bytes) exactly
 * as the same span of quantize_mx_cols_bf16_ex over the whole token axis; tok_off % 64 == 0,
 * R <= ntok <= R rounded up to 64 (tokens R .. ntok-1 are zero padding). */
void quantize_mx_rowcol_bf16_ex(uint8_t* qr, uint8_t* scales_r, uint8_t* qc, uint8_t* scales_c,
                                const uint16_t* x, long long R, int C, long long ldx, long long ldqc,
                                long long tok_off, long long ntok);
/* LayerNorm forward (train_vit.rs:453-480) straight into both MX forms: exactly
 * layernorm_forward_bf16 (mean / rstd as it writes them) followed by quantize_mx_rowcol_bf16_ex of
 * its bf16 output, without the bf16 tensor; inp [R][C] fp32, C a multiple of 256 in 256 .. 2048
 * (not 1792). */
/* the trainer's residual-gradient LayerNorm backward (train_vit.rs:603-637 + the residual add,
 * "bf16 + lo8" planes: dres_out = dres_in + LN_dinp(dout); dweight / dbias / dres_colsum (nullable)
 * += the column sums of dout * xhat / dout / dres_out in a fixed order) ... */
void layernorm_backward_stream(uint16_t* dres_out, uint8_t* lo_out, const uint16_t* dres_in, const uint8_t* lo_in,
                               float* dweight, float* dbias, float* dres_colsum, const uint16_t* dout, const float* inp,
                               const float* weight, const float* mean, const float* rstd, long long R, int C);
/* ... and the same with both MX forms of dres_out's bf16 plane written beside it (exactly
 * quantize_mx_rowcol_bf16_ex of dres_out; the column sums group rows differently: equal within fp32
 * rounding, not bitwise); C a multiple of 256 in 256 .. 1280 */
void layernorm_backward_stream_mx(uint16_t* dres_out, uint8_t* lo_out, const uint16_t* dres_in, const uint8_t* lo_in,
                                  float* dweight, float* dbias, float* dres_colsum, const uint16_t* dout,
                                  const float* inp, const float* weight, const float* mean, const float* rstd,
                                  long long R, int C, uint8_t* qr, uint8_t* scales_r, uint8_t* qc, uint8_t* scales_c,
                                  long long ldqc, long long tok_off, long long ntok);
void layernorm_forward_mx(uint8_t* qr, uint8_t* scales_r, uint8_t* qc, uint8_t* scales_c, float* mean,
                          float* rstd, const float* inp, const float* weight, const float* bias, long long R,
                          int C, long long ldqc, long long tok_off, long long ntok);
void gemm_fp8_fused(void* C, void* C2, long long ldc, const void* aux, long long ldaux,
                    const uint8_t* A, const uint8_t* a_scale, long long lda, const uint8_t* B,
                    const uint8_t* b_scale, long long ldb, const float* bias, float* colsum_out,
                    int M, int N, int K, int epi);
/* gemm_fp8_fused with the fused MX copy of the bf16 output (epi 4 / 8: the GELU output C2; epi 6 / 9: C):
 * mx_q [M][N] e4m3 (ld N), mx_s lane-native scales for mx_rows_padded(M) rows, bit-identical to
 * quantize_mx_bf16_ex of that bf16 output (padding rows' scales are left as given). */
void gemm_fp8_fused_mx(void* C, void* C2, long long ldc, const void* aux, long long ldaux, const uint8_t* A,
                       const uint8_t* a_scale, long long lda, const uint8_t* B, const uint8_t* b_scale,
                       long long ldb, const float* bias, float* colsum_out, int M, int N, int K, int epi,
                       uint8_t* mx_q, uint8_t* mx_s);
/* gemm_fp8_fused_mx plus the column-wise MX copy of the same output (the weight gradient's
 * operand): output row m -> token mxc_off + m of mxc_q [N][mxc_ld] + scales mxc_s
 * (mx_scale_size(N, mxc_ld) bytes), equal byte for byte to quantize_mx_cols_bf16_ex of the bf16
 * output; M % 64 == 0, N % 64 == 0, mxc_off % 64 == 0.  The MX-copied bf16 output (C2 of epi 4 / 8,
 * C of epi 6 / 9) may be NULL: not stored. */
void gemm_fp8_fused_mxc(void* C, void* C2, long long ldc, const void* aux, long long ldaux, const uint8_t* A,
                        const uint8_t* a_scale, long long lda, const uint8_t* B, const uint8_t* b_scale,
                        long long ldb, const float* bias, float* colsum_out, int M, int N, int K, int epi,
                        uint8_t* mx_q, uint8_t* mx_s, uint8_t* mxc_q, uint8_t* mxc_s, long long mxc_ld,
                        long long mxc_off);
/* tools: GEMM engine selection (0 or any other number = the default; 1 = 128x128 everywhere,
 * 2 = 256x256 one tile per workgroup with the split-K weight gradients on 256x128, 7 = production:
 * 2 with the persistent streaming 256x256 engine for the K-contiguous GEMMs, 11 = 7 with the
 * ping-pong 192x256 engine for the shapes it takes) and diagnostics (flag 2: skip epilogues, main-loop
 * timing only; flag 16: the persistent engine drains its stores after each epilogue; flag 32: every
 * output row stored onto row 0 (timing only, wrong outputs: no HBM write traffic); (flags >> 8) &
 * 0xFF: first-round stagger in 0.5 us units; (flags >> 16) & 0xF = g + 1: persistent-engine tile
 * groups of g row panels, 0 = column-major ... default 8 for K <= 768, else row-major) */
void gemm_bf16_set_variant(int variant);
void gemm_bf16_set_debug(int flags);
/* diagnostic: per-workgroup timestamps of the 256x256 bf16 engines into trace (device,
 * 16 x u64 per workgroup of the next launches, 100 MHz s_memrealtime: 0 start, 1 main-loop end,
 * 2 end of wave 0, 3 hardware id = XCC_ID << 32 | HW_ID, 4 + w end of wave w, 12 first K-step's
 * operands landed); NULL turns it off */
void gemm_bf16_set_trace(unsigned long long* trace);
/* ------------------------------------------------------------------ random erasing
 * timm's RandomErasing on a normalised fp32 batch: dev_pixels [batch][3][img][img] (device, any 4-byte
 * alignment), in place, on stream (a hipStream_t; NULL = the context stream).  host_boxes
 * [batch][max_count][4] = x0, y0, x1, y1 per box, the box being [x0, x1) x [y0, y1) of all three channel
 * planes; a box with x0 == x1 or y0 == y1 is empty.  Pixels outside every box keep their bits.  Inside:
 *   VIT_ERASE_CONST  +0.0f;
 *   VIT_ERASE_PIXEL  z(p) at the absolute position p = (c * img + y) * img + x of the image, so overlapping
 *                    boxes agree and a pixel's value does not depend on the box that covers it;
 *   VIT_ERASE_RAND   one colour per box and channel: z(3 * img * img + 3 * k + c) for box k (where boxes
 *                    overlap, the colour of the box with the largest k, as erasing them in order gives).
 * Every covered pixel is written once, by the last box that covers it.
 * z(p) of image b: sn = seed ^ splitmix64(0x65726e6f697365 (ASCII "ernoise"), host_keys[b]) (the counter-form
 * splitmix64 of vit_drop_path_draw), w = the word of the stream sn at position p, and in double
 *   u1 = ((w >> 40) + 1) * 2^-24                 in (0, 1]
 *   u2 = ((w >> 16) & 0xFFFFFF) * 2^-24          in [0, 1)
 *   z  = (float)( sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2) )
 * Box-Muller with every operation one rounded double operation and one rounding to fp32 (no FMA can form),
 * so the result depends on (seed, key, p) alone: not on the batch, the slot or the box.
 * The host validates everything before any GPU work: a box not 0 <= x0 <= x1 <= img, 0 <= y0 <= y1 <= img,
 * max_count outside 1..4, an unknown mode, host_keys == NULL in a noise mode (CONST may pass NULL), img
 * outside 1..8192 or more than 65535 boxes return non-zero with vit_last_error and leave the batch
 * untouched.  The non-empty boxes go to the device as one small asynchronous copy and one launch covers
 * them all; a call without a non-empty box launches nothing.  Returns once the host arrays have been
 * read. */
enum { VIT_ERASE_CONST = 0, VIT_ERASE_RAND = 1, VIT_ERASE_PIXEL = 2 };
int vit_random_erase_f32(float* dev_pixels, int batch, int img, const int* host_boxes, int max_count, int mode,
                         unsigned long long seed, const long long* host_keys, void* stream);
void convert_f32_to_bf16(uint16_t* out, const float* inp, long long n);
void convert_bf16_to_f32(float* out, const uint16_t* inp, long long n);

#ifdef __cplusplus
}
#endif
#endif
