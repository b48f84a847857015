/*
 * vit_trainer.h — C ABI of the native host trainer in libvit_hip.so.
 *
 * Mirrors the reference's model-level interface (/root/reference/train_vit.rs):
 *   struct ViT + build_from_checkpoint (:65-186)  -> vit_trainer_create + vit_trainer_set_params
 *   ViT::forward(inputs, targets, B, T) (:188)     -> vit_trainer_set_batch + vit_trainer_forward
 *   ViT::backward() (:271)                         -> vit_trainer_zero_grad + vit_trainer_backward
 *   optimizer_step(&mut ViT, lr) (:737)            -> vit_trainer_step
 *   mean_loss field (:85, :263)                    -> vit_trainer_mean_loss
 * Parameters cross this boundary in the reference's canonical type-major order (the 16
 * ParameterTensors of train_vit.rs:10-27 / param_sizes :115-131, with wte -> patch_w, patch_b,
 * cls and the tied LM head -> head_w, head_b; 20 tensors).  On the device the trainer keeps them
 * layer-major in reverse layer order so that backward finalises one contiguous gradient range per
 * layer (the unit of the overlapped RCCL all-reduce).
 *
 * Precision modes:
 *   VIT_FP32 (0): the reference op sequence on the GPU (the fp32 C-ABI ops of vit_ops.h,
 *                 materialised attention) — the parity path (<= 1e-4 rel vs the CPU oracle).
 *   VIT_BF16 (1): the fast path — bf16 MFMA GEMMs with fused epilogues, fused attention,
 *                 fp32 master weights / gradients / residual stream / LN statistics.
 *                 Head sizes 32/64/80/96/128 use the MFMA attention while T <= 320 (generic
 *                 VALU kernels beyond), and a patch whose 3*P*P is not a multiple of 8 runs the
 *                 patch embedding on the fp32 GEMM.
 *   VIT_FP8 (2):  BASELINE config 5 ("fp8 weights/activations"): VIT_BF16 with the forward and
 *                 input-gradient GEMMs of every layer (qkv, proj, fc, fcproj) on MXFP8 operands
 *                 (OCP e4m3 + one E8M0 scale per 32 k-elements, v_mfma_scale_f32_32x32x64_f8f6f4);
 *                 weights quantized from the fp32 master after every optimizer step, activations /
 *                 output gradients quantized as each GEMM consumes them.  Weight gradients,
 *                 attention, LayerNorm, the residual stream and the optimizer stay bf16 / fp32.
 *                 Needs C % 64 == 0.
 * All calls are asynchronous on the trainer's stream unless noted; functions returning int
 * return 0 on success (details via vit_last_error()).
 */
#ifndef VIT_TRAINER_H
#define VIT_TRAINER_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int img, patch, in_ch, channels, num_layers, num_heads, num_classes;
} vit_config_t;

enum { VIT_FP32 = 0, VIT_BF16 = 1, VIT_FP8 = 2 };
enum { VIT_MIX_NONE = 0, VIT_MIX_MIXUP = 1, VIT_MIX_CUTMIX = 2 };  /* vit_trainer_mix_batch modes */
enum { VIT_NUM_PARAM_TENSORS = 20 };
enum { VIT_MAX_LAYERS = 64 };  /* num_layers range accepted by vit_trainer_create / vit_layout_query */

typedef struct vit_trainer vit_trainer_t;

vit_trainer_t* vit_trainer_create(const vit_config_t* cfg, int batch, int precision, int device);
void vit_trainer_destroy(vit_trainer_t* t);
long long vit_trainer_num_params(const vit_trainer_t* t);
/* bytes of device memory held by the trainer */
long long vit_trainer_device_bytes(const vit_trainer_t* t);
/* canonical (type-major) fp32 host arrays of vit_trainer_num_params() elements; synchronous */
int vit_trainer_set_params(vit_trainer_t* t, const float* host_params);
int vit_trainer_get_params(vit_trainer_t* t, float* host_params);
int vit_trainer_get_grads(vit_trainer_t* t, float* host_grads);
/* pixels [batch,3,img,img] fp32, labels [batch] int32 (host); synchronous upload.
 * labels NULL = a forward-only batch (the reference's targets == null branch, train_vit.rs:
 * 254-266): no loss, vit_trainer_mean_loss returns -1, vit_trainer_backward fails */
int vit_trainer_set_batch(vit_trainer_t* t, const float* host_pixels, const int* host_labels);
/* same from device pointers (stream-ordered device copy) */
int vit_trainer_set_batch_device(vit_trainer_t* t, const float* dev_pixels, const int* dev_labels);
/* ---- soft targets: label smoothing, mixup and cutmix on the device batch.  Row r of the loss has
 *      the target distribution t = (1-eps) (lam 1[labels[r]] + (1-lam) 1[labels[B-1-r]]) + eps/V
 *      (lam = 1 for an unmixed batch); loss = lse(logits) - t . logits, dlogits = (probs - t) dloss.
 *      With eps == 0 and no mix the head issues exactly the hard-label launches. ---- */
/* 0 <= eps < 1 (default 0); persists across batches; a hyper-parameter, not written to checkpoints */
int vit_trainer_set_label_smoothing(vit_trainer_t* t, float eps);
/* mix the current device batch in place, image i with image B-1-i (for odd B the middle image is
 * left as it is); call after any vit_trainer_set_batch* variant; asynchronous on the trainer's
 * stream.  The batch stays mixed until the next set_batch*.
 *   VIT_MIX_NONE:   no-op;
 *   VIT_MIX_MIXUP:  x_i' = lam x_i + (1-lam) x_j with lam in [0,1], every product and the sum
 *                   rounded to fp32 on its own (no FMA), 1-lam taken in fp32;
 *   VIT_MIX_CUTMIX: the box [x0,x1) x [y0,y1) (inside the image; may be empty) of all three channel
 *                   planes is swapped between i and j; the lam argument is ignored and
 *                   lam = 1 - box_area / img^2 (in double, rounded to float) weighs the labels.
 * A mix with lam == 1 leaves the targets hard.  Non-zero (with vit_last_error) on a bad argument,
 * a batch without labels, or a second mix of the same batch; the batch is then left as it was. */
int vit_trainer_mix_batch(vit_trainer_t* t, int mode, float lam, int x0, int y0, int x1, int y1);
/* the current device batch [batch,3,img,img] fp32 (mixed or not) to the host; synchronous */
int vit_trainer_get_pixels(vit_trainer_t* t, float* host);
/* forward; b_global = global batch of the data-parallel job (dloss = 1/b_global, D15) */
int vit_trainer_forward(vit_trainer_t* t, int b_global);
int vit_trainer_zero_grad(vit_trainer_t* t);
int vit_trainer_backward(vit_trainer_t* t);   /* also launches the overlapped all-reduce (DP) */
int vit_trainer_step(vit_trainer_t* t, float lr); /* waits for the all-reduce, then SGD */
/* AdamW: the update the reference's m_memory / v_memory (train_vit.rs:73-74)
 * were allocated for, which its SGD optimizer_step (:737) never runs.  t = number of AdamW steps
 * so far + 1 (kept by the trainer, saved in checkpoints); m, v are allocated and zeroed on the
 * first call.  Decoupled weight decay, on every parameter unless parameter groups (below) scale it
 * per tensor (lr -> lr * lr_mul, wd -> weight_decay * wd_mul of the parameter's tensor and layer):
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g g;  p -= lr (m/(1-b1^t) / (sqrt(v/(1-b2^t)) + eps) + wd p) */
int vit_trainer_step_adamw(vit_trainer_t* t, float lr, float beta1, float beta2, float eps,
                           float weight_decay);
/* LAMB (You et al. 2020; timm's Lamb with grad_averaging): AdamW's direction scaled per
 * tensor and layer (a segment: one entry of vit_layout_query's indexing) by a trust ratio.  With m', v'
 * advanced and bias-corrected exactly as vit_trainer_step_adamw does (on g' = c * g under clipping) and
 * lr_e, wd_e the segment's lr and weight decay (parameter groups as for AdamW):
 *   u = m'/(1-b1^t) / (sqrt(v'/(1-b2^t)) + eps) + wd_e p        per element, every operation rounded to fp32
 *   wn = (float)sqrt(sum p^2), un = (float)sqrt(sum u^2)        over the segment's own elements, in double,
 *                                                                fixed order (deterministic, no atomics)
 *   r = wn / un if the segment is adapted and wn > 0 and un > 0, else 1
 *   p -= (lr_e * r) u
 * A segment is adapted if wd_e != 0 (timm: tensors without weight decay keep r = 1), or always under
 * VIT_LAMB_ALWAYS_ADAPT; VIT_LAMB_TRUST_CLIP caps r at 1 (LAMBC).  Where every r is 1 (weight_decay = 0, no
 * flags) the step has the bits of vit_trainer_step_adamw in p, m and v.  lr_mul = 0 freezes a segment's
 * values; its m, v and ratio are still computed.  The state (m, v, t, the stored hyper-parameters) is
 * AdamW's: the two step kinds may be mixed, both advance t, and a checkpoint saved after LAMB steps is an
 * AdamW-state file.  The bf16 shadow, the EMA (vit_trainer_set_ema) and the low-precision copies follow
 * as after an AdamW step; vit_trainer_get_grads still returns the raw gradients.  Waits for the
 * all-reduce first; data parallelism needs nothing more (identical gradients give identical ratios).
 * The first call allocates m, v and the per-tile / per-segment buffers (counted in
 * vit_trainer_device_bytes from then on).  beta1, beta2 outside [0, 1), a negative or non-finite eps or
 * weight_decay, and unknown flag bits return non-zero + vit_last_error and change nothing; so does a call
 * while the EMA weights are in use. */
enum { VIT_LAMB_ALWAYS_ADAPT = 1, VIT_LAMB_TRUST_CLIP = 2 };
int vit_trainer_step_lamb(vit_trainer_t* t, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int flags);
/* the last LAMB step's |w|, |u| and trust ratio, each [20 * num_layers] in vit_layout_query's indexing
 * (unused entries hold 0, 0, 1), and the number of LAMB steps so far.  Any pointer may be NULL.  An error
 * before the first LAMB step.  Synchronous. */
int vit_trainer_get_lamb_info(vit_trainer_t* t, float* w_norm, float* u_norm, float* ratio, long long* steps);
/* ---- global-norm gradient clipping, for vit_trainer_step, vit_trainer_step_adamw
 *      and vit_trainer_train_step.  Before the update the device computes S = sum of g^2 over every
 *      parameter's gradient (every square and sum in double, fixed order: deterministic),
 *      norm = (float)sqrt(S) and, in fp32 with IEEE division, c = max_norm / (norm + 1e-6f), c = 1
 *      unless c < 1 (the coefficient of torch.nn.utils.clip_grad_norm_); the optimizer kernels then
 *      use g' = c * g (rounded to fp32 on its own).  Nothing is read back on the step path.
 *      c == 1 gives the bits of the unclipped update.
 *      Unlike torch the gradient arena is NOT scaled: vit_trainer_get_grads keeps returning the raw
 *      gradients (the all-reduced ones under data parallelism, whose norm is then the one taken,
 *      identical on every rank).  Non-finite gradients get no special handling: the arithmetic
 *      above is simply applied (a NaN norm gives c = 1, an infinite one c = 0).
 *      With clipping on, vit_trainer_train_step does not take the early per-chunk SGD ("early_sgd":
 *      no parameter may change before the whole norm exists). ---- */
/* max_norm > 0 (may be +INFINITY: compute the norm, never scale); 0 = off (default).  NaN or a
 * negative value is an error and leaves the previous setting.  A hyper-parameter: persists across
 * steps, not written to checkpoints. */
int vit_trainer_set_grad_clip(vit_trainer_t* t, float max_norm);
/* global L2 norm of the gradients the last clipped optimizer step used (after the all-reduce under
 * DP); -1 if no step has computed one.  Synchronous. */
float vit_trainer_grad_norm(vit_trainer_t* t);
/* ---- parameter groups: per-tensor, per-layer multipliers of the learning rate and of
 *      the weight decay, applied inside the fused optimizer kernels of vit_trainer_step,
 *      vit_trainer_step_adamw and vit_trainer_train_step (the early per-chunk SGD included).  For the
 *      entry e of a parameter's tensor and layer the update runs with lr_e = lr * lr_mul[e] and
 *      wd_e = weight_decay * wd_mul[e], each one fp32 multiply rounded on its own, in place of lr and
 *      weight_decay; under clipping on g' = c * g as before.  1.0f * x == x, so all-ones multipliers
 *      give the bits of the ungrouped step.  Plain SGD has no weight decay and uses lr_mul only; momentum SGD
 *      (vit_trainer_set_sgd) uses both, and its buffer advances for a frozen tensor like AdamW's m and v.
 *      lr_mul == 0 freezes a tensor's values; AdamW's m and v of that tensor still advance (as in a
 *      torch parameter group with lr = 0), and its gradient is still computed.
 *      vit_trainer_grad_norm and the clip factor ignore the groups: the norm is over all raw gradients.
 *      Under data parallelism every rank must set the same tables. ---- */
/* lr_mul, wd_mul: [20 * num_layers] floats in the indexing of vit_layout_query's tensor_off
 * (tensor ti of the canonical order, layer l at [ti * num_layers + l]; unlayered tensors use l = 0 and
 * their other entries are ignored and read back as 1).  Either NULL = all ones.  Both NULL = groups
 * off (the default).  Every used entry must be finite and >= 0; otherwise non-zero + vit_last_error
 * and the previous setting stays.  A hyper-parameter: persists across steps, not written to
 * checkpoints.  Call between steps; synchronous (waits for the steps in flight). */
int vit_trainer_set_param_groups(vit_trainer_t* t, const float* lr_mul, const float* wd_mul);
/* the multipliers in force (ones when off; either pointer may be NULL); *on (nullable) = 1 if
 * groups are on */
int vit_trainer_get_param_groups(vit_trainer_t* t, float* lr_mul, float* wd_mul, int* on);
/* ---- stochastic depth / drop path: a table s[l][br][b] of non-negative finite scales, l the
 *      layer, br 0 = the attention branch and 1 = the MLP branch, b the image ([num_layers][2][batch]
 *      floats).  With y the branch's output (its bias included), for every row r of image b:
 *        forward:   x_out[r] = x_in[r] + fl32(s * y[r])       (the product rounded to fp32 on its own, no FMA);
 *        backward:  the pass-through gradient is unchanged; the branch's upstream gradient is
 *                   dy[r] = fl32(s * dout[r]), taken from the fp32 value (in bf16 mode that product, rounded
 *                   to bf16, is the operand of the branch's input- and weight-gradient GEMMs); the branch's
 *                   last bias gradient (attproj_b, fcproj_b) is the column sum of those fp32 products.
 *      s = 0 drops the branch for an image, s = 1 / (1 - p) keeps it at the usual rescale; 1.0f * x == x, so an
 *      all-ones table gives the bits of a step without one.  A trainer that never sets a table issues
 *      exactly the launches it did before.  VIT_FP32 and VIT_BF16 modes. ---- */
/* one-shot, like vit_trainer_set_augment_plan: the table applies to the next vit_trainer_forward /
 * vit_trainer_train_step of a batch that has labels and to that forward's backward, and is cleared by it (a
 * stale mask never repeats).  vit_trainer_eval and forwards of a batch without labels never drop and
 * leave a pending table pending.  NULL clears a pending table.  An entry that is not finite and >= 0:
 * non-zero + vit_last_error, the previous state stays.  VIT_FP8 mode: an error ("not supported in fp8
 * mode").  Returns once the host array has been read; the device buffers (the per-row table and, in bf16
 * mode, two [B*T, C] bf16 planes) are allocated by the first call and counted in
 * vit_trainer_device_bytes.  Not written to checkpoints. */
int vit_trainer_set_drop_path(vit_trainer_t* t, const float* host_scales);
/* the table the last training forward used into out ([num_layers][2][batch], nullable); *used (nullable)
 * = 0 if that forward ran without one (out is then left as it is) */
int vit_trainer_get_drop_path(vit_trainer_t* t, float* out, int* used);
/* ---- random erasing (timm's RandomErasing, DeiT: prob 0.25, pixel mode, one box): erase the
 *      current device batch in place on the trainer's stream with vit_random_erase_f32 (vit_ops.h: the boxes
 *      [batch][max_count][4], the modes VIT_ERASE_CONST / _RAND / _PIXEL, the normal z(p), the errors).  Call
 *      after any vit_trainer_set_batch* variant (it is ordered behind the u8 and JPEG paths' normalise) and
 *      before vit_trainer_mix_batch: erase first, then mix, timm's order without the prefetcher.  Works with
 *      or without labels and in every precision mode; touches only the pixels.  Non-zero + vit_last_error,
 *      the batch left as it was, on a bad argument, after vit_trainer_mix_batch of the same batch ("the batch
 *      is already mixed") and on a second erase of the same batch ("already erased"); every set_batch*
 *      resets both states.  Returns once the host arrays have been read (no wait for the stream).  The
 *      device list buffer is allocated by the first call that has a box and counted in
 *      vit_trainer_device_bytes.  Nothing is written to checkpoints; a trainer that never calls it issues the
 *      launches it always did.  The caller chooses the keys: epoch * N + record where it knows the record,
 *      (step * world + rank) * batch + i otherwise, so that ranks draw different boxes. ---- */
int vit_trainer_erase_batch(vit_trainer_t* t, const int* host_boxes, int max_count, int mode,
                            unsigned long long seed, const long long* host_keys);
/* host-only draw of such a table (no GPU call), out [num_layers][2][batch]:
 *   p_l = linear ? (float)((double)rate * l / (num_layers - 1)) : rate   (rate for num_layers == 1; timm's
 *         linspace(0, rate, depth));
 *   w   = the splitmix64 counter stream of s = seed ^ splitmix64(0x64726f7070617468, key) at position
 *         (2 l + br) * batch + b (the generator of the loaders' shuffle and vit_randaugment_draw);
 *   u   = (w >> 40) * 2^-24; the branch is kept iff u >= p_l;
 *   out = kept ? 1.0f / (1.0f - p_l) : 0.0f   (fp32 IEEE division).
 * The caller chooses key, e.g. step * world + rank, so that ranks draw different masks.  rate outside
 * [0, 1) (or a bad size): non-zero + vit_last_error. */
int vit_drop_path_draw(unsigned long long seed, long long key, int num_layers, int batch, float rate,
                       int linear, float* out);
/* host-only draw of one square image's erase boxes (no GPU call): timm's RandomErasing._erase on the
 * project's generator.  boxes [max_count][4] = x0, y0, x1, y1 (boxes past *count and failed boxes are
 * 0, 0, 0, 0), *count = the number of boxes drawn (0: the image is not erased).
 *   w_k = word k of the splitmix64 counter stream of s = seed ^ splitmix64(0x6572617365, key) (ASCII
 *         "erase"); every uniform is u = (w >> 11) * 2^-53 in double;
 *   w_0: the image is erased iff u < prob;
 *   w_1: count = min_count + floor(u * (max_count - min_count + 1)) (consumed even when the two are equal);
 *   box k, attempt a of 10: u0 .. u3 from the words 2 + (k * 10 + a) * 4 + {0, 1, 2, 3}:
 *     target = (min_area + u0 * (max_area - min_area)) * (img * img) / count
 *     aspect = exp(log(min_aspect) + u1 * (log(max_aspect) - log(min_aspect)))
 *     h = (int)rint(sqrt(target * aspect)), w = (int)rint(sqrt(target / aspect))   (ties to even)
 *     if w < img and h < img: top = floor(u2 * (img - h + 1)), left = floor(u3 * (img - w + 1)), the box is
 *     [left, left + w) x [top, top + h) and the attempts end; after ten failures the box is empty
 *   (all in double, evaluated left to right as written, with the C library's exp / log / sqrt).
 * Word positions are fixed and the draw is stateless: the boxes depend on (seed, key) and the arguments
 * only.  timm's defaults: min_area 0.02, max_area 1/3, min_aspect 0.3, max_aspect 1/0.3, counts 1, 1.
 * prob outside [0, 1], areas not 0 < min <= max <= 1, aspects not 0 < min <= max, counts not
 * 1 <= min <= max <= 4, img < 1: non-zero + vit_last_error, the outputs untouched. */
int vit_random_erase_draw(unsigned long long seed, long long key, int img, double prob, double min_area,
                          double max_area, double min_aspect, double max_aspect, int min_count, int max_count,
                          int* boxes, int* count);
/* ---- exponential moving average of the weights (timm's ModelEmaV2): one more fp32 arena e,
 *      advanced by every optimizer step while on.  With d the decay and omd = (float)(1.0 - (double)d), taken
 *      once on the host, for every element
 *          e' = fl32( fl32(d * e) + fl32(omd * p') )
 *      with p' the fp32 master value the step has just written; each product and the sum rounded to fp32 on
 *      its own (no FMA): numpy's fp32 `d * e + omd * p`.  In bf16 / fp8 mode (and for AdamW and momentum SGD in every mode) the
 *      update runs inside the optimizer kernels, which hold p' in registers; fp32-mode plain SGD launches
 *      ema_update (vit_ops.h) behind its update on the same stream: the same bits.  A trainer that never turns
 *      EMA on issues the launches, allocates the memory and writes the checkpoint bytes it always did.
 *      Data parallelism needs nothing more: every rank holds identical parameters after a step and applies
 *      the same elementwise update, so the averages are identical too (every rank must set the same decay). ---- */
/* decay 0 = off (the default), 0 < decay < 1 = on; NaN, negative or >= 1: non-zero + vit_last_error and the
 * previous setting stays.  The first switch from off to on allocates the arena (arena_elems floats, counted in
 * vit_trainer_device_bytes from then on), seeds it with a device copy of the current parameters and sets the
 * update count to 0; it waits for the steps in flight.  A call while on only changes d (no wait, no re-seed:
 * a host-side warm-up schedule may call it before every step).  Switching off keeps the arena; the next
 * switch on seeds it again.  vit_trainer_step, vit_trainer_step_adamw and vit_trainer_train_step advance the
 * average once per call while on (also at lr = 0, and for tensors frozen by lr_mul = 0); vit_trainer_set_params
 * does not touch it. */
int vit_trainer_set_ema(vit_trainer_t* t, float decay);
/* *decay (0 while off), *updates (optimizer steps averaged since the seed), *on; any pointer may be NULL */
int vit_trainer_get_ema_info(vit_trainer_t* t, float* decay, long long* updates, int* on);
/* canonical host copy of the average / overwrite it from one; synchronous; an error while EMA is off */
int vit_trainer_get_ema(vit_trainer_t* t, float* host);
int vit_trainer_set_ema_params(vit_trainer_t* t, const float* host);
/* evaluate with the averaged weights.  on = 1 exchanges the live and the averaged arena (a pointer exchange)
 * and refreshes every derived copy (the bf16 shadow, the transposed copies, the fp8 MX copies): until on = 0,
 * vit_trainer_eval / _forward / _get_logits use the average and vit_trainer_get_params returns it, and
 * vit_trainer_backward, _step, _step_adamw, _train_step, _zero_grad, _set_params, _set_ema, _set_ema_params, _set_sgd,
 * _load_checkpoint and _save_checkpoint return non-zero ("... EMA weights in use") and change nothing.
 * on = 0 exchanges back and refreshes again: the live fp32 parameters keep their bits and the derived
 * copies, deterministic functions of them, get theirs back.  on = 1 twice, on = 0 while not in use, and
 * on = 1 while EMA is off are errors.  Synchronous; waits for the side streams' work first. */
int vit_trainer_ema_weights(vit_trainer_t* t, int on);
/* ---- momentum SGD: torch.optim.SGD's update with momentum, dampening, Nesterov and coupled
 *      weight decay, as a setting of vit_trainer_step and vit_trainer_train_step (the early per-chunk update
 *      included), run inside the optimizer kernels.  For one element, with c the clip factor under clipping,
 *      lr_e = lr * lr_mul and wd_e = weight_decay * wd_mul of the element's parameter group (one fp32 multiply
 *      each, as for AdamW), mu the momentum and omd = (float)(1.0 - (double)dampening) taken once on the host,
 *      every operation rounded to fp32 on its own (no FMA):
 *          g1 = clipping ? c * g : g
 *          g2 = wd_e != 0 ? g1 + wd_e * p : g1
 *          b' = first ? g2 : mu * b + omd * g2
 *          d  = nesterov ? g2 + mu * b' : b'
 *          p' = p - lr_e * d
 *      `first` is the first momentum step after the buffer was created or reset (torch's buf = grad.clone(),
 *      without dampening).  A tensor with lr_mul = 0 keeps its values while its buffer advances.  The EMA reads
 *      p' and the bf16 shadow gets bf16(p'), as for plain SGD.  The buffer is one more fp32 arena, separate from
 *      AdamW's m and v: the step kinds may be interleaved and neither touches the other's state;
 *      vit_trainer_set_params does not touch it.  Under data parallelism every rank must set the same values. ---- */
/* 0, 0, 0, 0 = plain SGD (the default): the launches, the memory and the checkpoint bytes of a trainer that never
 * called this.  momentum > 0: the first such step allocates the buffer (arena_elems floats, zeroed, counted in
 * vit_trainer_device_bytes from then on) and runs with first = 1; every momentum step advances the step count
 * once (also at lr = 0).  Setting momentum back to 0 keeps the buffer and the count, plain steps do not touch
 * them, and turning it on again continues from them.  Every value must be finite, momentum >= 0 and
 * weight_decay >= 0; nesterov needs momentum > 0 and dampening == 0 (torch's rule); weight_decay > 0 needs
 * momentum > 0 (plain SGD has no decayed form here).  Otherwise, and while the EMA weights are in use:
 * non-zero + vit_last_error, the previous setting stays.  A hyper-parameter: persists across steps; written to
 * checkpoints together with the buffer. */
int vit_trainer_set_sgd(vit_trainer_t* t, float momentum, float dampening, float weight_decay, int nesterov);
/* the setting in force and the number of momentum steps since the buffer was seeded; any pointer may be NULL */
int vit_trainer_get_sgd_info(vit_trainer_t* t, float* momentum, float* dampening, float* weight_decay,
                             int* nesterov, long long* steps);
/* canonical host copy of the momentum buffer; synchronous; an error before the first momentum step */
int vit_trainer_get_momentum(vit_trainer_t* t, float* host);
/* ---- gradient accumulation over micro-batches: with steps = N > 1 the calls of
 *      vit_trainer_backward are counted in windows of N and their gradients summed on the device, so that one
 *      optimizer step sees a batch N times the one that fits.  `done` is the number of micro-steps in the open
 *      window: 0 = no window is open, N = the window is complete and not yet consumed.
 *        backward 1 of a window:   acc = g          (acc: one more fp32 arena of arena_elems floats, allocated by
 *                                                    the first such backward and counted in vit_trainer_device_bytes)
 *        backward k, 1 < k < N:    acc = fl32(acc + g)   per element
 *        backward N:               g = fl32(acc + g), written into the gradient arena itself
 *      so after backward N the gradient arena holds (((g1 + g2) + g3) + ... + gN), each sum rounded to fp32 once,
 *      in this fixed order: a function of the micro-batches and their order only, not of streams, chunks or the
 *      form that ran (option "accum_overlap").  The arena's padding stays zero.  A backward while done == N opens
 *      a new window (done = 1).  Everything at step time reads the gradient arena as always, so the clip norm and
 *      factor (vit_trainer_set_grad_clip) are those of the accumulated gradient, parameter groups, the EMA, momentum
 *      SGD, AdamW and LAMB need nothing more, and vit_trainer_get_grads returns the micro-batch's own gradient
 *      mid-window and the sum after backward N.
 *      Scaling is the caller's: pass b_global = N * batch * world to vit_trainer_forward / _train_step
 *      (dloss = 1 / b_global), and the sum is the gradient of the mean loss over the whole window.
 *      vit_trainer_step, _step_adamw and _step_lamb return non-zero with vit_last_error ("... gradient
 *      accumulation: micro-step k of N") and change nothing while 0 < done < N; otherwise they run as always
 *      and set done = 0.  vit_trainer_train_step: a call that leaves done < N does zero_grad + forward +
 *      backward + accumulate and returns 0 without an update; the call that completes the window also steps
 *      (only that call may take the early per-chunk SGD, each chunk's update behind the chunk's final sum).
 *      The mix, the erase, the one-shot drop-path table, the augment plan and vit_trainer_mean_loss stay per
 *      micro-batch.  vit_trainer_eval and forwards of a batch without labels do not count and do not touch acc.
 *      vit_trainer_save_checkpoint is an error mid-window and writes nothing; vit_trainer_load_checkpoint sets
 *      done = 0.  Data parallelism: backwards 1 .. N-1 issue no all-reduce (torch's no_sync); backward N reduces
 *      the accumulated gradient, per chunk behind the chunk's final sum with overlap on, whole at step time
 *      otherwise.  Every rank must set the same N.
 *      steps == 1, or never set: nothing is allocated, and the launches, their order and the checkpoint bytes
 *      are those of a trainer without the feature. ---- */
/* steps >= 1; 1 = off (the default).  Any call, also with the same value, abandons an open window (done = 0):
 * the way out of one.  steps < 1: non-zero + vit_last_error, the previous setting stays.  Waits for the work in
 * flight.  A hyper-parameter: persists across steps, not written to checkpoints. */
int vit_trainer_set_grad_accum(vit_trainer_t* t, int steps);
/* *steps and *done as above; either pointer may be NULL */
int vit_trainer_get_grad_accum_info(vit_trainer_t* t, int* steps, int* done);
/* canonical host copy of the accumulator acc while 0 < done < N; an error otherwise; synchronous */
int vit_trainer_get_grad_accum(vit_trainer_t* t, float* host);
/* canonical host copies of m, v (either may be NULL) and the step count; synchronous */
int vit_trainer_get_adamw_state(vit_trainer_t* t, float* m, float* v, int* step);
/* eval: forward of the current batch, then top-1 per image on the device.
 * host_pred [batch] (nullable) gets the predicted classes (first maximum, as numpy.argmax);
 * host_correct (nullable) gets the number equal to the labels, or -1 when the batch was set
 * without labels; for a mixed batch these are the batch's own labels (ta), not the partner's.
 * Synchronous. */
int vit_trainer_eval(vit_trainer_t* t, int* host_pred, int* host_correct);
/* zero_grad + forward + backward + step */
int vit_trainer_train_step(vit_trainer_t* t, float lr, int b_global);
/* synchronous readbacks; mean_loss = -1 for a batch without labels (the mean of the per-row
 * soft-target losses when smoothing or a mix is on) */
float vit_trainer_mean_loss(vit_trainer_t* t);
int vit_trainer_get_logits(vit_trainer_t* t, float* host_logits); /* [batch, num_classes] */
int vit_trainer_sync(vit_trainer_t* t);
void* vit_trainer_stream(vit_trainer_t* t);

/* device gradient-arena layout (host-only, no GPU needed): tensor_off [20 * num_layers] element
 * offsets of tensor ti (canonical order), layer l at [ti * num_layers + l] (unlayered tensors:
 * l = 0, the other entries 0); chunk_off [num_layers + 3] boundaries of the all-reduce chunks in
 * backward's completion order (0 = head + final LN, 1..L = layers L-1..0, L+1 = embedding);
 * arena_elems = arena size (with 64-element alignment padding).  Returns the chunk count (L + 2),
 * -1 on a bad config.  Any pointer may be NULL. */
int vit_layout_query(const vit_config_t* cfg, long long* tensor_off, long long* chunk_off,
                     long long* arena_elems);

/* ---- data parallelism over RCCL (one process per GPU) ---- */
int vit_dp_unique_id_size(void);
int vit_dp_get_unique_id(char* out);   /* rank 0 creates; broadcast the bytes out of band */
/* chunks: 0 = one all-reduce of the whole gradient arena after backward;
 *         1 = per-layer chunks on a side stream overlapped with backward (default) */
int vit_trainer_dp_init(vit_trainer_t* t, int rank, int world, const char* unique_id, int overlap);
/* ranks of the trainer's RCCL communicator (ncclCommCount); 0 before vit_trainer_dp_init */
int vit_trainer_dp_ranks(vit_trainer_t* t);

/* ---- stream concurrency (bf16 mode): on (default) = the batch runs as two micro-batch row halves
 *      on two streams and the weight-gradient GEMMs on a third; off = one stream, kernels one at a
 *      time (per-kernel roofline timing).  Call between steps. ---- */
int vit_trainer_set_concurrency(vit_trainer_t* t, int on);
/* ---- tuning options for A/B measurements in one process (call between steps):
 *      "microbatch" = number of micro-batch streams wanted (1 .. 4; the largest divisor of B),
 *      "early_sgd" = -1 (default: on in fp8 mode, off in bf16; measured per dtype): one GPU, bf16 / fp8, concurrency on: vit_trainer_train_step
 *      updates each gradient chunk (head, layer L-1 .. 0, embedding) as soon as the backward has
 *      finished it, on a side stream beside the rest of the backward (same bits as one pass),
 *      "clip_overlap" = -1 (default: auto = 0 in bf16 and fp8 mode, measured): with
 *      gradient clipping on, bf16 / fp8 and concurrency on, 1 takes each gradient chunk's partial
 *      sums of squares on the side (all-reduce) stream as soon as the backward has finished the
 *      chunk, 0 takes them all at step time on the main stream (same bits either way),
 *      "accum_overlap" = -1 (default: auto = 0 in bf16 mode, 1 in fp8 mode, measured): under
 *      gradient accumulation, bf16 / fp8 and concurrency on, 1 sums each gradient chunk on the side
 *      (all-reduce) stream as soon as the backward has finished the chunk, 0 sums the whole arena in one
 *      launch behind the backward (same bits either way),
 *      "last_cls" = 1 (default; bf16 mode only, ignored in fp32 and fp8 mode): the classifier head reads
 *      only the CLS row of each image, so the last block's attention projection, LayerNorm 2, fc + GELU
 *      and fcproj and the fc / attention-projection input gradients run on the B CLS rows instead of all
 *      B*T (same loss, logits and gradients bit for bit).  0: every row,
 *      "last_cls_bwd" = 2 (default; honoured with last_cls on): 1 = the last block's three weight
 *      gradients skip the K-steps of the token axis that hold no CLS row, 2 = also its fcproj input
 *      gradient on the CLS rows, the fc-bias column sums kept in the full-size grouping (same bits
 *      again).  0: both full size,
 *      "ema_fused" = 1 (default): with EMA on (vit_trainer_set_ema) the bf16 / fp8 optimizer kernels and AdamW
 *      advance the average themselves; 0 runs them as without EMA and launches ema_update behind each on
 *      the same stream (same bits; the A/B of tools/bench_ema.py),
 *      "dp_probe" = 1: every gradient chunk is also copied, on the all-reduce stream right after
 *      its all-reduce, into a snapshot arena (read with vit_trainer_get_dp_snapshot) — a check
 *      that each overlapped chunk was final when it was reduced.
 *      Returns non-zero (and sets the error) for an unknown name. ---- */
int vit_trainer_set_option(vit_trainer_t* t, const char* name, int value);
/* canonical host copy of the dp_probe snapshot arena; synchronous */
int vit_trainer_get_dp_snapshot(vit_trainer_t* t, float* host);

/* ---- per-kernel-class timing with HIP events on the stream each kernel runs on ---- */
int vit_trainer_set_timing(vit_trainer_t* t, int on);
/* fills up to max entries; returns the number of classes. names point to static strings */
int vit_trainer_timing(vit_trainer_t* t, const char** names, double* total_ms, long long* calls,
                       double* flops, int max);
void vit_trainer_timing_reset(vit_trainer_t* t);

#ifdef __cplusplus
}
#endif
#endif
