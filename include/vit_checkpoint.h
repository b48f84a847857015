/*
 * vit_checkpoint.h — ViT checkpoint files, host-only functions of libvit_hip.so.
 *
 * The reference's loader, ViT::build_from_checkpoint (/root/reference/train_vit.rs:89-186),
 * follows the llm.c convention: a 256-entry header at byte 0, the fp32 parameters in canonical
 * type-major order at byte 1024.  Its save_checkpoint / load_checkpoint (:715-735) write and read
 * only `wte`, with no header, and it reads the header into a byte array (D8), so the
 * reference has no complete format to stay compatible with.  This one keeps the convention and
 * completes it for the ViT tensors:
 *
 *   int32 header[256] (little endian) at byte 0
 *     [0] VIT_CKPT_MAGIC   [1] VIT_CKPT_VERSION
 *     [2] max_seq_len T = (img/patch)^2 + 1    (the reference's header[2])
 *     [3] num_classes     (the reference's vocab_size slot, header[3])
 *     [4] num_layers  [5] num_heads  [6] channels   (header[4..6], as the reference)
 *     [7] img  [8] patch  [9] in_ch
 *     [10] flags: bit 0 = AdamW state (m, v) follows the parameters
 *                 bit 1 = an EMA of the weights follows them (behind m and v when bit 0 is set too)
 *                 bit 2 = a momentum-SGD buffer follows them (last: behind m, v and the EMA)
 *     [11] AdamW step t (number of completed AdamW updates)
 *     [12] / [13] num_params, low / high 32 bits
 *     [14..17] beta1, beta2, eps, weight_decay of the last AdamW update (IEEE fp32 bits)
 *     [18] the EMA's decay (IEEE fp32 bits)   [19] / [20] its update count, low / high 32 bits
 *          (all three zero unless flags bit 1 is set)
 *     [21] / [22] the momentum step count, low / high 32 bits   [23..25] momentum, dampening, weight decay
 *          (IEEE fp32 bits)   [26] nesterov   (all six zero unless flags bit 2 is set)
 *     rest zero
 *   fp32 params[num_params] at byte 1024, in the 20-tensor canonical order of vit_trainer.h
 *   (patch_w, patch_b, cls, wpe, ln1w .. fcprojb (each [L, ...]), lnfw, lnfb, head_w, head_b)
 *   if flags & 1: fp32 m[num_params], then fp32 v[num_params], same order.
 *   if flags & 2: fp32 ema[num_params], same order.
 *   if flags & 4: fp32 momentum[num_params], same order.
 * A file without an EMA has the bytes it had before bit 1 existed, one without a momentum buffer those it
 * had before bit 2 existed (every older layout is a prefix); the version stays 1.
 *
 * All functions return 0 on success; on failure non-zero with the reason in vit_last_error().
 */
#ifndef VIT_CHECKPOINT_H
#define VIT_CHECKPOINT_H

#include "vit_trainer.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { VIT_CKPT_MAGIC = 20261016, VIT_CKPT_VERSION = 1, VIT_CKPT_HEADER_BYTES = 1024 };

typedef struct {
    float beta1, beta2, eps, weight_decay;
} vit_adamw_t;

/* the momentum-SGD setting (vit_trainer_set_sgd) */
typedef struct {
    float momentum, dampening, weight_decay;
    int nesterov;
} vit_sgd_t;

typedef struct {
    vit_config_t cfg;
    long long num_params;
    int has_opt;        /* AdamW m / v present */
    int step;           /* AdamW t */
    vit_adamw_t adamw;
} vit_checkpoint_info_t;

/* canonical parameter count of a config (sum of the 20 tensor sizes) */
long long vit_config_num_params(const vit_config_t* cfg);
/* header only; validates magic, version, T == (img/patch)^2+1 and the file size (of every layout: with or
 * without the AdamW state, the EMA array and the momentum buffer; this struct does not report the last two:
 * vit_checkpoint_read_ema, vit_checkpoint_read_momentum) */
int vit_checkpoint_read_info(const char* path, vit_checkpoint_info_t* info);
/* m, v: NULL for a parameters-only file (then step / adamw are ignored) */
int vit_checkpoint_write(const char* path, const vit_config_t* cfg, const float* params,
                         const float* m, const float* v, int step, const vit_adamw_t* adamw);
/* reads params (and m, v when non-NULL and present in the file) of num_params elements; fails if
 * the file's config differs from *cfg.  An EMA array in the file is ignored. */
int vit_checkpoint_read(const char* path, const vit_config_t* cfg, float* params, float* m,
                        float* v);
/* vit_checkpoint_write with an EMA of the weights: ema NULL writes exactly the file vit_checkpoint_write does
 * (ema_decay / ema_updates ignored); otherwise ema[num_params] follows the other arrays and the header
 * carries ema_decay and ema_updates (>= 0) */
int vit_checkpoint_write_ex(const char* path, const vit_config_t* cfg, const float* params,
                            const float* m, const float* v, int step, const vit_adamw_t* adamw,
                            const float* ema, float ema_decay, long long ema_updates);
/* *has_ema = 1 if the file holds an EMA, then *decay, *updates from the header and ema[num_params] (NULL: query
 * only); without one *has_ema = 0, *decay = 0, *updates = 0 and ema is left alone.  Every out pointer may be
 * NULL.  Fails if the file's config differs from *cfg. */
int vit_checkpoint_read_ema(const char* path, const vit_config_t* cfg, float* ema, float* decay,
                            long long* updates, int* has_ema);

/* vit_checkpoint_write_ex with a momentum-SGD buffer: momentum NULL writes exactly the file
 * vit_checkpoint_write_ex does (sgd / momentum_steps ignored); otherwise momentum[num_params] follows every
 * other array and the header carries *sgd (non-NULL) and momentum_steps (>= 0) */
int vit_checkpoint_write_sgd(const char* path, const vit_config_t* cfg, const float* params,
                             const float* m, const float* v, int step, const vit_adamw_t* adamw,
                             const float* ema, float ema_decay, long long ema_updates,
                             const float* momentum, const vit_sgd_t* sgd, long long momentum_steps);
/* *has = 1 if the file holds a momentum buffer, then *sgd, *steps from the header and momentum[num_params]
 * (NULL: query only); without one *has = 0, *sgd all zero, *steps = 0 and momentum is left alone.  Every out
 * pointer may be NULL.  Fails if the file's config differs from *cfg. */
int vit_checkpoint_read_momentum(const char* path, const vit_config_t* cfg, float* momentum, vit_sgd_t* sgd,
                                 long long* steps, int* has);

/* ---- trainer-level save / resume (synchronous).  Save writes the AdamW state once an AdamW
 *      step has run, and the EMA (vit_trainer_set_ema) while it is on; load restores params (and m, v, t
 *      when present) and refreshes the bf16 shadows.  Loading a file with an EMA turns EMA on with the
 *      file's decay, values and update count; loading one without into a trainer whose EMA is on seeds the
 *      average again from the loaded parameters (count 0).  Save writes the momentum buffer, its step count
 *      and the vit_trainer_set_sgd setting once a momentum step has run; load restores all of them from a file
 *      that has them, and for a file without them sets the count to 0 (the next momentum step seeds the buffer
 *      again) and leaves the setting alone. ---- */
int vit_trainer_save_checkpoint(vit_trainer_t* t, const char* path);
int vit_trainer_load_checkpoint(vit_trainer_t* t, const char* path);

#ifdef __cplusplus
}
#endif
#endif
