// checkpoint_internal.h — the checkpoint format (include/vit_checkpoint.h) stated once, for checkpoint.cpp's
// public functions and the trainer's save / load (trainer.hip).  Internal: nothing here is exported.
#pragma once
#include <cstdio>
#include <memory>

#include "../../include/vit_checkpoint.h"

namespace vit {
namespace ckpt {

// The arrays behind the header, in file order: each num_params fp32 in canonical order.
enum Section { SEC_PARAMS, SEC_M, SEC_V, SEC_EMA, SEC_MOMENTUM, SEC_COUNT };
enum { FLAG_ADAMW = 1, FLAG_EMA = 2, FLAG_MOMENTUM = 4 };  // header flags

// Everything the 256-int header carries.  The EMA and momentum fields are zero unless their flag is set.
struct Header {
    int magic = VIT_CKPT_MAGIC, version = VIT_CKPT_VERSION, max_seq_len = 0;
    vit_config_t cfg{};
    long long num_params = 0;
    int flags = 0;
    int step = 0;  // AdamW t and the hyper-parameters of its last update
    vit_adamw_t adamw{0.f, 0.f, 0.f, 0.f};
    float ema_decay = 0.f;
    long long ema_updates = 0;
    long long momentum_steps = 0;
    vit_sgd_t sgd{0.f, 0.f, 0.f, 0};

    bool has(Section s) const;
    long long offset(Section s) const;  // byte offset of a present section
    long long file_bytes() const;       // the header and every present section
};

// Writes path (through path.tmp, fsync, rename and the directory's fsync): the header and the non-NULL
// sections.  flags, max_seq_len and num_params come from h.cfg and the pointers; the AdamW, EMA and momentum
// fields of an absent section are written as zero.  sec[SEC_PARAMS] non-NULL, sec[SEC_M] and sec[SEC_V] both
// or neither.  0, or non-zero with the error set.
int write(const char* path, Header h, const float* const (&sec)[SEC_COUNT]);

// One open file: the header parsed and validated once (magic, version, config, max_seq_len, num_params and
// the file size of its layout), then any of its sections.  Every call: 0, or non-zero with the error set.
class Reader {
public:
    int open(const char* path);
    int require_config(const vit_config_t* cfg);  // fails unless cfg is the file's config
    int read(Section s, float* dst);              // a present section into dst[num_params]
    const Header& header() const { return h_; }

private:
    std::unique_ptr<FILE, int (*)(FILE*)> f_{nullptr, fclose};
    const char* path_ = nullptr;
    Header h_;
};
}  // namespace ckpt
}  // namespace vit
