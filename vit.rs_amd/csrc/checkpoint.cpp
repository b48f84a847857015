// checkpoint.cpp — ViT checkpoint files (include/vit_checkpoint.h), host-only code.
//
// Format: the llm.c convention of ViT::build_from_checkpoint (/root/reference/train_vit.rs:
// 89-143: 256-int header at byte 0, fp32 type-major parameters at byte 1024) completed with the
// ViT tensors and the optional AdamW state, EMA and momentum buffer; see the header file for the field table.
//
// The format is stated once (checkpoint_internal.h): header_walk holds the slot numbers, for header_parse and
// header_encode; kSections the arrays in file order with their presence rules, and offsets and the file size
// come from that table.  ckpt::write is the one writer, ckpt::Reader the one reader (one open, one
// validation); the public functions below and the trainer's save / load are calls of those two.
#include "checkpoint_internal.h"

#include <fcntl.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <string>

namespace vit {
void set_error(const char* fmt, ...);
}
using vit::set_error;
using namespace vit::ckpt;

namespace {

bool config_ok(const vit_config_t& c) {
    return c.img > 0 && c.patch > 0 && c.img % c.patch == 0 && c.in_ch > 0 && c.channels > 0 &&
           c.num_layers > 0 && c.num_heads > 0 && c.channels % c.num_heads == 0 &&
           c.num_classes > 0;
}
long long seq_len(const vit_config_t& c) { return (long long)(c.img / c.patch) * (c.img / c.patch) + 1; }

constexpr int HEADER_INTS = VIT_CKPT_HEADER_BYTES / 4;

// The header slots (the table in include/vit_checkpoint.h), in this one walk only, which both directions
// take: PARSE fills h from the words, otherwise h is written into them.  The AdamW fields are written for a
// file with m / v and parsed as they stand; the EMA and momentum fields go either way only under their flag.
template <bool PARSE>
struct Slots {
    int32_t* w;
    void i32(int k, int& x) { PARSE ? (void)(x = w[k]) : (void)(w[k] = x); }
    void f32(int k, float& x) { PARSE ? memcpy(&x, &w[k], 4) : memcpy(&w[k], &x, 4); }
    void i64(int k, long long& x) {  // low / high 32 bits
        if (PARSE) x = (long long)(uint32_t)w[k] | ((long long)(uint32_t)w[k + 1] << 32);
        else w[k] = (int32_t)(uint32_t)(x & 0xffffffffLL), w[k + 1] = (int32_t)(uint32_t)(x >> 32);
    }
};
template <bool PARSE>
void header_walk(Slots<PARSE> io, Header& h) {
    io.i32(0, h.magic); io.i32(1, h.version); io.i32(2, h.max_seq_len);
    io.i32(3, h.cfg.num_classes); io.i32(4, h.cfg.num_layers); io.i32(5, h.cfg.num_heads); io.i32(6, h.cfg.channels);
    io.i32(7, h.cfg.img); io.i32(8, h.cfg.patch); io.i32(9, h.cfg.in_ch);
    io.i32(10, h.flags);
    io.i64(12, h.num_params);
    if (PARSE || (h.flags & FLAG_ADAMW)) {
        io.i32(11, h.step);
        io.f32(14, h.adamw.beta1); io.f32(15, h.adamw.beta2); io.f32(16, h.adamw.eps); io.f32(17, h.adamw.weight_decay);
    }
    if (h.flags & FLAG_EMA) {
        io.f32(18, h.ema_decay);
        io.i64(19, h.ema_updates);
    }
    if (h.flags & FLAG_MOMENTUM) {
        io.i64(21, h.momentum_steps);
        io.f32(23, h.sgd.momentum); io.f32(24, h.sgd.dampening); io.f32(25, h.sgd.weight_decay);
        int nesterov = h.sgd.nesterov != 0;  // a 0 / 1 word in the file, any non-zero word read as 1
        io.i32(26, nesterov);
        h.sgd.nesterov = nesterov != 0;
    }
}
void header_encode(Header h, int32_t (&w)[HEADER_INTS]) {
    memset(w, 0, sizeof(w));
    header_walk(Slots<false>{w}, h);
}
Header header_parse(int32_t (&w)[HEADER_INTS]) {
    Header h;
    header_walk(Slots<true>{w}, h);
    return h;
}

// The sections in file order: the flag that says a file has it (0: always) and its name in a "short ...
// section" error.
const struct {
    int flag;
    const char* what;
} kSections[SEC_COUNT] = {{0, "parameter"}, {FLAG_ADAMW, "optimizer"}, {FLAG_ADAMW, "optimizer"}, {FLAG_EMA, "EMA"},
                          {FLAG_MOMENTUM, "momentum"}};

bool write_all(FILE* f, const void* p, size_t bytes) { return fwrite(p, 1, bytes, f) == bytes; }
bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

}  // namespace

namespace vit {
namespace ckpt {

bool Header::has(Section s) const { return kSections[s].flag == 0 || (flags & kSections[s].flag) != 0; }
long long Header::offset(Section s) const {
    long long at = VIT_CKPT_HEADER_BYTES;
    for (int k = 0; k < s; k++)
        if (has((Section)k)) at += num_params * 4;
    return at;
}
long long Header::file_bytes() const { return offset(SEC_COUNT); }

int write(const char* path, Header h, const float* const (&sec)[SEC_COUNT]) {
    if (!path || !sec[SEC_PARAMS] || (!sec[SEC_M]) != (!sec[SEC_V])) {
        set_error("vit_checkpoint_write: bad arguments");
        return 1;
    }
    if (!config_ok(h.cfg)) {
        set_error("vit_checkpoint_write: invalid config");
        return 1;
    }
    h.max_seq_len = (int)seq_len(h.cfg);
    h.num_params = vit_config_num_params(&h.cfg);
    h.flags = 0;
    for (int k = 0; k < SEC_COUNT; k++)
        if (sec[k]) h.flags |= kSections[k].flag;
    int32_t hdr[HEADER_INTS];
    header_encode(h, hdr);
    // write to path.tmp and rename, so an interrupted save never leaves a truncated checkpoint
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) {
        set_error("checkpoint %s: cannot create", tmp.c_str());
        return 1;
    }
    bool ok = write_all(f, hdr, sizeof(hdr));
    for (int k = 0; ok && k < SEC_COUNT; k++)
        if (sec[k]) ok = write_all(f, sec[k], (size_t)h.num_params * 4);
    // durable before the rename: the data blocks must reach the disk before the new name does
    ok = ok && fflush(f) == 0 && fsync(fileno(f)) == 0;
    if (fclose(f) != 0 || !ok) {
        set_error("checkpoint %s: write failed", tmp.c_str());
        remove(tmp.c_str());
        return 1;
    }
    if (rename(tmp.c_str(), path) != 0) {
        set_error("checkpoint %s: rename failed", path);
        remove(tmp.c_str());
        return 1;
    }
    // and the rename itself: fsync the directory entry
    std::string dir(path);
    const size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? "." : (slash == 0 ? "/" : dir.substr(0, slash));
    const int dfd = open(dir.c_str(), O_RDONLY | O_DIRECTORY);
    if (dfd >= 0) {
        fsync(dfd);
        close(dfd);
    }
    return 0;
}

int Reader::open(const char* path) {
    if (!path) {
        set_error("vit_checkpoint_read_info: null argument");
        return 1;
    }
    path_ = path;
    f_.reset(fopen(path, "rb"));
    if (!f_) {
        set_error("checkpoint %s: cannot open", path);
        return 1;
    }
    int32_t w[HEADER_INTS];
    if (!read_all(f_.get(), w, sizeof(w))) {
        set_error("checkpoint %s: short header", path);
        return 1;
    }
    h_ = header_parse(w);
    if (h_.magic != VIT_CKPT_MAGIC || h_.version != VIT_CKPT_VERSION) {
        set_error("checkpoint %s: bad magic/version %d/%d", path, h_.magic, h_.version);
        return 1;
    }
    if (!config_ok(h_.cfg)) {
        set_error("checkpoint %s: invalid config in header", path);
        return 1;
    }
    if (h_.max_seq_len != seq_len(h_.cfg)) {
        set_error("checkpoint %s: max_seq_len %d != (img/patch)^2+1 = %lld", path, h_.max_seq_len,
                  seq_len(h_.cfg));
        return 1;
    }
    if (h_.num_params != vit_config_num_params(&h_.cfg)) {
        set_error("checkpoint %s: num_params %lld does not match the config (%lld)", path, h_.num_params,
                  vit_config_num_params(&h_.cfg));
        return 1;
    }
    if (fseeko(f_.get(), 0, SEEK_END) != 0) {
        set_error("checkpoint %s: seek failed", path);
        return 1;
    }
    const long long want = h_.file_bytes(), have = (long long)ftello(f_.get());
    if (have != want) {
        set_error("checkpoint %s: %lld bytes, expected %lld", path, have, want);
        return 1;
    }
    return 0;
}

int Reader::require_config(const vit_config_t* cfg) {
    if (cfg && memcmp(&h_.cfg, cfg, sizeof(vit_config_t)) == 0) return 0;
    set_error("checkpoint %s: config differs from the model's", path_);
    return 1;
}

int Reader::read(Section s, float* dst) {
    if (!h_.has(s) || fseeko(f_.get(), h_.offset(s), SEEK_SET) != 0 ||
        !read_all(f_.get(), dst, (size_t)h_.num_params * 4)) {
        set_error("checkpoint %s: short %s section", path_, kSections[s].what);
        return 1;
    }
    return 0;
}

}  // namespace ckpt
}  // namespace vit

extern "C" {

long long vit_config_num_params(const vit_config_t* cfg) {
    if (!cfg || !config_ok(*cfg)) return 0;
    const long long C = cfg->channels, L = cfg->num_layers, NC = cfg->num_classes;
    const long long np = (long long)(cfg->img / cfg->patch) * (cfg->img / cfg->patch);
    const long long K = (long long)cfg->in_ch * cfg->patch * cfg->patch, T = np + 1;
    // the 20 canonical tensors (vit_trainer.h): embed, 12 per-layer kinds, lnf, head
    return C * K + C + C + T * C + L * (C + C + 3 * C * C + 3 * C + C * C + C + C + C +
                                        4 * C * C + 4 * C + 4 * C * C + C) +
           C + C + NC * C + NC;
}

int vit_checkpoint_read_info(const char* path, vit_checkpoint_info_t* info) {
    Reader r;
    if (r.open(info ? path : nullptr)) return 1;
    const Header& h = r.header();
    *info = vit_checkpoint_info_t{h.cfg, h.num_params, h.has(SEC_M), h.step, h.adamw};
    return 0;
}

int vit_checkpoint_write(const char* path, const vit_config_t* cfg, const float* params,
                         const float* m, const float* v, int step, const vit_adamw_t* adamw) {
    return vit_checkpoint_write_sgd(path, cfg, params, m, v, step, adamw, nullptr, 0.f, 0, nullptr, nullptr, 0);
}

int vit_checkpoint_write_ex(const char* path, const vit_config_t* cfg, const float* params,
                            const float* m, const float* v, int step, const vit_adamw_t* adamw,
                            const float* ema, float ema_decay, long long ema_updates) {
    return vit_checkpoint_write_sgd(path, cfg, params, m, v, step, adamw, ema, ema_decay, ema_updates, nullptr,
                                    nullptr, 0);
}

int vit_checkpoint_write_sgd(const char* path, const vit_config_t* cfg, const float* params,
                             const float* m, const float* v, int step, const vit_adamw_t* adamw,
                             const float* ema, float ema_decay, long long ema_updates,
                             const float* momentum, const vit_sgd_t* sgd, long long momentum_steps) {
    if (!cfg || (ema && ema_updates < 0) || (momentum && (!sgd || momentum_steps < 0))) {
        set_error("vit_checkpoint_write: bad arguments");
        return 1;
    }
    Header h;
    h.cfg = *cfg;
    h.step = step;
    if (adamw) h.adamw = *adamw;
    h.ema_decay = ema_decay;
    h.ema_updates = ema_updates;
    h.momentum_steps = momentum_steps;
    if (sgd) h.sgd = *sgd;
    return write(path, h, {params, m, v, ema, momentum});
}

int vit_checkpoint_read(const char* path, const vit_config_t* cfg, float* params, float* m,
                        float* v) {
    Reader r;
    if (r.open(path) || r.require_config(params ? cfg : nullptr) || r.read(SEC_PARAMS, params)) return 1;
    if (!r.header().has(SEC_M)) return 0;
    return (m && r.read(SEC_M, m)) || (v && r.read(SEC_V, v));
}

int vit_checkpoint_read_ema(const char* path, const vit_config_t* cfg, float* ema, float* decay,
                            long long* updates, int* has_ema) {
    Reader r;
    if (r.open(path) || r.require_config(cfg)) return 1;
    const Header& h = r.header();
    if (has_ema) *has_ema = h.has(SEC_EMA);
    if (decay) *decay = h.ema_decay;
    if (updates) *updates = h.ema_updates;
    return h.has(SEC_EMA) && ema && r.read(SEC_EMA, ema);
}

int vit_checkpoint_read_momentum(const char* path, const vit_config_t* cfg, float* momentum, vit_sgd_t* sgd,
                                 long long* steps, int* has_momentum) {
    Reader r;
    if (r.open(path) || r.require_config(cfg)) return 1;
    const Header& h = r.header();
    if (has_momentum) *has_momentum = h.has(SEC_MOMENTUM);
    if (sgd) *sgd = h.sgd;
    if (steps) *steps = h.momentum_steps;
    return h.has(SEC_MOMENTUM) && momentum && r.read(SEC_MOMENTUM, momentum);
}

}  // extern "C"
