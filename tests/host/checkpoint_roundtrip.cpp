// checkpoint_roundtrip.cpp — a stand-alone host program over vit.rs_amd/csrc/checkpoint.cpp (no HIP, no Python):
// every layout of the checkpoint format written and read back through every public reader with every
// combination of NULL and non-NULL out pointers, then every cut of every file refused with the caller's
// buffers untouched.  Exits non-zero on the first mismatch.  Built and run by
// tests/test_checkpoint_sections_cpu.py.
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vit_checkpoint.h"

// the library's error channel (context.hip there): the last message is kept
static char g_error[512];
namespace vit {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace vit
extern "C" int vit_last_error(const char** msg) {
    if (msg) *msg = g_error;
    return g_error[0] != 0;
}

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            fprintf(stderr, "%s:%d: %s failed (%s; last error: %s)\n", __FILE__, __LINE__, #cond, g_what.c_str(), \
                    g_error);                                                                        \
            exit(1);                                                                                 \
        }                                                                                            \
    } while (0)

static std::string g_what;

static const vit_config_t CFG{4, 2, 1, 4, 1, 2, 3};  // 311 parameters
static const vit_adamw_t HP{0.9f, 0.95f, 1e-8f, 0.1f};
static const vit_sgd_t SGD{0.9f, 0.0f, 5e-4f, 1};
static const int STEP = 7;
static const float DECAY = 0.9999f;
static const long long UPDATES = (1LL << 33) + 5, MSTEPS = (1LL << 34) + 3;
static const float SENTINEL = -77.25f;

struct Layout {
    bool opt, ema, mom;
};

static std::vector<float> filled(long long n, int salt) {
    std::vector<float> a((size_t)n);
    for (long long i = 0; i < n; i++) a[(size_t)i] = (float)(salt * 1000 + i) * 0.125f - 3.0f;
    return a;
}
static bool same(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * 4) == 0;
}
static bool untouched(const std::vector<float>& a) {
    for (float x : a)
        if (memcmp(&x, &SENTINEL, 4) != 0) return false;
    return true;
}
static std::vector<char> slurp(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    CHECK(f);
    std::vector<char> out;
    char buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return out;
}
static void spit(const std::string& path, const std::vector<char>& bytes, size_t len) {
    FILE* f = fopen(path.c_str(), "wb");
    CHECK(f);
    std::vector<char> b(bytes);
    b.resize(len, 0);  // (a length behind the end pads with zero bytes)
    CHECK(fwrite(b.data(), 1, len, f) == len);
    fclose(f);
}

// Every reader with every combination of out pointers.  ok: the file is a valid one of layout L and the
// results are compared with the arrays written; !ok: every call must fail and leave every output as it was.
static void read_all_ways(const std::string& path, const Layout& L, bool ok, const std::vector<float> (&src)[5]) {
    const long long n = vit_config_num_params(&CFG);
    const char* p = path.c_str();
    {
        vit_checkpoint_info_t info;
        memset(&info, 0x5a, sizeof info);
        vit_checkpoint_info_t before = info;
        const int rc = vit_checkpoint_read_info(p, &info);
        CHECK((rc == 0) == ok);
        if (ok) {
            CHECK(memcmp(&info.cfg, &CFG, sizeof CFG) == 0 && info.num_params == n && info.has_opt == (L.opt ? 1 : 0));
            CHECK(info.step == (L.opt ? STEP : 0));
            const vit_adamw_t want = L.opt ? HP : vit_adamw_t{0.f, 0.f, 0.f, 0.f};
            CHECK(memcmp(&info.adamw, &want, sizeof want) == 0);
        } else {
            CHECK(memcmp(&info, &before, sizeof info) == 0);
        }
        CHECK(vit_checkpoint_read_info(p, nullptr) != 0);
    }
    for (int mask = 0; mask < 4; mask++) {  // vit_checkpoint_read: m, v
        std::vector<float> a((size_t)n, SENTINEL), m((size_t)n, SENTINEL), v((size_t)n, SENTINEL);
        const int rc = vit_checkpoint_read(p, &CFG, a.data(), (mask & 1) ? m.data() : nullptr, (mask & 2) ? v.data() : nullptr);
        CHECK((rc == 0) == ok);
        if (ok) {
            CHECK(same(a, src[0]));
            CHECK((L.opt && (mask & 1)) ? same(m, src[1]) : untouched(m));
            CHECK((L.opt && (mask & 2)) ? same(v, src[2]) : untouched(v));
        } else {
            CHECK(untouched(a) && untouched(m) && untouched(v));
        }
    }
    {
        std::vector<float> a((size_t)n, SENTINEL);
        CHECK(vit_checkpoint_read(p, nullptr, a.data(), nullptr, nullptr) != 0 && untouched(a));
        CHECK(vit_checkpoint_read(p, &CFG, nullptr, nullptr, nullptr) != 0);
    }
    for (int mask = 0; mask < 16; mask++) {  // vit_checkpoint_read_ema: ema, decay, updates, has_ema
        std::vector<float> e((size_t)n, SENTINEL);
        float d = SENTINEL;
        long long u = -5;
        int has = -5;
        const int rc = vit_checkpoint_read_ema(p, &CFG, (mask & 1) ? e.data() : nullptr, (mask & 2) ? &d : nullptr,
                                               (mask & 4) ? &u : nullptr, (mask & 8) ? &has : nullptr);
        CHECK((rc == 0) == ok);
        if (ok) {
            CHECK((L.ema && (mask & 1)) ? same(e, src[3]) : untouched(e));
            CHECK((mask & 2) ? d == (L.ema ? DECAY : 0.f) : d == SENTINEL);
            CHECK((mask & 4) ? u == (L.ema ? UPDATES : 0) : u == -5);
            CHECK((mask & 8) ? has == (L.ema ? 1 : 0) : has == -5);
        } else {
            CHECK(untouched(e) && d == SENTINEL && u == -5 && has == -5);
        }
    }
    for (int mask = 0; mask < 16; mask++) {  // vit_checkpoint_read_momentum: momentum, sgd, steps, has
        std::vector<float> b((size_t)n, SENTINEL);
        vit_sgd_t sg{SENTINEL, SENTINEL, SENTINEL, -5};
        const vit_sgd_t before = sg, zero{0.f, 0.f, 0.f, 0};
        long long st = -5;
        int has = -5;
        const int rc = vit_checkpoint_read_momentum(p, &CFG, (mask & 1) ? b.data() : nullptr, (mask & 2) ? &sg : nullptr,
                                                    (mask & 4) ? &st : nullptr, (mask & 8) ? &has : nullptr);
        CHECK((rc == 0) == ok);
        if (ok) {
            CHECK((L.mom && (mask & 1)) ? same(b, src[4]) : untouched(b));
            const vit_sgd_t& want = (mask & 2) ? (L.mom ? SGD : zero) : before;
            CHECK(memcmp(&sg, &want, sizeof sg) == 0);
            CHECK((mask & 4) ? st == (L.mom ? MSTEPS : 0) : st == -5);
            CHECK((mask & 8) ? has == (L.mom ? 1 : 0) : has == -5);
        } else {
            CHECK(untouched(b) && memcmp(&sg, &before, sizeof sg) == 0 && st == -5 && has == -5);
        }
    }
    {  // another config: the three array readers refuse
        vit_config_t other = CFG;
        other.num_classes += 1;
        std::vector<float> a((size_t)n, SENTINEL);
        CHECK(vit_checkpoint_read(p, &other, a.data(), nullptr, nullptr) != 0 && untouched(a));
        CHECK(vit_checkpoint_read_ema(p, &other, a.data(), nullptr, nullptr, nullptr) != 0 && untouched(a));
        CHECK(vit_checkpoint_read_momentum(p, &other, a.data(), nullptr, nullptr, nullptr) != 0 && untouched(a));
        CHECK(vit_checkpoint_read_ema(p, nullptr, nullptr, nullptr, nullptr, nullptr) != 0);
        CHECK(vit_checkpoint_read_momentum(p, nullptr, nullptr, nullptr, nullptr, nullptr) != 0);
    }
}

int main() {
    const long long n = vit_config_num_params(&CFG);
    g_what = "setup";
    CHECK(n == 311);
    char tmpl[] = "/tmp/vit_ckpt_roundtrip_XXXXXX";
    CHECK(mkdtemp(tmpl));
    const std::string dir = tmpl, path = dir + "/x.bin", other = dir + "/y.bin", bad = dir + "/bad.bin";
    const std::vector<float> src[5] = {filled(n, 1), filled(n, 2), filled(n, 3), filled(n, 4), filled(n, 5)};
    int files = 0, cuts = 0;
    for (int k = 0; k < 8; k++) {
        const Layout L{(k & 1) != 0, (k & 2) != 0, (k & 4) != 0};
        g_what = std::string("layout") + (L.opt ? " adamw" : "") + (L.ema ? " ema" : "") + (L.mom ? " momentum" : "");
        const float *m = L.opt ? src[1].data() : nullptr, *v = L.opt ? src[2].data() : nullptr;
        const float *e = L.ema ? src[3].data() : nullptr, *b = L.mom ? src[4].data() : nullptr;
        CHECK(vit_checkpoint_write_sgd(path.c_str(), &CFG, src[0].data(), m, v, STEP, &HP, e, DECAY, UPDATES, b, &SGD,
                                       MSTEPS) == 0);
        const std::vector<char> raw = slurp(path);
        const int sections = 1 + 2 * L.opt + L.ema + L.mom;
        CHECK((long long)raw.size() == VIT_CKPT_HEADER_BYTES + 4 * n * sections);
        CHECK(access((path + ".tmp").c_str(), F_OK) != 0);
        // the older writers give the same bytes for the layouts they can write
        if (!L.mom) {
            CHECK(vit_checkpoint_write_ex(other.c_str(), &CFG, src[0].data(), m, v, STEP, &HP, e, DECAY, UPDATES) == 0);
            CHECK(slurp(other) == raw);
        }
        if (!L.mom && !L.ema) {
            CHECK(vit_checkpoint_write(other.c_str(), &CFG, src[0].data(), m, v, STEP, &HP) == 0);
            CHECK(slurp(other) == raw);
        }
        read_all_ways(path, L, true, src);
        files++;
        // cuts: inside the header, and one byte either side of every section boundary (the end included:
        // one byte short, one byte long)
        std::vector<size_t> lens = {0, 4, 1023};
        for (int s = 0; s <= sections; s++) {
            const size_t at = (size_t)(VIT_CKPT_HEADER_BYTES + 4 * n * s);
            lens.push_back(at - 1);
            lens.push_back(at + 1);
        }
        for (size_t len : lens) {
            g_what += " cut";
            spit(bad, raw, len);
            read_all_ways(bad, L, false, src);
            cuts++;
        }
    }
    // bad arguments to the writer
    g_what = "writer arguments";
    CHECK(vit_checkpoint_write_sgd(path.c_str(), &CFG, src[0].data(), src[1].data(), nullptr, 0, nullptr, nullptr, 0.f, 0,
                                   nullptr, nullptr, 0) != 0);
    CHECK(vit_checkpoint_write_sgd(path.c_str(), &CFG, src[0].data(), nullptr, nullptr, 0, nullptr, src[3].data(), 0.5f, -1,
                                   nullptr, nullptr, 0) != 0);
    CHECK(vit_checkpoint_write_sgd(path.c_str(), &CFG, src[0].data(), nullptr, nullptr, 0, nullptr, nullptr, 0.f, 0,
                                   src[4].data(), nullptr, 0) != 0);
    CHECK(vit_checkpoint_write_sgd(path.c_str(), &CFG, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0.f, 0, nullptr,
                                   nullptr, 0) != 0);
    remove(path.c_str());
    remove(other.c_str());
    remove(bad.c_str());
    rmdir(dir.c_str());
    printf("checkpoint_roundtrip ok: %d layouts, %d cuts\n", files, cuts);
    return 0;
}
