// render_continuous_rules_san.cpp -- the argument check of sots_render_continuous (render_continuous_check,
// csrc/sots_rules.h: pure host code) driven stand-alone, for an AddressSanitizer + UndefinedBehaviorSanitizer build with plain
// g++ (tests/test_render_continuous_cpu.py).  Prints "ok: <n> checks" and returns 0 when every code and text is the expected one.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_rules.h"

static int checks = 0, failures = 0;

static void expect(const sots::Fault &f, int code, const char *needle, int line)
{
    ++checks;
    if (f.code != code || (needle && !strstr(f.text, needle))) {
        printf("line %d: code %d (want %d), text \"%s\" (want \"%s\")\n", line, f.code, code, f.text, needle ? needle : "");
        ++failures;
    }
}
#define EXPECT(f, code, needle) expect((f), (code), (needle), __LINE__)

static const uint32_t n = 1024, d = 6, rows = 7;

int main()
{
    std::vector<float> values((size_t)rows * d, 0.5f), out((size_t)(rows - 1) * n + n);
    const size_t bytes = values.size() * sizeof(float);
    auto args = [](uint32_t hop, uint32_t flags = 0, uint32_t per_pass = 0, uint32_t size = sizeof(sots_render_continuous_args)) {
        sots_render_continuous_args a;
        a.struct_size = size, a.hop = hop, a.flags = flags, a.samples_per_pass = per_pass;
        return a;
    };
    auto check = [&](const sots_render_continuous_args *a, uint32_t arith = SOTS_ARITH_CPU_PATH, size_t nbytes = ~(size_t)0, uint32_t num_rows = rows,
                     const float *o = nullptr, uint64_t out_samples = ~0ull) {
        return sots::render_continuous_check(a, n, d, arith, values.data(), nbytes == ~(size_t)0 ? bytes : nbytes, num_rows, o ? o : out.data(),
                                             out_samples == ~0ull ? out.size() : out_samples);
    };
    sots_render_continuous_args a = args(n);
    EXPECT(check(&a), SOTS_OK, nullptr);
    a = args(1, SOTS_RENDER_GLIDE, 4097);
    EXPECT(check(&a), SOTS_OK, nullptr);
    EXPECT(check(nullptr), SOTS_ERR_INVALID, "null args");
    a = args(n, 0, 0, sizeof(sots_render_continuous_args) - 4);
    EXPECT(check(&a), SOTS_ERR_INVALID, "struct_size");
    a = args(n, 0, 0, sizeof(sots_render_continuous_args) + 4);
    EXPECT(check(&a), SOTS_ERR_INVALID, "struct_size");
    a = args(0);
    EXPECT(check(&a), SOTS_ERR_INVALID, "hop 0 outside 1..1024");
    a = args(n + 1);
    EXPECT(check(&a), SOTS_ERR_INVALID, "hop 1025 outside 1..1024");
    a = args(0xFFFFFFFFu);
    EXPECT(check(&a), SOTS_ERR_INVALID, "outside 1..1024");
    a = args(n, 2);
    EXPECT(check(&a), SOTS_ERR_INVALID, "unknown flags 0x2");
    a = args(n, 0x80000001u);
    EXPECT(check(&a), SOTS_ERR_INVALID, "unknown flags");
    a = args(n);
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, 0, 0), SOTS_ERR_INVALID, "num_rows");
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes - 4), SOTS_ERR_SIZE, "168 bytes of values, got 164");
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes + 24), SOTS_ERR_SIZE, "bytes of values");
    // S = (num_rows - 1) hop + N: 2^31 - 1024 + ... below the limit is a size question, at and above it INVALID whatever the bytes say
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes, (1u << 21) - 1u), SOTS_ERR_SIZE, "bytes of values");
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes, 1u << 21), SOTS_ERR_INVALID, "2^31");
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes, 0xFFFFFFFFu), SOTS_ERR_INVALID, "2^31");
    a = args(1);
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes, 0xFFFFFFFFu), SOTS_ERR_INVALID, "2^31");
    EXPECT(check(&a, SOTS_ARITH_CPU_PATH, bytes, 0x7FFFFFFFu - n), SOTS_ERR_SIZE, "bytes of values");
    a = args(n);
    EXPECT(sots::render_continuous_check(&a, n, d, SOTS_ARITH_CPU_PATH, nullptr, bytes, rows, out.data(), out.size()), SOTS_ERR_SIZE, "values");
    EXPECT(sots::render_continuous_check(&a, n, d, SOTS_ARITH_CPU_PATH, values.data(), bytes, rows, nullptr, out.size()), SOTS_ERR_INVALID, "null output");
    EXPECT(sots::render_continuous_check(&a, n, d, SOTS_ARITH_CPU_PATH, values.data(), bytes, rows, nullptr, 0), SOTS_OK, nullptr);
    EXPECT(check(&a, SOTS_ARITH_DEVICE_KERNELS), SOTS_ERR_STATE, "SOTS_ARITH_DEVICE_KERNELS");
    if (failures) return printf("%d of %d checks failed\n", failures, checks), 1;
    printf("ok: %d checks\n", checks);
    return 0;
}
