// render_graph_feedback_rules_san.cpp -- the argument check of sots_render_graph_feedback (render_graph_feedback_check), its
// pass cap (graph_feedback_max_pass) and the library's choice of chain form (graph_feedback_form), all pure host code of
// csrc/sots_rules.h, driven stand-alone for an AddressSanitizer + UndefinedBehaviorSanitizer build with plain g++
// (tests/test_render_graph_feedback_cpu.py).  Prints "ok: <n> checks" and returns 0 when everything is as expected.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_rules.h"

static int checks = 0, failures = 0;

static void expect(const sots::Fault &f, int code, const char *needle, int line)
{
    ++checks;
    const bool named = f.code == SOTS_OK || strstr(f.text, "sots_render_graph_feedback: ") == f.text; // every refusal names the call
    if (f.code != code || !named || (needle && !strstr(f.text, needle))) {
        printf("line %d: code %d (want %d), text \"%s\" (want \"%s\")\n", line, f.code, code, f.text, needle ? needle : "");
        ++failures;
    }
}
#define EXPECT(f, code, needle) expect((f), (code), (needle), __LINE__)
static void truth(bool ok, const char *what, int line)
{
    ++checks;
    if (!ok) {
        printf("line %d: %s\n", line, what);
        ++failures;
    }
}
#define TRUE(ok, what) truth((ok), (what), __LINE__)

static const uint32_t n = 1024, d = 6, rows = 7;

int main()
{
    std::vector<float> values((size_t)rows * d, 0.5f), out((size_t)(rows - 1) * n + n);
    const size_t bytes = values.size() * sizeof(float);
    auto args = [](uint32_t hop, uint32_t flags = 0, uint32_t per_pass = 0, uint32_t form = 0, uint32_t cap = 0,
                   uint32_t size = sizeof(sots_render_graph_feedback_args)) {
        sots_render_graph_feedback_args a;
        a.struct_size = size, a.hop = hop, a.flags = flags, a.samples_per_pass = per_pass, a.chain_form = form, a.relax_cap = cap;
        return a;
    };
    auto check = [&](const sots_render_graph_feedback_args *a, size_t nbytes = ~(size_t)0, uint32_t num_rows = rows) {
        return sots::render_graph_feedback_check(SOTS_SYNTH_GRAPH, a, n, d, values.data(), nbytes == ~(size_t)0 ? bytes : nbytes, num_rows, out.data(),
                                                 out.size());
    };
    TRUE(sizeof(sots_render_graph_feedback_args) == 24, "sots_render_graph_feedback_args is six 32-bit words");
    sots_render_graph_feedback_args a = args(n);
    EXPECT(check(&a), SOTS_OK, nullptr);
    for (uint32_t form = 0; form <= 2; ++form)
        for (uint32_t cap : {0u, 1u, 8u, 4096u}) {
            a = args(1, SOTS_RENDER_GLIDE, 4097, form, cap);
            EXPECT(check(&a), SOTS_OK, nullptr);
        }
    // ---- one fault at a time ----
    a = args(n);
    for (uint32_t kind : {(uint32_t)SOTS_SYNTH_2OP, (uint32_t)SOTS_SYNTH_3OP_SERIES, (uint32_t)SOTS_SYNTH_TRIPLE_PAR, (uint32_t)SOTS_SYNTH_4OP_SERIES})
        EXPECT(sots::render_graph_feedback_check(kind, &a, n, d, values.data(), bytes, rows, out.data(), out.size()), SOTS_ERR_STATE,
               "the handle runs a fixed voice");
    EXPECT(check(nullptr), SOTS_ERR_INVALID, "null args");
    a = args(n, 0, 0, 0, 0, sizeof(sots_render_graph_feedback_args) - 4);
    EXPECT(check(&a), SOTS_ERR_INVALID, "struct_size");
    a = args(n, 0, 0, 0, 0, sizeof(sots_render_continuous_args)); // the other renderers' argument block is not this one's
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
    a = args(n, 0, 0, 3);
    EXPECT(check(&a), SOTS_ERR_INVALID, "chain_form 3 is not a form");
    a = args(n, 0, 0, 0xFFFFFFFFu);
    EXPECT(check(&a), SOTS_ERR_INVALID, "chain_form");
    a = args(n, 0, 0, 2, 4097);
    EXPECT(check(&a), SOTS_ERR_INVALID, "relax_cap 4097 outside 0..4096");
    a = args(n, 0, 0, 1, 0xFFFFFFFFu); // (checked whatever the form)
    EXPECT(check(&a), SOTS_ERR_INVALID, "relax_cap");
    a = args(n);
    EXPECT(check(&a, 0, 0), SOTS_ERR_INVALID, "num_rows");
    EXPECT(check(&a, bytes - 4), SOTS_ERR_SIZE, "168 bytes of values, got 164");
    EXPECT(check(&a, bytes + 24), SOTS_ERR_SIZE, "bytes of values");
    EXPECT(check(&a, bytes, (1u << 21) - 1u), SOTS_ERR_SIZE, "bytes of values");
    EXPECT(check(&a, (size_t)(1u << 21) * d * sizeof(float), 1u << 21), SOTS_ERR_INVALID, "2^31");
    EXPECT(check(&a, bytes, 0xFFFFFFFFu), SOTS_ERR_INVALID, "2^31");
    a = args(1);
    EXPECT(check(&a, bytes, 0xFFFFFFFFu), SOTS_ERR_INVALID, "2^31");
    EXPECT(check(&a, bytes, 0x7FFFFFFFu - n), SOTS_ERR_SIZE, "bytes of values");
    a = args(n);
    EXPECT(sots::render_graph_feedback_check(SOTS_SYNTH_GRAPH, &a, n, d, nullptr, bytes, rows, out.data(), out.size()), SOTS_ERR_SIZE, "values");
    EXPECT(sots::render_graph_feedback_check(SOTS_SYNTH_GRAPH, &a, n, d, values.data(), bytes, rows, nullptr, out.size()), SOTS_ERR_INVALID, "null output");
    EXPECT(sots::render_graph_feedback_check(SOTS_SYNTH_GRAPH, &a, n, d, values.data(), bytes, rows, nullptr, 0), SOTS_OK, nullptr);

    // ---- the pass cap: whole tiles of 4096, at most 1024 of them, phase words and t buffers of a pass within 96 MiB ----
    for (uint32_t ops = 2; ops <= 8; ++ops)
        for (uint32_t fb = 0; fb <= ops; ++fb) {
            const uint64_t cap = sots::graph_feedback_max_pass(ops, fb), buffers = ops + fb;
            TRUE(cap % 4096u == 0 && cap >= 4096u && cap / 4096u <= 1024u && cap * buffers * 4u <= (96ull << 20) &&
                     (cap == (1u << 22) || (cap + 4096u) * buffers * 4u > (96ull << 20)),
                 "the pass cap");
            if (fb == 0) TRUE(cap == sots::graph_continuous_max_pass(ops), "without feedback operators the cap is sots_render_graph_continuous's");
        }
    TRUE(sots::graph_feedback_max_pass(2, 2) == 1u << 22 && sots::graph_feedback_max_pass(3, 3) == 1u << 22 &&
             sots::graph_feedback_max_pass(8, 8) == 1572864u && sots::graph_feedback_max_pass(8, 3) == 2285568u,
         "the caps as computed by hand");

    // ---- the library's choice of form: one of the two forms for every index that can be set, and a cap within the range ----
    for (float beta : {1e-10f, 0.25f, 0.5f, 0.75f, 1.0f, 1.5f, 2.0f}) {
        const uint32_t form = sots::graph_feedback_form(beta);
        TRUE(form == sots::kChainSerial || form == sots::kChainRelax, "the library's form is a form");
        TRUE(form == (beta <= 1.5f ? sots::kChainRelax : sots::kChainSerial), "relaxation up to the last index at which it was measured to win, 1.5");
    }
    TRUE(sots::graph_feedback_form(0x1.800002p+0f) == sots::kChainSerial, "the next index above 1.5 is rendered serially");
    TRUE(sots::kRelaxCapLibrary >= 1u && sots::kRelaxCapLibrary <= sots::kRelaxCapMax && sots::kRelaxCapMax == 4096u, "the library's cap");
    if (failures) return printf("%d of %d checks failed\n", failures, checks), 1;
    printf("ok: %d checks\n", checks);
    return 0;
}
