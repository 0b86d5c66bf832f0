// render_graph_genes_rules_san.cpp -- the argument check of sots_render_graph_genes (render_graph_genes_check), the helper that
// says which operators run a chain and which of them take their index from a gene column (graph_gene_ops), the form rule
// (graph_genes_form) and the pass cap (graph_feedback_max_pass), all pure host code of csrc/sots_rules.h, driven stand-alone for
// an AddressSanitizer + UndefinedBehaviorSanitizer build with plain g++ (tests/test_render_graph_genes_cpu.py).  Prints
// "ok: <n> checks" and returns 0 when everything is as expected.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_rules.h"

static int checks = 0, failures = 0;

static void expect(const sots::Fault &f, int code, const char *needle, int line)
{
    ++checks;
    const bool named = f.code == SOTS_OK || strstr(f.text, "sots_render_graph_genes: ") == f.text; // every refusal names the call
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

static const uint32_t n = 1024, d = 7, rows = 7; // chain3 with one gene operator

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
        return sots::render_graph_genes_check(SOTS_SYNTH_GRAPH, a, n, d, values.data(), nbytes == ~(size_t)0 ? bytes : nbytes, num_rows, out.data(),
                                              out.size());
    };
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
        EXPECT(sots::render_graph_genes_check(kind, &a, n, d, values.data(), bytes, rows, out.data(), out.size()), SOTS_ERR_STATE,
               "the handle runs a fixed voice");
    EXPECT(check(nullptr), SOTS_ERR_INVALID, "null args");
    a = args(n, 0, 0, 0, 0, sizeof(sots_render_graph_feedback_args) - 4);
    EXPECT(check(&a), SOTS_ERR_INVALID, "sots_render_graph_feedback_args.struct_size");
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
    EXPECT(check(&a, bytes - 4), SOTS_ERR_SIZE, "196 bytes of values, got 192"); // 7 rows of the context's D = 7 genes
    EXPECT(check(&a, (size_t)rows * 6 * sizeof(float)), SOTS_ERR_SIZE, "196 bytes of values, got 168"); // rows without their gene column
    EXPECT(check(&a, bytes + 28), SOTS_ERR_SIZE, "bytes of values");
    EXPECT(check(&a, bytes, (1u << 21) - 1u), SOTS_ERR_SIZE, "bytes of values");
    EXPECT(check(&a, (size_t)(1u << 21) * d * sizeof(float), 1u << 21), SOTS_ERR_INVALID, "2^31");
    EXPECT(check(&a, bytes, 0xFFFFFFFFu), SOTS_ERR_INVALID, "2^31");
    a = args(1);
    EXPECT(check(&a, bytes, 0xFFFFFFFFu), SOTS_ERR_INVALID, "2^31");
    EXPECT(check(&a, bytes, 0x7FFFFFFFu - n), SOTS_ERR_SIZE, "bytes of values");
    a = args(n);
    EXPECT(sots::render_graph_genes_check(SOTS_SYNTH_GRAPH, &a, n, d, nullptr, bytes, rows, out.data(), out.size()), SOTS_ERR_SIZE, "values");
    EXPECT(sots::render_graph_genes_check(SOTS_SYNTH_GRAPH, &a, n, d, values.data(), bytes, rows, nullptr, out.size()), SOTS_ERR_INVALID, "null output");
    EXPECT(sots::render_graph_genes_check(SOTS_SYNTH_GRAPH, &a, n, d, values.data(), bytes, rows, nullptr, 0), SOTS_OK, nullptr);

    // ---- the two entry points of the fixed setting keep their refusal of a gene context, code and text ----
    {
        const sots::Fault f = sots::render_graph_feedback_check(SOTS_SYNTH_GRAPH, &a, n, d, values.data(), bytes, rows, out.data(), out.size(), 0b010);
        TRUE(f.code == SOTS_ERR_STATE &&
                 !strcmp(f.text, "sots_render_graph_feedback: the feedback indices of operators 0x2 are genes (sots_create_graph_genes): every row "
                                 "has its own; sots_render_overlap_add renders such a voice"),
             "sots_render_graph_feedback refuses a gene context as before");
        const float none[8] = {0};
        sots_render_continuous_args ca;
        ca.struct_size = sizeof ca, ca.hop = n, ca.flags = 0, ca.samples_per_pass = 0;
        const sots::Fault g = sots::render_graph_continuous_check(SOTS_SYNTH_GRAPH, none, &ca, n, d, values.data(), bytes, rows, out.data(), out.size(), 0b010);
        TRUE(g.code == SOTS_ERR_STATE &&
                 !strcmp(g.text, "sots_render_graph_continuous: the feedback indices of operators 0x2 are genes (sots_create_graph_genes): every "
                                 "row has its own; sots_render_overlap_add renders such a voice"),
             "sots_render_graph_continuous refuses a gene context as before");
    }

    // ---- which operators run a chain, which take their index from a gene column, and the column: every mask at OPS = 3 ----
    for (uint32_t mask = 0; mask < 8u; ++mask)
        for (uint32_t fixed = 0; fixed < 8u; ++fixed) {
            if (mask & fixed) continue; // (sots_set_voice_feedback refuses an index other than 0 on a gene operator)
            float beta[8] = {0};
            for (uint32_t j = 0; j < 3u; ++j) beta[j] = fixed >> j & 1u ? 0.5f + (float)j : 0.0f;
            const sots::GraphGeneOps g = sots::graph_gene_ops(3, mask, beta);
            TRUE(g.genes == mask && g.flagged == (mask | fixed), "the flagged set is the mask and the operators with an index other than 0");
            uint32_t next = 6; // 2 OPS: the columns follow the mask's set bits, ascending
            for (uint32_t j = 0; j < 8u; ++j) {
                if (mask >> j & 1u) {
                    TRUE(g.column[j] == next && g.column[j] == sots::feedback_gene_column(3, mask, j), "a gene operator's column");
                    ++next;
                } else {
                    TRUE(g.column[j] == 0u, "no column where the index is no gene");
                }
            }
            TRUE(next == sots::graph_dims(3, mask), "the columns end where the row ends");
        }
    {
        float beta[8] = {0};
        beta[7] = 1.0f; // beyond the operators: not looked at
        const sots::GraphGeneOps g = sots::graph_gene_ops(3, 0, beta);
        TRUE(g.flagged == 0u && g.genes == 0u, "nothing beyond the operators is flagged");
    }

    // ---- the form rule ----
    for (float beta : {0.0f, 1e-10f, 0.25f, 1.0f, 1.5f, 0x1.800002p+0f, 2.0f}) {
        TRUE(sots::graph_genes_form(sots::kChainLibrary, true, beta) == sots::kChainRelax, "a gene operator is relaxed under the library's choice");
        if (beta != 0.0f)
            TRUE(sots::graph_genes_form(sots::kChainLibrary, false, beta) == sots::graph_feedback_form(beta), "a fixed-index operator keeps its rule");
        for (bool gene : {false, true}) {
            TRUE(sots::graph_genes_form(sots::kChainSerial, gene, beta) == sots::kChainSerial, "chain_form 1 forces the serial form");
            TRUE(sots::graph_genes_form(sots::kChainRelax, gene, beta) == sots::kChainRelax, "chain_form 2 forces the relaxation");
        }
    }
    TRUE(sots::graph_genes_form(sots::kChainLibrary, false, 2.0f) == sots::kChainSerial, "a fixed index of 2 is still rendered serially");
    TRUE(sots::kRelaxCapLibrary == 1024u && sots::kRelaxCapLibrary <= sots::kRelaxCapMax, "the library's cap");

    // ---- the pass cap, gene operators counted among the flagged: whole tiles of 4096, at most 1024 of them, within 96 MiB ----
    for (uint32_t ops = 2; ops <= 8; ++ops)
        for (uint32_t fb = 0; fb <= ops; ++fb) {
            const uint64_t cap = sots::graph_feedback_max_pass(ops, fb), buffers = ops + fb;
            TRUE(cap % 4096u == 0 && cap >= 4096u && cap / 4096u <= 1024u && cap * buffers * 4u <= (96ull << 20) &&
                     (cap == (1u << 22) || (cap + 4096u) * buffers * 4u > (96ull << 20)),
                 "the pass cap");
        }
    {
        float beta[8] = {0.5f, 0, 0, 0, 0, 0, 0, 0};
        const sots::GraphGeneOps g = sots::graph_gene_ops(8, 0b11111110, beta);
        TRUE(sots::graph_feedback_max_pass(8, (uint32_t)__builtin_popcount(g.flagged)) == 1572864u, "eight flagged operators of eight");
    }

    // ---- the effective index, as the chain kernels make it ----
    TRUE(sots::effective_feedback(-1.0f) == 0.0f && sots::effective_feedback(3.0f) == 2.0f && sots::effective_feedback(0.5f) == 0.5f &&
             sots::effective_feedback(__builtin_nanf("")) == 0.0f && !__builtin_signbit(sots::effective_feedback(-0.0f)) &&
             sots::effective_feedback(__builtin_inff()) == 2.0f && sots::effective_feedback(-__builtin_inff()) == 0.0f,
         "effective_feedback");
    static_assert(sots::effective_feedback(1.0f) == 1.0f, "a constant expression: device code calls it");
    if (failures) return printf("%d of %d checks failed\n", failures, checks), 1;
    printf("ok: %d checks\n", checks);
    return 0;
}
