// render_mode_test.cpp -- CPU-only check of the renderMode key (no GPU, no libsots_hip): prints, for every JSON text on
// the command line, "mode <text> -> given <0|1> renderMode <n>" or "mode <text> -> refused: <the refusal's text>", which
// tests/test_render_continuous_cpu.py compares.
#include <cstdio>
#include <string>

#include "Match_JSON.hpp"

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        try {
            const std::string text = argv[i];
            const Json h = JsonParser(text).value();
            uint32_t mode = 0;
            const bool given = readRenderModeKey(h, mode);
            printf("mode %s -> given %d renderMode %u\n", argv[i], (int)given, mode);
        } catch (const std::exception &e) {
            printf("mode %s -> refused: %s\n", argv[i], e.what());
        }
    }
    return 0;
}
