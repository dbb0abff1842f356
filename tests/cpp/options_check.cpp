// options_check.cpp -- what the option table (raytracer.glsl_amd/csrc/rt_options.hpp) decides, on the host alone.  Reads lines from
// standard input and answers each with one line:
//   reset             a default Options                          -> "ok"
//   set KEY VALUE     find + set, as rtgl_set_option             -> "ok" | "refused MESSAGE" | "unknown"
//   get KEY           find + the field, as rtgl_get_option       -> "value N" | "unknown"
//   env NAME TEXT     read_environment over a DEFAULT Options with NAME=TEXT (TEXT: the rest of the line, as it stands) and nothing else
//                     set; answers the field of NAME's row       -> "value N set|kept" | "unknown"
//   rows              the table                                  -> one line "row KEY ENV FLAGS" per row ("-": none), then "ok"
// Exit status 0 unless a line could not be read.  (tests/test_options.py builds this with the address and undefined-behaviour
// sanitizers and compares the answers with the replies recorded from the library, tests/golden/option_replies.json.)
#include "../../raytracer.glsl_amd/csrc/rt_options.hpp"

#include <cstdio>
#include <string>

namespace op = rt_options;
static std::string g_name, g_text;
static const char *one_variable(const char *name) { return g_name == name ? g_text.c_str() : nullptr; }

int main()
{
    op::Options opt;
    char line[512];
    while (std::fgets(line, sizeof line, stdin)) {
        std::string s(line);
        if (s.empty() || s.back() != '\n') { std::fprintf(stderr, "line too long or unterminated: %s\n", line); return 2; }
        s.pop_back();
        char key[128]; int value = 0;
        if (s == "reset") { opt = op::Options(); std::puts("ok"); }
        else if (s == "rows") {
            for (const op::Row &row : op::kRows) std::printf("row %s %s %u\n", row.key ? row.key : "-", row.env ? row.env : "-", row.flags);
            std::puts("ok");
        } else if (std::sscanf(s.c_str(), "set %127s %d", key, &value) == 2) {
            const op::Row *row = op::find(key);
            if (!row || !(row->flags & op::kSet)) std::puts("unknown");
            else if (const char *message = op::set(opt, *row, value)) std::printf("refused %s\n", message);
            else std::puts("ok");
        } else if (std::sscanf(s.c_str(), "get %127s", key) == 1) {
            const op::Row *row = op::find(key);
            if (!row || !(row->flags & op::kGet)) std::puts("unknown");
            else std::printf("value %d\n", opt.*row->field);
        } else if (std::sscanf(s.c_str(), "env %127s", key) == 1 && s.size() >= 5 + std::strlen(key)) {
            g_name = key; g_text = s.substr(5 + g_name.size());
            const op::Row *row = nullptr;
            for (const op::Row &r : op::kRows) if (r.env && g_name == r.env) row = &r;
            if (!row) { std::puts("unknown"); continue; }
            op::Options fresh;
            const uint32_t rows = op::read_environment(fresh, one_variable);
            std::printf("value %d %s\n", fresh.*row->field, rows & op::row_bit(row->field) ? "set" : "kept");
        } else { std::fprintf(stderr, "not understood: %s\n", s.c_str()); return 2; }
    }
    return 0;
}
