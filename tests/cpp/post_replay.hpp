// What the four *_plan_check programs share when they replay tests/golden/post_replies.json (tests/test_post_plans.py): a line of standard
// input is a verb and integers; a parameter record comes as its 32-bit words, or as the word "null" for a NULL pointer (the defaults stay).
// An answer is one line: "0" and what a success left, "<rc>\t<entry point>: <message>", or "tiled" where the refusal's text is rtgl_amd.hip's.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace post_replay {

constexpr int kInvalid = -1, kState = -4;      // (RTGL_ERR_INVALID, RTGL_ERR_STATE)

struct Line { std::string verb; std::vector<long long> n; bool null_record = false; };

inline bool next(Line &line)
{
    std::string text, word;
    if (!std::getline(std::cin, text)) return false;
    std::istringstream in(text);
    line = Line{};
    in >> line.verb;
    while (in >> word) {
        if (word == "null") line.null_record = true;
        else line.n.push_back(std::stoll(word));
    }
    return true;
}

// the record of a line over the defaults in `p`
template <typename P> void take(const Line &line, P &p)
{
    if (line.null_record) return;
    uint32_t words[sizeof(P) / 4];
    for (size_t k = 0; k < sizeof(P) / 4; ++k) words[k] = (uint32_t)line.n.at(k);
    std::memcpy(&p, words, sizeof p);
}

inline bool refuse(int rc, const char *who, const char *why)
{
    if (why) std::printf("%d\t%s: %s\n", rc, who, why);
    return why != nullptr;
}

}  // namespace post_replay
