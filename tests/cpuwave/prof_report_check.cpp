// prof_report_check.cpp — the fused development report (csrc/bgx_host_prof.cpp)
// on a synthetic clock buffer: the lines that pick single workgroups (median,
// slowest, last launch shape) must read those workgroups' slots, kProfSlotWords
// apart. Linked against the report's source only; built with
// -fsanitize=address,undefined (tests/test_prof_report.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bgx_prof.h"

static int failures = 0;

static void expect(const std::string& text, const char* want) {
    if (text.find(want) == std::string::npos) {
        fprintf(stderr, "missing: %s\n", want);
        ++failures;
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* dump = argv[1];
    // workgroups 300..999 ran the last launch; workgroup b began at 5000 + b and
    // took 1000 + 10 (b - 300) ticks (100 per us): the median of the 700 is
    // workgroup 650 (45.0 us), the slowest 999 (79.9 us). Prologue 300 ticks,
    // epilogue 500, the loop in between; shader cycles 24 per tick (2400 MHz).
    const int first = 300, last = 999, n_active = last - first + 1;
    std::vector<unsigned long long> p((size_t)kProfSlots * kProfSlotWords, 0);
    for (int b = 0; b < kProfSlots; ++b) {
        unsigned long long* q = &p[(size_t)b * kProfSlotWords];
        q[5] = 1;                   // workgroup steps
        q[18] = 16;                 // wave-steps
        q[26] = 100000 + b;         // rows
        q[27] = 200000 + b;         // tier-2 jobs
        q[28] = 300000 + b;         // lane-steps
        if (b < first || b > last) continue;   // begin = end = 0: did not run
        const unsigned long long begin = 5000 + b, dur = 1000 + 10ull * (b - first);
        q[24] = begin;
        q[19] = begin + 300;
        q[20] = begin + dur - 500;
        q[25] = begin + dur;
        q[21] = dur * 24;
    }
    char* buf = nullptr;
    size_t len = 0;
    FILE* out = open_memstream(&buf, &len);
    if (!out) return 2;
    fused_prof_report(p.data(), kProfSlots, out, dump);
    fclose(out);
    const std::string text(buf, len);
    free(buf);
    fputs(text.c_str(), stdout);

    expect(text, "last launch, 700 workgroups: duration us min 10.0 p50 45.0");
    expect(text, "max 79.9; begin skew 7.0 us, span 86.9 us; lane-steps 300999; rows / tier-2 jobs: "
                 "median workgroup 100650 / 200650, slowest 100999 / 200999");
    expect(text, "last launch shape (median workgroup): prologue 3.0 us, step loop 37.0 us, epilogue 5.0 us; "
                 "shader clock 2400 MHz");

    // the dump: a header, then one line per workgroup that ran, with its own words
    FILE* fp = fopen(dump, "r");
    if (!fp) return 2;
    char line[256];
    int lines = 0;
    bool saw_median = false;
    while (fgets(line, sizeof(line), fp)) {
        ++lines;
        if (!strcmp(line, "650,5650,10150,5950,9650,100650,200650,300650\n")) saw_median = true;
    }
    fclose(fp);
    if (lines != 1 + n_active || !saw_median) {
        fprintf(stderr, "dump: %d lines (want %d), median workgroup's line %s\n", lines, 1 + n_active,
                saw_median ? "found" : "missing");
        ++failures;
    }
    return failures ? 1 : 0;
}
