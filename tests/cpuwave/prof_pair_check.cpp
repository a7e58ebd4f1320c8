// prof_pair_check.cpp — the pairing survey lines of the fused development
// report (csrc/bgx_host_prof.cpp) on a synthetic clock buffer: words 88..94 of
// every workgroup slot, summed over the slots, against the item clocks in
// words 8, 10, 14 and 16. Linked against the report's source only; built with
// -fsanitize=address,undefined (tests/test_prof_pair_report.py).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bgx_prof.h"

int main() {
    // 1,024 workgroups, 10 workgroup steps each. Per workgroup: item clocks
    // 4,000 + 1,000 + 2,000 + 3,000 = 10,000 ticks (100 per us); 5 rule-mode
    // two-move jobs of 400 ticks together (0.80 us each, 0.40 wave-us per
    // workgroup step, 4.0 % of the items); 9 pipelined claims, 4 of a
    // rule-mode non-doubles lane, 1 of those with a partner (25.0 %).
    std::vector<unsigned long long> p((size_t)kProfSlots * kProfSlotWords, 0);
    for (int b = 0; b < kProfSlots; ++b) {
        unsigned long long* q = &p[(size_t)b * kProfSlotWords];
        q[5] = 10;
        q[18] = 120;
        q[8] = 4000;
        q[10] = 1000;
        q[14] = 2000;
        q[16] = 3000;
        q[88] = 400;
        q[89] = 5;
        q[90] = 9;
        q[91] = 4;
        q[92] = 1;
        q[93] = 0;   // no pair items: the item clocks above are all
        q[94] = 0;
    }
    char* buf = nullptr;
    size_t len = 0;
    FILE* out = open_memstream(&buf, &len);
    if (!out) return 2;
    fused_prof_report(p.data(), kProfSlots, out, nullptr);
    fclose(out);
    const std::string text(buf, len);
    free(buf);
    fputs(text.c_str(), stdout);
    int failures = 0;
    const char* want[] = {
        "tier-1 rule-mode two-move job: 0.80 us (5120 jobs), 0.40 wave-us per workgroup step, 4.0 % of the item "
        "wave-us\n",
        "pipelined job claims 9216: 4096 of a rule-mode non-doubles lane, 1024 of them (25.0 %) with a second such "
        "lane ready and unclaimed\n",
        "tier-1 pair items: 0 pairs formed (0.00 per workgroup step), 0.00 us each, 0.00 wave-us per workgroup step\n",
    };
    for (const char* w : want)
        if (text.find(w) == std::string::npos) {
            fprintf(stderr, "missing: %s", w);
            ++failures;
        }
    return failures ? 1 : 0;
}
