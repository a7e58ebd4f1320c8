// bgx_prof.h — the fused kernel's development report (BGX_FUSED_PROF): the
// shape of its clock buffer and the host function that prints it
// (bgx_host_prof.cpp). Plain C++: no HIP, no engine types.
#pragma once

#include <cstdio>

// one slot per workgroup, kProfSlotWords u64 words each (bgx_fused.hip PROF_STRIDE)
constexpr int kProfSlotWords = 128;
constexpr int kProfSlots = 1024;

// Per workgroup-step averages over all launches (wall clock, 100 MHz) and the
// last launch's per-workgroup spread, printed to `out`; dump_path (or null):
// a CSV of the last launch, one line per workgroup that ran.
__attribute__((visibility("hidden"))) void fused_prof_report(const unsigned long long* slots, int n_slots, FILE* out,
                                                              const char* dump_path);
