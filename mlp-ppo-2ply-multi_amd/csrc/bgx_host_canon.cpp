// bgx_host_canon.cpp — bgx_harvest_canonical and its workspace size (declared
// in include/bgx.h): argument checks and the two launches of bgx_canon.hip.
// No allocation, no pointer query and no wait: the call can be captured.
#include <cstdint>

#include "bgx_canon.h"
#include "bgx_host.h"

namespace {

struct Range {
    const char* name;
    uintptr_t lo, hi;   // [lo, hi)
    bool output;
};

bool overlap(const Range& a, const Range& b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

int bgx_harvest_canonical_workspace(int n_eps, int lanes, uint64_t* bytes) {
    return guarded("bgx_harvest_canonical_workspace", [&]() -> int {
        if (n_eps < 0 || lanes < 1 || !bytes)
            return fail(BGX_E_ARG, "bgx_harvest_canonical_workspace: n_eps=%d lanes=%d", n_eps, lanes);
        *bytes = bgx::canon_work_bytes(n_eps, lanes);
        return BGX_OK;
    });
}

int bgx_harvest_canonical(const uint32_t* d_headers, const uint32_t* d_records, int n_eps, int n_records,
                          int lane_base, int lanes, uint32_t* d_out_headers, uint32_t* d_out_records,
                          int32_t* d_out_offs, uint32_t* d_status, void* d_work, uint64_t work_bytes, void* stream) {
    return guarded("bgx_harvest_canonical", [&]() -> int {
        const char* name = "bgx_harvest_canonical";
        if (n_eps < 0 || n_records < 0 || lane_base < 0 || lanes < 1)
            return fail(BGX_E_ARG, "%s: n_eps=%d n_records=%d lane_base=%d lanes=%d", name, n_eps, n_records,
                        lane_base, lanes);
        if (!d_out_offs || !d_status) return fail(BGX_E_ARG, "%s: null d_out_offs / d_status", name);
        if ((n_eps > 0 && (!d_headers || !d_out_headers || !d_work)) || (n_records > 0 && (!d_records || !d_out_records)))
            return fail(BGX_E_ARG, "%s: null pointer", name);
        if ((uintptr_t)d_out_offs % 4 != 0 || (uintptr_t)d_status % 4 != 0)
            return fail(BGX_E_ARG, "%s: d_out_offs / d_status is not 4-byte aligned", name);
        // headers and records move as 16-byte words
        if ((uintptr_t)d_headers % 16 != 0 || (uintptr_t)d_out_headers % 16 != 0 || (uintptr_t)d_records % 16 != 0 ||
            (uintptr_t)d_out_records % 16 != 0 || (uintptr_t)d_work % 16 != 0)
            return fail(BGX_E_ARG, "%s: headers, records and d_work must be 16-byte aligned", name);
        const uint64_t need = bgx::canon_work_bytes(n_eps, lanes);
        if (n_eps > 0 && work_bytes < need)
            return fail(BGX_E_ARG, "%s: work_bytes=%llu < %llu (bgx_harvest_canonical_workspace)", name,
                        (unsigned long long)work_bytes, (unsigned long long)need);
        const uint64_t hb = (uint64_t)n_eps * 64, rb = (uint64_t)n_records * 48;
        const Range r[] = {
            {"d_headers", (uintptr_t)d_headers, (uintptr_t)d_headers + hb, false},
            {"d_records", (uintptr_t)d_records, (uintptr_t)d_records + rb, false},
            {"d_out_headers", (uintptr_t)d_out_headers, (uintptr_t)d_out_headers + hb, true},
            {"d_out_records", (uintptr_t)d_out_records, (uintptr_t)d_out_records + rb, true},
            {"d_out_offs", (uintptr_t)d_out_offs, (uintptr_t)d_out_offs + ((uint64_t)n_eps + 1) * 4, true},
            {"d_status", (uintptr_t)d_status, (uintptr_t)d_status + 4, true},
            {"d_work", (uintptr_t)d_work, (uintptr_t)d_work + (n_eps > 0 ? need : 0), true},
        };
        constexpr int NR = (int)(sizeof(r) / sizeof(r[0]));
        for (int i = 0; i < NR; ++i)
            for (int j = i + 1; j < NR; ++j)
                if ((r[i].output || r[j].output) && overlap(r[i], r[j]))
                    return fail(BGX_E_ARG, "%s: %s overlaps %s", name, r[j].name, r[i].name);
        if (n_eps == 0) {   // d_out_offs[0] = 0, nothing else
            HIP_TRY(bgx_launch_episode_offsets(nullptr, 0, d_out_offs, (hipStream_t)stream));
            return BGX_OK;
        }
        const bgx::CanonWork w = bgx::canon_work(d_work, n_eps, lanes);
        HIP_TRY(bgx_launch_canon_index(d_headers, n_eps, n_records, (uint32_t)lane_base, lanes, d_out_offs, d_status, w,
                                       (hipStream_t)stream));
        HIP_TRY(bgx_launch_canon_copy(d_headers, d_records, n_eps, n_records, w, d_out_offs, d_out_headers,
                                      d_out_records, (hipStream_t)stream));
        return BGX_OK;
    });
}

}  // extern "C"
