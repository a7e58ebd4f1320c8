// bgx_host_copy.cpp — copies across the boundary: page-locked host ranges,
// stream copies, DMA-engine copies through the HSA runtime, and IPC handles.
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstring>
#include <mutex>

#include "bgx_host.h"

// ---- DMA-engine copies (SDMA through the HSA runtime). On this ROCm the HIP
// runtime serves device <-> host hipMemcpyAsync with blit kernels, which need
// compute units and so queue behind a persistent kernel; these copies go to a
// DMA engine explicitly (hsa_amd_memory_async_copy_on_engine, forced SDMA).
namespace {
struct DmaDev {
    bool ready = false;
    hsa_agent_t gpu{}, cpu{};
    hsa_amd_sdma_engine_id_t engine = HSA_AMD_SDMA_ENGINE_0;
};
std::mutex g_dma_mu;
DmaDev g_dma[64];

struct AgentQuery {
    uint32_t bdf = 0, domain = 0;
    hsa_agent_t gpu{}, cpu{};
    bool have_gpu = false, have_cpu = false;
};

hsa_status_t find_agents(hsa_agent_t a, void* data) {
    AgentQuery* q = (AgentQuery*)data;
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_CPU && !q->have_cpu) {
        q->cpu = a;
        q->have_cpu = true;
    } else if (t == HSA_DEVICE_TYPE_GPU && !q->have_gpu) {
        uint32_t bdf = 0, dom = 0;
        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf);
        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom);
        if (bdf == q->bdf && dom == q->domain) {
            q->gpu = a;
            q->have_gpu = true;
        }
    }
    return HSA_STATUS_SUCCESS;
}

int dma_setup(int dev, DmaDev** out) {
    std::lock_guard<std::mutex> g(g_dma_mu);
    if (dev < 0 || dev >= 64) return fail(BGX_E_ARG, "bgx_dma: device %d", dev);
    DmaDev& d = g_dma[dev];
    if (!d.ready) {
        int bus = 0, slot = 0, dom = 0;
        HIP_TRY(hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, dev));
        HIP_TRY(hipDeviceGetAttribute(&slot, hipDeviceAttributePciDeviceId, dev));
        HIP_TRY(hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, dev));
        if (hsa_init() != HSA_STATUS_SUCCESS) return fail(BGX_E_STATE, "bgx_dma: hsa_init failed");
        AgentQuery q;
        q.bdf = ((uint32_t)bus << 8) | ((uint32_t)slot << 3);
        q.domain = (uint32_t)dom;
        hsa_iterate_agents(find_agents, &q);
        if (!q.have_gpu || !q.have_cpu) return fail(BGX_E_STATE, "bgx_dma: no HSA agent for device %d", dev);
        // the CPU agent of the GPU's own NUMA node (a multi-socket host lists one
        // CPU agent per node; the first one found may be the far socket)
        hsa_agent_t near{};
        if (hsa_agent_get_info(q.gpu, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_NEAREST_CPU, &near) == HSA_STATUS_SUCCESS &&
            near.handle != 0)
            q.cpu = near;
        uint32_t mask = 0;
        if (hsa_amd_memory_copy_engine_status(q.cpu, q.gpu, &mask) != HSA_STATUS_SUCCESS || mask == 0)
            return fail(BGX_E_STATE, "bgx_dma: no DMA engine available for device %d -> host", dev);
        d.gpu = q.gpu;
        d.cpu = q.cpu;
        d.engine = (hsa_amd_sdma_engine_id_t)(mask & (~mask + 1u));   // the lowest available engine
        d.ready = true;
    }
    *out = &d;
    return BGX_OK;
}
}  // namespace

extern "C" {

int bgx_host_register(void* h_ptr, uint64_t bytes) {
    return guarded("bgx_host_register", [&]() -> int {
        if (!h_ptr || bytes == 0) return fail(BGX_E_ARG, "bgx_host_register: bad arguments");
        HIP_TRY(hipHostRegister(h_ptr, (size_t)bytes, hipHostRegisterPortable));
        return BGX_OK;
    });
}

int bgx_host_unregister(void* h_ptr) {
    return guarded("bgx_host_unregister", [&]() -> int {
        if (!h_ptr) return fail(BGX_E_ARG, "bgx_host_unregister: null pointer");
        HIP_TRY(hipHostUnregister(h_ptr));
        return BGX_OK;
    });
}

int bgx_copy_async(void* dst, const void* src, uint64_t bytes, int kind, void* stream) {
    return guarded("bgx_copy_async", [&]() -> int {
        if (bytes == 0) return BGX_OK;
        if (!dst || !src || kind < 0 || kind > 4) return fail(BGX_E_ARG, "bgx_copy_async: bad arguments");
        const hipMemcpyKind k[5] = {hipMemcpyDefault, hipMemcpyHostToDevice, hipMemcpyDeviceToHost,
                                    hipMemcpyDeviceToDevice, hipMemcpyDeviceToDeviceNoCU};
        HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, k[kind], (hipStream_t)stream));
        return BGX_OK;
    });
}

int bgx_dma_copy_d2h(void* h_dst, const void* d_src, uint64_t bytes, int device, uint64_t* ticket) {
    return guarded("bgx_dma_copy_d2h", [&]() -> int {
        if (!h_dst || !d_src || !ticket) return fail(BGX_E_ARG, "bgx_dma_copy_d2h: null pointer");
        *ticket = 0;
        if (bytes == 0) return BGX_OK;
        DmaDev* d = nullptr;
        if (int rc = dma_setup(device, &d)) return rc;
        void* dst = nullptr;   // the device-visible address of the page-locked host range
        HIP_TRY(hipHostGetDevicePointer(&dst, h_dst, 0));
        // one engine: splitting a copy over several engines moved no more than one
        // (~53-56 GB/s device -> host for 8-32 MiB; profiles/round3/dma_split/)
        hsa_signal_t sig;
        if (hsa_signal_create(1, 0, nullptr, &sig) != HSA_STATUS_SUCCESS)
            return fail(BGX_E_STATE, "bgx_dma_copy_d2h: hsa_signal_create failed");
        const hsa_status_t st = hsa_amd_memory_async_copy_on_engine(dst, d->cpu, d_src, d->gpu, (size_t)bytes, 0,
                                                                    nullptr, sig, d->engine, true);
        if (st != HSA_STATUS_SUCCESS) {
            hsa_signal_destroy(sig);
            return fail(BGX_E_STATE, "bgx_dma_copy_d2h: hsa_amd_memory_async_copy_on_engine failed (%d)", (int)st);
        }
        *ticket = sig.handle;
        return BGX_OK;
    });
}

int bgx_dma_wait(uint64_t ticket, int timeout_ms) {
    return guarded("bgx_dma_wait", [&]() -> int {
        if (ticket == 0) return BGX_OK;
        hsa_signal_t sig;
        sig.handle = ticket;
        const uint64_t ns = timeout_ms > 0 ? (uint64_t)timeout_ms * 1000000ull : UINT64_MAX;
        // spin for the first 2 ms (a harvest's copy takes ~0.1-1 ms; a blocked
        // wait adds an interrupt's wake-up), then sleep in the wait
        const uint64_t spin_ns = ns < 2000000ull ? ns : 2000000ull;
        hsa_signal_value_t v = hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, 1, spin_ns, HSA_WAIT_STATE_ACTIVE);
        if (v >= 1 && ns > spin_ns)
            v = hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, 1, ns - spin_ns, HSA_WAIT_STATE_BLOCKED);
        // past the timeout the copy is still in flight: the ticket stays valid (a
        // later wait may see it end; its signal is destroyed then) and the caller
        // must keep both buffers alive (bgx/hostgather.py STUCK_COPIES)
        if (v >= 1) return fail(BGX_E_STATE, "bgx_dma_wait: copy not finished after %d ms", timeout_ms);
        hsa_signal_destroy(sig);
        return BGX_OK;
    });
}

int bgx_dma_copy_d2d(void* d_dst, int dst_device, const void* d_src, int src_device, uint64_t bytes,
                     uint64_t* ticket) {
    return guarded("bgx_dma_copy_d2d", [&]() -> int {
        if (!d_dst || !d_src || !ticket) return fail(BGX_E_ARG, "bgx_dma_copy_d2d: null pointer");
        *ticket = 0;
        if (bytes == 0) return BGX_OK;
        DmaDev *s = nullptr, *d = nullptr;
        if (int rc = dma_setup(src_device, &s)) return rc;
        if (int rc = dma_setup(dst_device, &d)) return rc;
        // an SDMA engine of the source GPU that serves this pair (xGMI engines for
        // a peer GPU); none listed (e.g. a copy within one GPU on some drivers):
        // the runtime's own choice
        uint32_t mask = 0;
        const bool eng = hsa_amd_memory_copy_engine_status(d->gpu, s->gpu, &mask) == HSA_STATUS_SUCCESS && mask != 0;
        hsa_signal_t sig;
        if (hsa_signal_create(1, 0, nullptr, &sig) != HSA_STATUS_SUCCESS)
            return fail(BGX_E_STATE, "bgx_dma_copy_d2d: hsa_signal_create failed");
        const hsa_status_t st =
            eng ? hsa_amd_memory_async_copy_on_engine(d_dst, d->gpu, d_src, s->gpu, (size_t)bytes, 0, nullptr, sig,
                                                      (hsa_amd_sdma_engine_id_t)(mask & (~mask + 1u)), true)
                : hsa_amd_memory_async_copy(d_dst, d->gpu, d_src, s->gpu, (size_t)bytes, 0, nullptr, sig);
        if (st != HSA_STATUS_SUCCESS) {
            hsa_signal_destroy(sig);
            return fail(BGX_E_STATE, "bgx_dma_copy_d2d: async copy failed (%d)", (int)st);
        }
        *ticket = sig.handle;
        return BGX_OK;
    });
}

int bgx_ipc_export(const void* d_ptr, uint8_t* handle64, uint64_t* offset) {
    return guarded("bgx_ipc_export", [&]() -> int {
        if (!d_ptr || !handle64 || !offset) return fail(BGX_E_ARG, "bgx_ipc_export: null pointer");
        static_assert(sizeof(hipIpcMemHandle_t) == 64, "64-byte IPC handles");
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        HIP_TRY(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_ptr));
        hipIpcMemHandle_t h;
        HIP_TRY(hipIpcGetMemHandle(&h, (void*)base));
        std::memcpy(handle64, &h, 64);
        *offset = (uint64_t)((const char*)d_ptr - (const char*)base);
        return BGX_OK;
    });
}

int bgx_ipc_open(const uint8_t* handle64, uint64_t offset, void** d_ptr) {
    return guarded("bgx_ipc_open", [&]() -> int {
        if (!handle64 || !d_ptr) return fail(BGX_E_ARG, "bgx_ipc_open: null pointer");
        hipIpcMemHandle_t h;
        std::memcpy(&h, handle64, 64);
        void* base = nullptr;
        HIP_TRY(hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess));
        *d_ptr = (char*)base + offset;
        return BGX_OK;
    });
}

int bgx_ipc_close(void* d_ptr, uint64_t offset) {
    return guarded("bgx_ipc_close", [&]() -> int {
        if (!d_ptr) return fail(BGX_E_ARG, "bgx_ipc_close: null pointer");
        HIP_TRY(hipIpcCloseMemHandle((char*)d_ptr - offset));
        return BGX_OK;
    });
}

}  // extern "C"
