// The little of ROCr (HSA) a program needs to run kernels from a code object of its own, without the
// HIP runtime: the agents and their memory pools, a GPU's identity, the code-object loader, one AQL
// kernel-dispatch packet, and a bounded wait. Nothing here knows what the kernels do.
//
// No RAII for the HSA objects, on purpose: its user (kernels/hsa_vector_add.cpp) tears down in a fixed
// order that it may skip altogether, and leaves on an error without any teardown.
#pragma once

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace amdkube {
namespace hsa {

constexpr uint64_t kWaitNs = 10ull * 1000 * 1000 * 1000;   // every GPU wait gives up after 10 s

struct Fail {
  std::string what;
  hsa_status_t st;
};

inline void check(hsa_status_t st, const char* what) {
  if (st != HSA_STATUS_SUCCESS && st != HSA_STATUS_INFO_BREAK) throw Fail{what, st};
}

inline const char* status_text(hsa_status_t st) {
  const char* msg = nullptr;
  hsa_status_string(st, &msg);
  return msg ? msg : "error";
}

// ---------------------------------------------------------------------------- agents and pools
struct Agents {
  std::vector<hsa_agent_t> gpus;
  hsa_agent_t cpu{};   // the first one
  bool have_cpu = false;
};

inline hsa_status_t on_agent(hsa_agent_t a, void* data) {
  auto* ag = static_cast<Agents*>(data);
  hsa_device_type_t t;
  check(hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t), "agent type");
  if (t == HSA_DEVICE_TYPE_GPU) ag->gpus.push_back(a);
  if (t == HSA_DEVICE_TYPE_CPU && !ag->have_cpu) {
    ag->cpu = a;
    ag->have_cpu = true;
  }
  return HSA_STATUS_SUCCESS;
}

struct Pools {   // the first pool of each kind that allows allocation
  hsa_amd_memory_pool_t device{}, kernarg{}, host{};   // GPU coarse-grained; CPU kernarg; CPU fine-grained
  bool have_device = false, have_kernarg = false, have_host = false;
};

// The GLOBAL_FLAGS of a pool in the global segment that the runtime may allocate from; 0 for any other.
inline uint32_t allocatable_global_flags(hsa_amd_memory_pool_t p) {
  hsa_amd_segment_t seg;
  uint32_t flags = 0;
  bool alloc = false;
  check(hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg), "pool segment");
  if (seg != HSA_AMD_SEGMENT_GLOBAL) return 0;
  check(hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags), "pool flags");
  check(hsa_amd_memory_pool_get_info(p, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &alloc), "pool alloc");
  return alloc ? flags : 0;
}

inline void take(hsa_amd_memory_pool_t p, bool wanted, hsa_amd_memory_pool_t* slot, bool* have) {
  if (wanted && !*have) {
    *slot = p;
    *have = true;
  }
}

inline hsa_status_t on_gpu_pool(hsa_amd_memory_pool_t p, void* data) {
  auto* pools = static_cast<Pools*>(data);
  take(p, allocatable_global_flags(p) & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED, &pools->device, &pools->have_device);
  return HSA_STATUS_SUCCESS;
}

inline hsa_status_t on_cpu_pool(hsa_amd_memory_pool_t p, void* data) {
  auto* pools = static_cast<Pools*>(data);
  const uint32_t flags = allocatable_global_flags(p);
  take(p, flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_KERNARG_INIT, &pools->kernarg, &pools->have_kernarg);
  take(p, flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_FINE_GRAINED, &pools->host, &pools->have_host);
  return HSA_STATUS_SUCCESS;
}

inline Pools find_pools(hsa_agent_t gpu, hsa_agent_t cpu) {
  Pools pools;
  check(hsa_amd_agent_iterate_memory_pools(gpu, on_gpu_pool, &pools), "gpu pools");
  check(hsa_amd_agent_iterate_memory_pools(cpu, on_cpu_pool, &pools), "cpu pools");
  if (!pools.have_device || !pools.have_kernarg || !pools.have_host) throw Fail{"memory pools missing", HSA_STATUS_ERROR};
  return pools;
}

// ---------------------------------------------------------------------------- a GPU's identity
inline hsa_status_t on_isa(hsa_isa_t isa, void* data) {
  uint32_t len = 0;
  check(hsa_isa_get_info_alt(isa, HSA_ISA_INFO_NAME_LENGTH, &len), "isa name length");
  std::string name(len, '\0');
  check(hsa_isa_get_info_alt(isa, HSA_ISA_INFO_NAME, &name[0]), "isa name");
  name = name.c_str();
  const std::string pre = "amdgcn-amd-amdhsa--";
  *static_cast<std::string*>(data) = name.rfind(pre, 0) == 0 ? name.substr(pre.size()) : name;
  return HSA_STATUS_INFO_BREAK;
}

struct GpuId {
  std::string product, arch, bus, uuid;   // product is empty where the host has no name for the device id
  uint32_t cus = 0;
};

inline GpuId identify(hsa_agent_t g) {
  GpuId id;
  char buf[128] = {0};
  if (hsa_agent_get_info(g, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_PRODUCT_NAME), buf) == HSA_STATUS_SUCCESS)
    id.product = buf;
  std::memset(buf, 0, sizeof buf);
  if (hsa_agent_get_info(g, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_UUID), buf) == HSA_STATUS_SUCCESS) id.uuid = buf;
  uint32_t bdf = 0, domain = 0;
  hsa_agent_get_info(g, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_BDFID), &bdf);
  hsa_agent_get_info(g, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DOMAIN), &domain);
  std::snprintf(buf, sizeof buf, "%04x:%02x:%02x.%x", domain, (bdf >> 8) & 0xff, (bdf >> 3) & 0x1f, bdf & 0x7);
  id.bus = buf;
  hsa_agent_get_info(g, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_COMPUTE_UNIT_COUNT), &id.cus);
  hsa_agent_iterate_isas(g, on_isa, &id.arch);
  return id;
}

// ---------------------------------------------------------------------------- code object, kernels
struct Program {   // a code object loaded for one GPU and frozen
  hsa_code_object_reader_t reader{};
  hsa_executable_t exe{};
};

inline Program load_program(hsa_agent_t gpu, const void* code_object, size_t size) {
  Program p;
  check(hsa_code_object_reader_create_from_memory(code_object, size, &p.reader), "code object reader");
  check(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr, &p.exe), "executable");
  check(hsa_executable_load_agent_code_object(p.exe, gpu, p.reader, nullptr, nullptr), "load code object (gfx950 only)");
  check(hsa_executable_freeze(p.exe, nullptr), "freeze executable");
  return p;
}

struct Kernel {
  uint64_t object = 0;
  uint32_t kasz = 0, gsz = 0, psz = 0;   // kernarg, group (LDS) and private segment sizes
};

// `name` is the descriptor's symbol: "<kernel>.kd"
inline Kernel kernel(const Program& p, hsa_agent_t gpu, const char* name) {
  hsa_executable_symbol_t sym;
  check(hsa_executable_get_symbol_by_name(p.exe, name, &gpu, &sym), name);
  Kernel k;
  check(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k.object), "kernel object");
  check(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &k.kasz), "kernarg size");
  check(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &k.gsz), "group size");
  check(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &k.psz), "private size");
  return k;
}

// ---------------------------------------------------------------------------- dispatch and wait
// One AQL kernel-dispatch packet of `groups` work-groups of `wg` work-items, with the barrier bit so
// packets on the queue run in order; system-scope fences both sides.
inline void dispatch(hsa_queue_t* q, const Kernel& k, void* kargs, uint64_t groups, uint32_t wg, hsa_signal_t completion) {
  if (groups == 0 || groups * wg > UINT32_MAX) throw Fail{"bad dispatch size", HSA_STATUS_ERROR};
  const uint64_t idx = hsa_queue_add_write_index_screlease(q, 1);
  while (idx - hsa_queue_load_read_index_scacquire(q) >= q->size) {
  }
  auto* pkt = static_cast<hsa_kernel_dispatch_packet_t*>(q->base_address) + (idx & (q->size - 1));
  std::memset(reinterpret_cast<char*>(pkt) + 4, 0, sizeof(*pkt) - 4);
  pkt->workgroup_size_x = static_cast<uint16_t>(wg);
  pkt->workgroup_size_y = pkt->workgroup_size_z = 1;
  pkt->grid_size_x = static_cast<uint32_t>(groups * wg);
  pkt->grid_size_y = pkt->grid_size_z = 1;
  pkt->kernel_object = k.object;
  pkt->kernarg_address = kargs;
  pkt->private_segment_size = k.psz;
  pkt->group_segment_size = k.gsz;
  pkt->completion_signal = completion;
  const uint16_t setup = 1u << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
  const uint16_t header = (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1u << HSA_PACKET_HEADER_BARRIER) |
                          (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                          (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
  __atomic_store_n(reinterpret_cast<uint32_t*>(pkt), static_cast<uint32_t>(header) | (static_cast<uint32_t>(setup) << 16),
                   __ATOMIC_RELEASE);
  hsa_signal_store_screlease(q->doorbell_signal, static_cast<hsa_signal_value_t>(idx));
}

inline void wait_zero(hsa_signal_t s, const char* what) {
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::nanoseconds(kWaitNs);
  while (hsa_signal_wait_scacquire(s, HSA_SIGNAL_CONDITION_LT, 1, 100 * 1000 * 1000, HSA_WAIT_STATE_BLOCKED) >= 1) {
    if (std::chrono::steady_clock::now() > deadline) throw Fail{std::string(what) + ": timed out", HSA_STATUS_ERROR};
  }
}

}  // namespace hsa
}  // namespace amdkube
