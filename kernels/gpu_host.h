// HIP host plumbing of the validation workloads: error checking, device identity, and the owners of
// device buffers and events, so that a thrown AK_HIP frees what a runner had allocated (the extension
// _hipops lives as long as its process). The only place that allocates or frees device memory and events.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace amdkube {

#define AK_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      throw std::runtime_error(std::string(#call) + ": " + hipGetErrorString(e_));         \
  } while (0)

struct DevInfo {
  std::string name, arch, pci_bus_id, uuid;
  size_t total_mem = 0;
  int cu_count = 0;
  int device = 0;
};

inline std::string uuid_string(const hipUUID& u) {
  // HIP reports the 16 raw bytes; AMD exposes them as the ASCII unique id, print both forms
  bool printable = true;
  for (int i = 0; i < 16; ++i) {
    unsigned char c = static_cast<unsigned char>(u.bytes[i]);
    if (c != 0 && (c < 0x20 || c > 0x7e)) printable = false;
  }
  if (printable) {
    std::string s(u.bytes, u.bytes + 16);
    s = s.c_str();
    if (!s.empty()) return "GPU-" + s;
  }
  char buf[40];
  for (int i = 0; i < 16; ++i) std::snprintf(buf + 2 * i, 3, "%02x", static_cast<unsigned char>(u.bytes[i]));
  return std::string("GPU-") + buf;
}

inline DevInfo dev_info(int dev) {
  DevInfo d;
  d.device = dev;
  hipDeviceProp_t p;
  AK_HIP(hipGetDeviceProperties(&p, dev));
  d.name = p.name;
  d.arch = p.gcnArchName;
  d.total_mem = p.totalGlobalMem;
  d.cu_count = p.multiProcessorCount;
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), dev) == hipSuccess) d.pci_bus_id = bus;
  hipUUID u;
  if (hipDeviceGetUuid(&u, dev) == hipSuccess) d.uuid = uuid_string(u);
  return d;
}

// A device allocation of `bytes` bytes. The constructors that do more than allocate delegate to the
// first, so the buffer is freed when their own step throws.
struct DevBuf {
  enum Zeroed { zeroed };
  void* p = nullptr;
  size_t bytes;
  explicit DevBuf(size_t n) : bytes(n) { AK_HIP(hipMalloc(&p, n ? n : 16)); }
  DevBuf(size_t n, Zeroed) : DevBuf(n) { zero(); }
  template <class T>
  explicit DevBuf(const std::vector<T>& v) : DevBuf(v.size() * sizeof(T)) {
    if (bytes) AK_HIP(hipMemcpy(p, v.data(), bytes, hipMemcpyHostToDevice));
  }
  ~DevBuf() { (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  void zero() { fill(0); }
  // every byte; 0xff makes each float a NaN and each word all ones: a tripwire for an element nobody wrote
  void fill(int byte) {
    if (bytes) AK_HIP(hipMemset(p, byte, bytes));
  }
  // the first n elements (all of them by default), after everything queued on the device
  template <class T>
  std::vector<T> download(size_t n = ~size_t(0)) const {
    std::vector<T> v(n < bytes / sizeof(T) ? n : bytes / sizeof(T));
    if (!v.empty()) AK_HIP(hipMemcpy(v.data(), p, v.size() * sizeof(T), hipMemcpyDeviceToHost));
    return v;
  }
};

struct GpuEvent {
  hipEvent_t e = nullptr;
  GpuEvent() { AK_HIP(hipEventCreate(&e)); }
  ~GpuEvent() { (void)hipEventDestroy(e); }
  GpuEvent(const GpuEvent&) = delete;
  GpuEvent& operator=(const GpuEvent&) = delete;
};

struct GpuTimer {
  GpuEvent t0, t1;
  // milliseconds on the device between the start of launch() and the end of what it queued
  template <class Launch>
  double time(Launch&& launch) {
    AK_HIP(hipEventRecord(t0.e));
    launch();
    AK_HIP(hipEventRecord(t1.e));
    AK_HIP(hipEventSynchronize(t1.e));
    float ms = 0;
    AK_HIP(hipEventElapsedTime(&ms, t0.e, t1.e));
    return static_cast<double>(ms);
  }
};

// the first records of a check: the device counts every request in nrec and keeps `recs.bytes / sizeof(Rec)`
template <class Rec>
inline std::vector<Rec> fetch_records(const DevBuf& nrec, const DevBuf& recs) {
  return recs.download<Rec>(nrec.download<unsigned>()[0]);
}

}  // namespace amdkube
