// AMDKUBE_VADD_TRACE: the phase times of hsa-vector-add, and where hsa_init's file I/O goes.
//
// The executable defines fopen / fclose / open / opendir itself, as one-line calls of the functions
// below, so ROCr's and libdrm's calls find them before libc's. Inside the window (the caller opens it
// around hsa_init, with tracing on) each call is counted and timed into the group its path belongs
// to, a stdio file from fopen to fclose (sysfs formats its answer in the read, not the open). The
// prefetch helper's own reads (native/sysfs_prefetch.h, t_in_helper) are left out. Outside the window
// the four functions pass straight through; fopen always goes through the prefetch's open_file.
//
// These run before main() and on ROCr's threads: everything here is constant-initialised and errno is
// what libc left on every path. The span table holds 64 stdio files open at
// once (ROCr holds one or two); a 65th is counted but its time is not.
// Checked by native/io_trace_selftest.cpp, also under ASan/UBSan and ThreadSanitizer.
#pragma once

#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <pthread.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sysfs_prefetch.h"

namespace amdkube {
namespace iotrace {

enum Group { kTopology, kProc, kSysSystem, kDrmPci, kDev, kOther, kGroups };
inline const char* const kGroupName[kGroups] = {"kfd-topology", "/proc", "/sys/devices/system", "drm+pci", "/dev", "other"};

struct Acc {
  std::atomic<uint64_t> fopens{0}, fopen_ns{0}, opens{0}, open_ns{0}, opendirs{0}, opendir_ns{0};   // constant-initialised
};
inline Acc g_acc[kGroups];
inline std::atomic<bool> g_window{false};   // true while the caller is inside hsa_init with tracing on
inline std::atomic<bool> g_paths{false};    // AMDKUBE_VADD_TRACE=paths: also list every path opened
inline bool tracing() { return g_window.load(std::memory_order_acquire) && !prefetch::t_in_helper; }
inline std::atomic<int64_t> g_kfd_enter_ns{0}, g_kfd_return_ns{0};
struct Span {
  FILE* f;
  int64_t t0;
  int group;
};
inline Span g_spans[64];                    // stdio files open right now
inline pthread_mutex_t g_spans_mu = PTHREAD_MUTEX_INITIALIZER;

inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The window: window_begin() just before the call to trace, window_end() just after; each returns its time.
inline int64_t window_begin(bool on, bool paths) {
  const int64_t t = now_ns();
  g_paths.store(on && paths, std::memory_order_relaxed);
  g_window.store(on, std::memory_order_release);
  return t;
}
inline int64_t window_end() {
  g_window.store(false, std::memory_order_release);
  return now_ns();
}

inline bool starts(const char* path, const char* prefix) { return std::strncmp(path, prefix, std::strlen(prefix)) == 0; }

inline int group_of(const char* path) {
  if (!path) return kOther;
  if (starts(path, "/sys/devices/virtual/kfd/kfd/topology")) return kTopology;
  if (starts(path, "/proc/")) return kProc;
  if (starts(path, "/sys/devices/system/")) return kSysSystem;
  if (starts(path, "/sys/class/drm") || starts(path, "/sys/bus/pci") || starts(path, "/sys/devices/pci") ||
      starts(path, "/sys/dev/char"))
    return kDrmPci;
  if (starts(path, "/dev/")) return kDev;
  return kOther;
}

inline void span_begin(FILE* f, int group, int64_t t0) {
  pthread_mutex_lock(&g_spans_mu);
  for (Span& s : g_spans)
    if (!s.f) {
      s = Span{f, t0, group};
      break;
    }
  pthread_mutex_unlock(&g_spans_mu);
}

// the span of `f`, if it was opened inside the window: closes it and returns its group, else -1
inline int span_end(FILE* f, int64_t* t0) {
  int group = -1;
  pthread_mutex_lock(&g_spans_mu);
  for (Span& s : g_spans)
    if (s.f == f) {
      group = s.group;
      *t0 = s.t0;
      s.f = nullptr;
      break;
    }
  pthread_mutex_unlock(&g_spans_mu);
  return group;
}

// The `name` after this executable's in symbol lookup order: a preload's if there is one, else libc's.
template <typename Fn>
Fn next(std::atomic<Fn>& slot, const char* name) {
  Fn fn = slot.load(std::memory_order_acquire);
  if (!fn) {
    fn = reinterpret_cast<Fn>(dlsym(RTLD_NEXT, name));
    slot.store(fn, std::memory_order_release);
  }
  return fn;
}

using fclose_fn = int (*)(FILE*);
using open_fn = int (*)(const char*, int, ...);
using opendir_fn = DIR* (*)(const char*);
inline std::atomic<fclose_fn> g_fclose{nullptr};
inline std::atomic<open_fn> g_open{nullptr};
inline std::atomic<opendir_fn> g_opendir{nullptr};

// ---------------------------------------------------------------------------- the four overrides' bodies
inline FILE* traced_fopen(const char* path, const char* mode) {
  if (!tracing()) return prefetch::open_file(path, mode);
  const int64_t t0 = now_ns();
  FILE* f = prefetch::open_file(path, mode);
  const int saved = errno;
  const int g = group_of(path);
  if (g_paths.load(std::memory_order_relaxed)) std::fprintf(stderr, "[path] fopen %s %s\n", path ? path : "(null)", f ? "ok" : std::strerror(saved));
  g_acc[g].fopens.fetch_add(1, std::memory_order_relaxed);
  if (f) span_begin(f, g, t0);
  else g_acc[g].fopen_ns.fetch_add(now_ns() - t0, std::memory_order_relaxed);
  errno = saved;
  return f;
}

inline int traced_fclose(FILE* f) {
  const int rc = next(g_fclose, "fclose")(f);
  if (tracing()) {
    const int saved = errno;
    int64_t t0 = 0;
    const int g = span_end(f, &t0);
    if (g >= 0) g_acc[g].fopen_ns.fetch_add(now_ns() - t0, std::memory_order_relaxed);
    errno = saved;
  }
  return rc;
}

// `ap` holds what followed `flags` in the caller's open(); `kfd_opened` runs once an open of /dev/kfd
// has returned, traced or not (for hsa-vector-add the wait its prefetch helper works in is over).
inline int traced_open(const char* path, int flags, va_list ap, void (*kfd_opened)()) {
  mode_t m = 0;
  if ((flags & O_CREAT) || (flags & O_TMPFILE) == O_TMPFILE) m = static_cast<mode_t>(va_arg(ap, int));
  const open_fn real = next(g_open, "open");
  const bool kfd = path && !std::strcmp(path, "/dev/kfd");
  if (!tracing() && !kfd) return real(path, flags, m);
  const int64_t t0 = now_ns();
  const int fd = real(path, flags, m);
  const int saved = errno;
  const int64_t t1 = now_ns();
  if (kfd && kfd_opened) kfd_opened();
  if (tracing()) {
    const int g = group_of(path);
    g_acc[g].opens.fetch_add(1, std::memory_order_relaxed);
    g_acc[g].open_ns.fetch_add(t1 - t0, std::memory_order_relaxed);
    if (kfd && !g_kfd_enter_ns.load()) {
      g_kfd_enter_ns.store(t0);
      g_kfd_return_ns.store(t1);
    }
  }
  errno = saved;
  return fd;
}

inline DIR* traced_opendir(const char* path) {
  const opendir_fn real = next(g_opendir, "opendir");
  if (!tracing()) return real(path);
  const int64_t t0 = now_ns();
  DIR* d = real(path);
  const int saved = errno;
  const int g = group_of(path);
  if (g_paths.load(std::memory_order_relaxed)) std::fprintf(stderr, "[path] opendir %s\n", path ? path : "(null)");
  g_acc[g].opendirs.fetch_add(1, std::memory_order_relaxed);
  g_acc[g].opendir_ns.fetch_add(now_ns() - t0, std::memory_order_relaxed);
  errno = saved;
  return d;
}

// ---------------------------------------------------------------------------- the [trace] lines
inline void print_phase(FILE* out, const char* phase, double ms) { std::fprintf(out, "[trace] %-14s %8.3f ms\n", phase, ms); }

// After the window: the traced call split at the /dev/kfd open (if there was one), then one line per group.
inline void report(FILE* out, int64_t begin_ns, int64_t end_ns) {
  const int64_t enter = g_kfd_enter_ns.load(), ret = g_kfd_return_ns.load();
  if (enter && ret) {
    print_phase(out, "init:pre-open", (enter - begin_ns) / 1e6);
    print_phase(out, "init:kfd-wait", (ret - enter) / 1e6);
    print_phase(out, "init:post-wait", (end_ns - ret) / 1e6);
  }
  for (int g = 0; g < kGroups; ++g) {
    const Acc& a = g_acc[g];
    std::fprintf(out, "[trace] io %-19s fopen=%llu fopen_ms=%.3f open=%llu open_ms=%.3f opendir=%llu opendir_ms=%.3f\n",
                 kGroupName[g], static_cast<unsigned long long>(a.fopens.load()), a.fopen_ns.load() / 1e6,
                 static_cast<unsigned long long>(a.opens.load()), a.open_ns.load() / 1e6,
                 static_cast<unsigned long long>(a.opendirs.load()), a.opendir_ns.load() / 1e6);
  }
}

struct Phases {   // per-phase wall times on stderr, when `on`
  bool on;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(const char* phase) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    print_phase(stderr, phase, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

}  // namespace iotrace
}  // namespace amdkube
