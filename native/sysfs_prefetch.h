// Prefetch of the files ROCr's hsa_init reads one by one, served back through fopen().
//
// After open("/dev/kfd") returns, hsa_init reads about nine thousand small files in sequence
// (measured on MI355X, docs/PERFORMANCE.md "Prefetching hsa_init's file reads"):
//   * the KFD topology under /sys/devices/virtual/kfd/kfd/topology, walked twice;
//   * the CPU caches under /sys/devices/system/node/node*/cpu*/cache/index*, walked twice;
//   * /proc/cpuinfo, twice.
// A GPU pod spends most of its life asleep in that open behind its predecessor's KFD release
// work, and none of the reading needs the KFD descriptor. So a helper thread started before
// hsa_init reads these files into memory during the wait (and stops when the wait ends:
// cancel()), and the executable's own fopen()
// (which ROCr's calls bind to before libc's) answers ROCr's reads from that snapshot with
// fmemopen(): libc's fscanf/fgets/fread/fclose then work on it unchanged.
//
// What is cached, and nothing else:
//   <topology>/system_properties and, under <topology>/nodes/*, gpu_id, name, properties and
//     {mem_banks,caches,io_links,p2p_links}/*/properties;
//   <cpu nodes>/node*/cpu*/cache/index*/shared_cpu_list for every CPU and, for the first CPU of
//     each list (the one the thunk describes the cache by), level, type, size,
//     coherency_line_size, ways_of_associativity, physical_line_partition, shared_cpu_map;
//   the cpuinfo file.
// generation_id (the thunk reads it before and after a walk to detect a topology change) and
// mem_banks/*/used_memory stay live, as does every name not on the list. The helper itself reads
// generation_id before and after its pass and drops the snapshot whole when the two differ.
//
// The helper enumerates with opendir/readdir and reads through the *next* fopen in lookup order
// (RTLD_NEXT), not a raw syscall: in a container the device-view preload (native/devview.c) sits
// there, and chaining through it keeps the pod's view of the host exactly what it is without
// the prefetch. An empty file, a file whose read failed (so EPERM/ENOENT stay the kernel's own
// answer) and any mode but "r" pass through untouched. A listed file asked for before the helper
// got to it is read by the asking thread itself, the same way, and kept: ROCr walks everything
// twice, so even a process whose helper had no wait to work in reads each file once, not twice.
// Every read of generation_id by the process is compared with the value the snapshot was taken
// under; a different one drops the snapshot, so the thunk's own before/after check of a walk
// keeps its meaning.
//
// Concurrency contract (checked by native/sysfs_prefetch_selftest.cpp under ThreadSanitizer):
//  * open_file() may run before main() and on any thread; until start() has published a
//    snapshot it touches nothing but two constant-initialised atomics;
//  * entries are published one at a time under the snapshot's mutex, by the helper or by a
//    reader that missed; a lookup takes the same mutex for the map probe only and never waits
//    for the helper's I/O;
//  * a published buffer is never freed or changed: snapshots live until the process exits, so a
//    FILE served from one stays valid whatever happens later (drop, a second start()).
#pragma once

#include <dirent.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

namespace amdkube {
namespace prefetch {

constexpr size_t kReadChunk = 4096;   // the helper's read buffer; larger files take more rounds

// Where the three groups of files live; an empty path leaves its group out. Tests point these
// at a fake tree.
struct Roots {
  std::string topology = "/sys/devices/virtual/kfd/kfd/topology";
  std::string cpu_nodes = "/sys/devices/system/node";
  std::string cpuinfo = "/proc/cpuinfo";
};

using fopen_fn = FILE* (*)(const char*, const char*);

struct Stats {
  uint64_t files = 0, bytes = 0;     // cached
  uint64_t hits = 0, misses = 0;     // fopen(…, "r") of a path under a root: served / passed through
  uint64_t distinct = 0;             // cached files served at least once
  double helper_ms = 0.0;
  bool dropped = false;
};

struct Entry {
  std::string path, data;
  std::atomic<bool> served{false};
  Entry(std::string p, std::string d) : path(std::move(p)), data(std::move(d)) {}
};

struct Snapshot {
  Roots roots;                                          // directories without a trailing slash
  std::string generation_path;                          // <topology>/generation_id
  std::mutex mu;                                        // guards `entries`, `index` and `generation`
  std::string generation;                               // the generation_id the snapshot is taken under
  std::deque<Entry> entries;                            // an element never moves
  std::unordered_map<std::string_view, Entry*> index;   // keyed by Entry::path
  std::atomic<bool> dropped{false};
  std::atomic<bool> cancelled{false};                   // the helper reads no further files
  std::atomic<uint64_t> bytes{0}, hits{0}, misses{0}, distinct{0}, nfiles{0};
  double helper_ms = 0.0;                               // written by the helper, read after join()
  std::function<void()> before_recheck;                 // test hook: runs between the two generation_id reads
  std::thread helper;
  Snapshot* older = nullptr;                            // earlier snapshots stay reachable (and alive)
};

inline std::atomic<fopen_fn> g_next_fopen{nullptr};
inline std::atomic<Snapshot*> g_snapshot{nullptr};
inline thread_local bool t_in_helper = false;           // true on the helper thread (an I/O trace leaves it out)

// The fopen after this executable's in symbol lookup order: a preload's if there is one, else libc's.
inline fopen_fn next_fopen() {
  fopen_fn fn = g_next_fopen.load(std::memory_order_acquire);
  if (!fn) {
    fn = reinterpret_cast<fopen_fn>(dlsym(RTLD_NEXT, "fopen"));
    g_next_fopen.store(fn, std::memory_order_release);
  }
  return fn;
}

inline bool under(const std::string& dir, const char* path) {
  const size_t n = dir.size();
  return n && std::strncmp(path, dir.c_str(), n) == 0 && path[n] == '/';
}

inline bool covered(const Snapshot& s, const char* path) {
  return under(s.roots.topology, path) || under(s.roots.cpu_nodes, path) ||
         (!s.roots.cpuinfo.empty() && s.roots.cpuinfo == path);
}

// Reads `path` whole through the next fopen. False when it cannot be opened or a read fails.
inline bool read_whole(const char* path, std::string* out) {
  FILE* f = next_fopen()(path, "r");
  if (!f) return false;
  out->clear();
  char buf[kReadChunk];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, k);
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}
inline bool read_whole(const std::string& path, std::string* out) { return read_whole(path.c_str(), out); }

// Reads `path` and publishes it; returns its entry (an earlier one if it was published
// meanwhile), or null when there is nothing to serve: unreadable or empty.
inline Entry* publish(Snapshot* s, const char* path) {
  std::string data;
  if (!read_whole(path, &data) || data.empty()) return nullptr;
  const size_t n = data.size();
  Entry* e;
  {
    std::lock_guard<std::mutex> g(s->mu);
    auto it = s->index.find(std::string_view(path));
    if (it != s->index.end()) return it->second;
    e = &s->entries.emplace_back(path, std::move(data));
    s->index.emplace(std::string_view(e->path), e);
  }
  s->nfiles.fetch_add(1, std::memory_order_relaxed);
  s->bytes.fetch_add(n, std::memory_order_relaxed);
  return e;
}

// The helper's publish: nothing more once it is cancelled.
inline const std::string* prefetch(Snapshot* s, const std::string& path) {
  if (s->cancelled.load(std::memory_order_relaxed)) return nullptr;
  Entry* e = publish(s, path.c_str());
  return e ? &e->data : nullptr;
}

inline bool one_of(const char* name, std::initializer_list<const char*> names) {
  for (const char* n : names)
    if (std::strcmp(name, n) == 0) return true;
  return false;
}

// Is `path` (under a root) one of the files on the list at the top of this file?
inline bool listed(const Snapshot& s, const char* path) {
  const char* slash = std::strrchr(path, '/');
  const char* base = slash ? slash + 1 : path;
  if (under(s.roots.topology, path)) return one_of(base, {"system_properties", "gpu_id", "name", "properties"});
  if (under(s.roots.cpu_nodes, path))
    return std::strstr(path + s.roots.cpu_nodes.size(), "/cache/index") &&
           one_of(base, {"shared_cpu_list", "level", "type", "size", "coherency_line_size", "ways_of_associativity",
                         "physical_line_partition", "shared_cpu_map"});
  return true;   // the cpuinfo file
}

// A read of <topology>/generation_id by the process: always the file's bytes of this moment,
// and a value other than the one the snapshot was taken under drops the snapshot, so a walk that
// its reader brackets with two generation reads never mixes cached and newer content unnoticed.
inline FILE* open_generation(Snapshot* s, const char* path) {
  std::string now;
  if (!read_whole(path, &now) || now.empty()) return nullptr;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->generation.empty()) s->generation = now;
  else if (s->generation != now) s->dropped.store(true, std::memory_order_release);
  Entry& e = s->entries.emplace_back(std::string(), std::move(now));   // not indexed: served once
  return fmemopen(const_cast<char*>(e.data.data()), e.data.size(), "r");
}

// The body of the executable's `extern "C" FILE* fopen(const char*, const char*)`.
inline FILE* open_file(const char* path, const char* mode) {
  Snapshot* s = g_snapshot.load(std::memory_order_acquire);
  if (s && !t_in_helper && path && mode && mode[0] == 'r' && mode[1] == '\0' && covered(*s, path)) {
    if (s->generation_path == path) {
      if (FILE* f = open_generation(s, path)) return f;
    } else if (!s->dropped.load(std::memory_order_acquire)) {
      Entry* e = nullptr;
      {
        std::lock_guard<std::mutex> g(s->mu);
        auto it = s->index.find(std::string_view(path));
        if (it != s->index.end()) e = it->second;
      }
      const bool hit = e != nullptr;
      // not there (yet): this thread reads the file, once, and keeps it for the next walk
      if (!e && listed(*s, path)) e = publish(s, path);
      if (e) {
        if (FILE* f = fmemopen(const_cast<char*>(e->data.data()), e->data.size(), "r")) {
          if (hit) {
            s->hits.fetch_add(1, std::memory_order_relaxed);
            if (!e->served.exchange(true, std::memory_order_relaxed)) s->distinct.fetch_add(1, std::memory_order_relaxed);
          } else {
            s->misses.fetch_add(1, std::memory_order_relaxed);
          }
          return f;
        }
      }
    }
    s->misses.fetch_add(1, std::memory_order_relaxed);
  }
  return next_fopen()(path, mode);
}

// Entries of a directory that start with `prefix` ("." and ".." left out), in the order ROCr
// asks for them (0, 1, … 10, 11).
inline std::vector<std::string> list_dir(const std::string& dir, const char* prefix = "") {
  std::vector<std::string> names;
  const size_t pl = std::strlen(prefix);
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d))
      if (std::strcmp(e->d_name, ".") != 0 && std::strcmp(e->d_name, "..") != 0 && std::strncmp(e->d_name, prefix, pl) == 0)
        names.emplace_back(e->d_name);
    closedir(d);
  }
  std::sort(names.begin(), names.end(), [](const std::string& a, const std::string& b) {
    return a.size() != b.size() ? a.size() < b.size() : a < b;
  });
  return names;
}

inline bool numbered(const std::string& name, size_t prefix_len) {
  return name.size() > prefix_len && name.find_first_not_of("0123456789", prefix_len) == std::string::npos;
}

inline void walk_topology(Snapshot* s) {
  const std::string& root = s->roots.topology;
  prefetch(s, root + "/system_properties");
  const std::string nodes = root + "/nodes";
  for (const std::string& node : list_dir(nodes)) {
    if (s->cancelled.load(std::memory_order_relaxed)) return;
    const std::string base = nodes + "/" + node;
    for (const char* leaf : {"gpu_id", "name", "properties"}) prefetch(s, base + "/" + leaf);
    for (const char* sub : {"mem_banks", "caches", "io_links", "p2p_links"})
      for (const std::string& e : list_dir(base + "/" + sub)) prefetch(s, base + "/" + sub + "/" + e + "/properties");
  }
}

inline void walk_cpu_caches(Snapshot* s) {
  for (const std::string& node : list_dir(s->roots.cpu_nodes, "node")) {
    if (!numbered(node, 4)) continue;
    const std::string nbase = s->roots.cpu_nodes + "/" + node;
    for (const std::string& cpu : list_dir(nbase, "cpu")) {
      if (!numbered(cpu, 3)) continue;   // cpumap, cpulist
      if (s->cancelled.load(std::memory_order_relaxed)) return;
      const std::string cbase = nbase + "/" + cpu + "/cache";
      for (const std::string& idx : list_dir(cbase, "index")) {
        const std::string ibase = cbase + "/" + idx;
        const std::string* list = prefetch(s, ibase + "/shared_cpu_list");
        // the thunk describes a cache once, by the first CPU that shares it
        if (!list || std::strtoul(list->c_str(), nullptr, 10) != std::strtoul(cpu.c_str() + 3, nullptr, 10)) continue;
        for (const char* leaf : {"level", "type", "size", "coherency_line_size", "ways_of_associativity",
                                 "physical_line_partition", "shared_cpu_map"})
          prefetch(s, ibase + "/" + leaf);
      }
    }
  }
}

inline void walk(Snapshot* s) {
  t_in_helper = true;
  const auto t0 = std::chrono::steady_clock::now();
  bool valid = true;
  if (!s->roots.topology.empty()) {
    const std::string& gen_path = s->generation_path;
    std::string gen0, gen1;
    valid = read_whole(gen_path, &gen0);
    if (valid) {
      std::lock_guard<std::mutex> g(s->mu);
      if (s->generation.empty()) s->generation = gen0;
      else valid = s->generation == gen0;
    }
    if (valid) {
      // most time saved per file read first, in case the wait ends early: every CPU-cache file is
      // asked for, while most of the topology describes GPUs this process cannot use
      if (!s->roots.cpu_nodes.empty()) walk_cpu_caches(s);
      if (!s->roots.cpuinfo.empty()) prefetch(s, s->roots.cpuinfo);
      walk_topology(s);
      if (s->before_recheck) s->before_recheck();
      // a topology that changed under the pass (or one whose generation cannot be read) is not served
      valid = read_whole(gen_path, &gen1) && gen0 == gen1;
    }
  } else {
    if (!s->roots.cpu_nodes.empty()) walk_cpu_caches(s);
    if (!s->roots.cpuinfo.empty()) prefetch(s, s->roots.cpuinfo);
  }
  if (!valid) s->dropped.store(true, std::memory_order_release);
  s->helper_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// AMDKUBE_VADD_PREFETCH=0 turns the prefetch off (pure pass-through).
inline bool enabled_by_env() {
  const char* v = std::getenv("AMDKUBE_VADD_PREFETCH");
  return !(v && std::strcmp(v, "0") == 0);
}

// Publishes an empty snapshot and starts the helper that fills it. Call join() before the
// process exits. A second start() leaves the earlier snapshot alive and unserved.
inline void start(Roots roots = Roots(), std::function<void()> before_recheck = {}) {
  for (std::string* dir : {&roots.topology, &roots.cpu_nodes})
    while (dir->size() > 1 && dir->back() == '/') dir->pop_back();
  next_fopen();
  auto* s = new Snapshot;
  s->roots = std::move(roots);
  if (!s->roots.topology.empty()) s->generation_path = s->roots.topology + "/generation_id";
  s->before_recheck = std::move(before_recheck);
  s->older = g_snapshot.load(std::memory_order_acquire);
  g_snapshot.store(s, std::memory_order_release);
  s->helper = std::thread(walk, s);
}

// Waits for the helper to finish its pass. Idempotent; a no-op when start() never ran.
inline void join() {
  Snapshot* s = g_snapshot.load(std::memory_order_acquire);
  if (s && s->helper.joinable()) s->helper.join();
}

// The helper reads no further files; what it has published stays served. For the caller whose
// wait is over: from here on the helper would only compete with the reader it works for
// (measured: two threads reading sysfs side by side are slower than one reading it all).
inline void cancel() {
  if (Snapshot* s = g_snapshot.load(std::memory_order_acquire)) s->cancelled.store(true, std::memory_order_relaxed);
}

// Back to pure pass-through (the snapshots stay alive for the FILEs already served).
inline void stop() {
  join();
  if (Snapshot* s = g_snapshot.load(std::memory_order_acquire)) s->dropped.store(true, std::memory_order_release);
}

// Counters of the current snapshot; helper_ms is valid after join().
inline Stats stats() {
  Stats st;
  if (Snapshot* s = g_snapshot.load(std::memory_order_acquire)) {
    st.files = s->nfiles.load(std::memory_order_relaxed);
    st.bytes = s->bytes.load(std::memory_order_relaxed);
    st.hits = s->hits.load(std::memory_order_relaxed);
    st.misses = s->misses.load(std::memory_order_relaxed);
    st.distinct = s->distinct.load(std::memory_order_relaxed);
    st.dropped = s->dropped.load(std::memory_order_acquire);
    st.helper_ms = s->helper.joinable() ? 0.0 : s->helper_ms;
  }
  return st;
}

}  // namespace prefetch
}  // namespace amdkube
