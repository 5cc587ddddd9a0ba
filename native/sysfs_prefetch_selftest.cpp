// Self-test for native/sysfs_prefetch.h on a fake KFD topology tree in a temp directory, through
// this program's own interposed fopen (the way kernels/hsa_vector_add.cpp uses the header).
// Built plain, with -fsanitize=address,undefined and with -fsanitize=thread by native/build.py;
// run by tests/test_sysfs_prefetch.py. Prints "OK …" and exits 0, or "FAIL: …" and exits 1.
//
//   sysfs-prefetch-selftest [--no-prefetch]     (AMDKUBE_VADD_PREFETCH=0 does the same)
// With the switch off the helper never starts: every read must still be right, with zero hits.
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "sysfs_prefetch.h"

namespace pf = amdkube::prefetch;

extern "C" FILE* fopen(const char* path, const char* mode) { return pf::open_file(path, mode); }

namespace {

int g_failed = 0;
#define EXPECT(cond, ...)                      \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++g_failed;                              \
    }                                          \
  } while (0)

void mkdirs(const std::string& path) {
  for (size_t i = 1; i <= path.size(); ++i)
    if (i == path.size() || path[i] == '/') mkdir(path.substr(0, i).c_str(), 0755);
}

// written and read back with libc's own fopen, never the interposed one
void write_direct(const std::string& path, const std::string& data) {
  mkdirs(path.substr(0, path.rfind('/')));
  FILE* f = pf::next_fopen()(path.c_str(), "w");
  if (!f || std::fwrite(data.data(), 1, data.size(), f) != data.size()) {
    std::printf("FAIL: cannot write %s\n", path.c_str());
    std::exit(1);
  }
  std::fclose(f);
}

bool slurp(FILE* f, std::string* out) {
  out->clear();
  char buf[257];   // not a divisor of the helper's chunk
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, k);
  return !std::ferror(f);
}

// through the interposed fopen
bool read_hooked(const std::string& path, std::string* out) {
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return false;
  const bool ok = slurp(f, out);
  std::fclose(f);
  return ok;
}

std::string properties(int node, int lines) {
  std::string s;
  for (int i = 0; i < lines; ++i) s += "prop_" + std::to_string(i) + " " + std::to_string(1000003ull * node + 7919ull * i) + "\n";
  return s;
}

struct Tree {
  std::string root;                            // the fake KFD topology
  pf::Roots roots;
  std::map<std::string, std::string> listed;   // path → content of every file the helper should cache
  std::map<std::string, std::string> fillable; // on the list, but not read ahead: kept once somebody reads them
  std::map<std::string, std::string> unlisted; // files beside them that must stay live
  std::string empty, big, one_byte;
};

Tree make_tree(const std::string& top) {
  Tree t;
  t.root = top + "/topology";
  auto put = [&](const std::string& rel, const std::string& data, bool listed) {
    write_direct(t.root + "/" + rel, data);
    if (listed && !data.empty()) t.listed[t.root + "/" + rel] = data;
  };
  put("generation_id", "2\n", false);
  put("system_properties", "platform_oem 35498446626881\nplatform_id 35322352389441\nplatform_rev 2\n", true);
  for (int node = 0; node < 11; ++node) {   // 11: node "10" sorts after "9" only numerically
    const std::string base = "nodes/" + std::to_string(node);
    put(base + "/gpu_id", node < 2 ? "0\n" : std::to_string(40000 + node) + "\n", true);
    put(base + "/name", node == 2 ? "x" : "ip discovery\n", true);
    put(base + "/properties", properties(node, node == 1 ? 700 : 40), true);   // node 1: > 2 read chunks
    for (int c = 0; c < (node < 2 ? 0 : 6); ++c)
      put(base + "/caches/" + std::to_string(c) + "/properties", node == 3 && c == 0 ? "" : properties(100 + c, 8), true);
    for (int l = 0; l < 2; ++l) put(base + "/io_links/" + std::to_string(l) + "/properties", properties(200 + l, 10), true);
    put(base + "/p2p_links/0/properties", properties(300, 10), true);
    put(base + "/mem_banks/0/properties", properties(400, 6), true);
    put(base + "/mem_banks/0/used_memory", "1048576\n", false);
    put(base + "/caches_note", "not on the list\n", false);
  }
  t.empty = t.root + "/nodes/3/caches/0/properties";
  t.big = t.root + "/nodes/1/properties";
  t.one_byte = t.root + "/nodes/2/name";
  // CPU caches: two NUMA nodes, CPUs in pairs that share L1/L2 (index0, index1), one L3 (index2) per node
  t.roots.topology = t.root;
  t.roots.cpu_nodes = top + "/system/node";
  t.roots.cpuinfo = top + "/cpuinfo";
  for (int cpu = 0; cpu < 12; ++cpu) {
    const int node = cpu / 6;
    for (int idx = 0; idx < 3; ++idx) {
      const int first = idx < 2 ? cpu & ~1 : node * 6, last = idx < 2 ? first + 1 : first + 5;
      const std::string base = t.roots.cpu_nodes + "/node" + std::to_string(node) + "/cpu" + std::to_string(cpu) + "/cache/index" +
                               std::to_string(idx) + "/";
      auto cput = [&](const std::string& leaf, const std::string& data, bool listed) {
        write_direct(base + leaf, data);
        (listed ? t.listed : std::strcmp(leaf.c_str(), "number_of_sets") ? t.fillable : t.unlisted)[base + leaf] = data;
      };
      cput("shared_cpu_list", std::to_string(first) + "-" + std::to_string(last) + "\n", true);
      const bool described = cpu == first;     // the other CPUs' copies are never asked for: not cached
      cput("level", std::to_string(idx + 1) + "\n", described);
      cput("type", idx == 0 ? "Data\n" : "Unified\n", described);
      cput("size", idx < 2 ? "48K\n" : "32768K\n", described);
      cput("coherency_line_size", "64\n", described);
      cput("ways_of_associativity", "12\n", described);
      cput("physical_line_partition", "1\n", described);
      cput("shared_cpu_map", "00000000,0000003f\n", described);
      cput("number_of_sets", "64\n", false);
    }
  }
  for (int node = 0; node < 2; ++node) {
    const std::string nbase = t.roots.cpu_nodes + "/node" + std::to_string(node) + "/";
    for (const char* leaf : {"cpumap", "cpulist", "meminfo"}) {
      write_direct(nbase + leaf, "0-5\n");
      t.unlisted[nbase + leaf] = "0-5\n";
    }
  }
  write_direct(t.roots.cpu_nodes + "/possible", "0-1\n");
  t.unlisted[t.roots.cpu_nodes + "/possible"] = "0-1\n";
  {
    std::string info;
    for (int cpu = 0; cpu < 12; ++cpu)
      info += "processor\t: " + std::to_string(cpu) + "\nvendor_id\t: AuthenticAMD\nmodel name\t: AMD EPYC\napicid\t\t: " +
              std::to_string(2 * cpu) + "\n\n";
    write_direct(t.roots.cpuinfo, info);
    t.listed[t.roots.cpuinfo] = info;
    write_direct(t.roots.cpuinfo + "2", "not cpuinfo\n");
    t.unlisted[t.roots.cpuinfo + "2"] = "not cpuinfo\n";
  }
  // the same basenames outside the root
  write_direct(top + "/elsewhere/nodes/0/properties", "outside 1\n");
  write_direct(top + "/topology2/nodes/0/properties", "outside 2\n");   // shares the root as a string prefix
  return t;
}

// every listed file reads back byte-identical; returns how many were read
size_t check_all(const Tree& t) {
  size_t n = 0;
  for (const auto& kv : t.listed) {
    std::string got;
    EXPECT(read_hooked(kv.first, &got), "cannot read %s", kv.first.c_str());
    EXPECT(got == kv.second, "%s: %zu bytes read, %zu expected", kv.first.c_str(), got.size(), kv.second.size());
    ++n;
  }
  return n;
}

// the same call on the interposed fopen and on libc's: same success, same errno, same bytes
void same_as_direct(const std::string& path, const char* mode) {
  errno = 0;
  FILE* a = fopen(path.c_str(), mode);
  const int ea = errno;
  errno = 0;
  FILE* b = pf::next_fopen()(path.c_str(), mode);
  const int eb = errno;
  EXPECT(!a == !b, "%s mode %s: hooked %p, direct %p", path.c_str(), mode, static_cast<void*>(a), static_cast<void*>(b));
  if (!a || !b) EXPECT(ea == eb, "%s mode %s: errno %d, direct %d", path.c_str(), mode, ea, eb);
  if (a && b && mode[0] == 'r') {
    std::string da, db;
    errno = 0;
    const bool oka = slurp(a, &da);
    const int ra = errno;
    errno = 0;
    const bool okb = slurp(b, &db);
    const int rb = errno;
    EXPECT(oka == okb && da == db, "%s mode %s: reads differ", path.c_str(), mode);
    if (!oka) EXPECT(ra == rb, "%s mode %s: read errno %d, direct %d", path.c_str(), mode, ra, rb);
  }
  if (a) std::fclose(a);
  if (b) std::fclose(b);
}

void run_off(const Tree& t) {
  check_all(t);
  same_as_direct(t.empty, "r");
  same_as_direct(t.root + "/nodes/0/absent", "r");
  const pf::Stats st = pf::stats();
  EXPECT(st.hits == 0 && st.files == 0, "switched off: %llu hits, %llu files", static_cast<unsigned long long>(st.hits),
         static_cast<unsigned long long>(st.files));
}

void run_on(const Tree& t, const std::string& top) {
  // 1. readers racing the helper: four threads open, read and close across the tree while it publishes
  pf::Roots slashed = t.roots;
  slashed.topology += "/";
  slashed.cpu_nodes += "//";
  pf::start(slashed);
  std::atomic<int> bad{0};
  std::vector<std::thread> readers;
  for (int r = 0; r < 4; ++r)
    readers.emplace_back([&t, &bad, r] {
      for (int round = 0; round < 6; ++round) {
        size_t i = 0;
        for (const auto& kv : t.listed) {
          if ((i++ + r) % 2) continue;
          std::string got;
          if (!read_hooked(kv.first, &got) || got != kv.second) ++bad;
        }
      }
    });
  for (auto& th : readers) th.join();
  pf::join();
  pf::join();   // idempotent
  EXPECT(bad == 0, "%d wrong reads while the helper was publishing", bad.load());
  pf::Stats st = pf::stats();
  EXPECT(!st.dropped, "snapshot dropped without a generation change");
  EXPECT(st.files == t.listed.size(), "%llu files cached, %zu listed", static_cast<unsigned long long>(st.files), t.listed.size());
  size_t bytes = 0;
  for (const auto& kv : t.listed) bytes += kv.second.size();
  EXPECT(st.bytes == bytes, "%llu bytes cached, %zu listed", static_cast<unsigned long long>(st.bytes), bytes);
  EXPECT(t.listed.at(t.big).size() > 2 * pf::kReadChunk, "big file too small for the test");

  // 2. every listed file, from the snapshot: one hit each, and again after fclose (ROCr's second walk)
  const uint64_t h0 = pf::stats().hits;
  const size_t n = check_all(t);
  EXPECT(pf::stats().hits == h0 + n, "first pass: %llu hits for %zu files", static_cast<unsigned long long>(pf::stats().hits - h0), n);
  check_all(t);
  EXPECT(pf::stats().hits == h0 + 2 * n, "second pass not served from the snapshot");
  EXPECT(pf::stats().distinct == n, "%llu distinct files served, %zu listed", static_cast<unsigned long long>(pf::stats().distinct), n);
  std::string got;
  EXPECT(read_hooked(t.one_byte, &got) && got == "x", "one-byte file");

  // 3. the real format, parsed with fscanf the way the thunk does
  {
    FILE* f = fopen(t.big.c_str(), "r");
    EXPECT(f != nullptr, "open %s", t.big.c_str());
    char name[256];
    unsigned long long value = 0;
    int lines = 0;
    bool right = true;
    while (f && std::fscanf(f, "%255s %llu\n", name, &value) == 2) {
      right = right && name == "prop_" + std::to_string(lines) && value == 1000003ull + 7919ull * lines;
      ++lines;
    }
    EXPECT(lines == 700 && right, "fscanf parsed %d lines (right=%d)", lines, right);
    if (f) std::fclose(f);
    // fgets + fread on one stream
    f = fopen((t.root + "/system_properties").c_str(), "r");
    char line[128];
    EXPECT(f && std::fgets(line, sizeof line, f) && !std::strcmp(line, "platform_oem 35498446626881\n"), "fgets");
    if (f) {
      const size_t k = std::fread(line, 1, sizeof line, f);
      EXPECT(k == std::strlen("platform_id 35322352389441\nplatform_rev 2\n") && std::feof(f), "fread after fgets: %zu", k);
      std::fclose(f);
    }
  }

  // 4. what passes through, with the kernel's own answer
  uint64_t hits = pf::stats().hits;
  same_as_direct(t.empty, "r");                               // an empty file is never cached
  same_as_direct(t.root + "/nodes/0/absent", "r");            // ENOENT
  same_as_direct(t.root + "/nodes/99/properties", "r");       // ENOENT, a listed name
  same_as_direct(t.root + "/nodes/0/caches", "r");            // a directory: the read answers EISDIR
  same_as_direct(t.root + "/nodes/0/properties/x", "r");      // ENOTDIR
  same_as_direct(t.root + "/nodes", "w");                     // EISDIR
  same_as_direct(t.root + "/nodes/0/caches_note", "r");       // not on the list
  EXPECT(read_hooked(top + "/elsewhere/nodes/0/properties", &got) && got == "outside 1\n", "path outside the root");
  EXPECT(read_hooked(top + "/topology2/nodes/0/properties", &got) && got == "outside 2\n", "sibling of the root");
  for (const auto& kv : t.unlisted) {                         // other CPUs' copies, names not on the list
    EXPECT(read_hooked(kv.first, &got) && got == kv.second, "unlisted %s", kv.first.c_str());
    same_as_direct(kv.first, "r");
  }
  EXPECT(pf::stats().hits == hits, "a pass-through case was served from the snapshot");
  // a listed file the helper did not read ahead: the first reader reads it through, the next is served
  for (const auto& kv : t.fillable) EXPECT(read_hooked(kv.first, &got) && got == kv.second, "first read of %s", kv.first.c_str());
  EXPECT(pf::stats().hits == hits, "a file nobody had read was served from the snapshot");
  for (const auto& kv : t.fillable) EXPECT(read_hooked(kv.first, &got) && got == kv.second, "second read of %s", kv.first.c_str());
  EXPECT(pf::stats().hits == hits + t.fillable.size(), "read-through files were not kept");
  hits = pf::stats().hits;
  // "w" and "r+" reach the real file even when it is cached
  const std::string victim = t.root + "/nodes/0/name";
  FILE* f = fopen(victim.c_str(), "w");
  EXPECT(f && std::fputs("rewritten\n", f) >= 0, "mode w");
  if (f) std::fclose(f);
  f = fopen(victim.c_str(), "r+");
  char now[64] = {0};
  EXPECT(f && std::fgets(now, sizeof now, f) && !std::strcmp(now, "rewritten\n"), "mode r+ reads the real file");
  if (f) {
    std::fseek(f, 0, SEEK_SET);
    std::fputs("R", f);
    std::fclose(f);
  }
  FILE* d = pf::next_fopen()(victim.c_str(), "r");
  EXPECT(d && slurp(d, &got) && got == "Rewritten\n", "writes through w and r+ did not reach the file: '%s'", got.c_str());
  if (d) std::fclose(d);
  EXPECT(pf::stats().hits == hits, "mode w or r+ was served from the snapshot");
  write_direct(victim, t.listed.at(victim));

  // 5. generation_id and used_memory are live; a reader that sees a new generation gets no cached file after it
  write_direct(t.root + "/nodes/4/mem_banks/0/used_memory", "2097152\n");
  EXPECT(read_hooked(t.root + "/nodes/4/mem_banks/0/used_memory", &got) && got == "2097152\n", "used_memory is not live");
  EXPECT(read_hooked(t.root + "/generation_id", &got) && got == "2\n" && !pf::stats().dropped, "generation_id unchanged");
  EXPECT(read_hooked(t.big, &got) && pf::stats().hits == hits + 1, "served under the unchanged generation");
  write_direct(t.root + "/generation_id", "3\n");
  write_direct(t.big, "changed 1\n");
  EXPECT(read_hooked(t.root + "/generation_id", &got) && got == "3\n", "generation_id is not live: '%s'", got.c_str());
  EXPECT(pf::stats().dropped, "a changed generation_id did not drop the snapshot");
  EXPECT(read_hooked(t.big, &got) && got == "changed 1\n", "stale file served after a generation change");
  EXPECT(pf::stats().hits == hits + 1, "a live file was served from the snapshot");
  write_direct(t.big, t.listed.at(t.big));
  pf::start(t.roots);
  pf::join();

  // 6. a FILE served earlier outlives a later snapshot
  FILE* held = fopen(t.big.c_str(), "r");
  EXPECT(held != nullptr, "open for hold");

  // 7. a generation_id that changes during the helper's pass drops the snapshot whole
  const std::string gen = t.root + "/generation_id";
  pf::start(t.roots, [gen] { write_direct(gen, "4\n"); });
  pf::join();
  st = pf::stats();
  EXPECT(st.dropped && st.files == t.listed.size(), "changed generation: dropped=%d files=%llu", st.dropped,
         static_cast<unsigned long long>(st.files));
  check_all(t);
  EXPECT(pf::stats().hits == 0, "a dropped snapshot served %llu files", static_cast<unsigned long long>(pf::stats().hits));
  if (held) {
    EXPECT(slurp(held, &got) && got == t.listed.at(t.big), "held FILE after a second start");
    std::fclose(held);
  }

  // 8. a tree without generation_id cannot be validated: nothing is served
  unlink(gen.c_str());
  pf::start(t.roots);
  pf::join();
  check_all(t);
  EXPECT(pf::stats().dropped && pf::stats().hits == 0, "served without a readable generation_id");

  // 9. a cancelled helper stops early; what it published is served, the rest read live
  write_direct(gen, "5\n");
  pf::start(t.roots);
  pf::cancel();
  pf::join();
  st = pf::stats();
  EXPECT(!st.dropped && st.files <= t.listed.size(), "cancelled: dropped=%d files=%llu", st.dropped,
         static_cast<unsigned long long>(st.files));
  check_all(t);
  EXPECT(pf::stats().hits == st.files && pf::stats().distinct == st.files, "cancelled: %llu hits for %llu cached files",
         static_cast<unsigned long long>(pf::stats().hits), static_cast<unsigned long long>(st.files));
  pf::start(t.roots, [] { pf::cancel(); });   // cancelled at the very end: everything is there and valid
  pf::join();
  EXPECT(!pf::stats().dropped && pf::stats().files == t.listed.size(), "cancel after the pass lost files");

  // 10. a fresh snapshot serves again; stop() ends it
  write_direct(gen, "5\n");
  pf::start(t.roots);
  pf::join();
  hits = pf::stats().hits;
  check_all(t);
  EXPECT(pf::stats().hits == hits + t.listed.size() && !pf::stats().dropped, "fresh snapshot not served");
  pf::stop();
  hits = pf::stats().hits;
  check_all(t);
  EXPECT(pf::stats().hits == hits, "served after stop()");
}

}  // namespace

int main(int argc, char** argv) {
  // before any snapshot exists the interposed fopen is a plain pass-through
  FILE* self = fopen("/proc/self/status", "r");
  if (!self) {
    std::printf("FAIL: fopen before start()\n");
    return 1;
  }
  std::fclose(self);

  bool on = pf::enabled_by_env();
  for (int i = 1; i < argc; ++i)
    if (!std::strcmp(argv[i], "--no-prefetch")) on = false;
  char tmpl[] = "/tmp/sysfs-prefetch-XXXXXX";
  if (!mkdtemp(tmpl)) {
    std::printf("FAIL: mkdtemp: %s\n", std::strerror(errno));
    return 1;
  }
  const std::string top = tmpl;
  const Tree t = make_tree(top);
  if (on) run_on(t, top);
  else run_off(t);
  const std::string rm = "rm -rf '" + top + "'";
  if (std::system(rm.c_str()) != 0) std::printf("warning: could not remove %s\n", top.c_str());
  if (g_failed) return 1;
  std::printf("OK prefetch=%s files=%zu\n", on ? "on" : "off", t.listed.size());
  return 0;
}
