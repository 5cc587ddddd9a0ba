// Self-test for native/io_trace.h through this program's own fopen / fclose / open / opendir, defined
// the way kernels/hsa_vector_add.cpp defines them. Built plain, with -fsanitize=address,undefined and
// with -fsanitize=thread by native/build.py; run by tests/test_io_trace.py. Prints "OK …" and exits 0,
// or "FAIL …" and exits 1.
//
//   io-trace-selftest          everything below
//   io-trace-selftest paths    a few opens with the path listing on: the test reads the [path] lines
//
// It opens nothing under /dev but /dev/null; its open of "/dev/kfd" asks for a directory, which the
// kernel refuses before any driver sees it (or the file is not there at all).
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "io_trace.h"

namespace iotrace = amdkube::iotrace;
namespace prefetch = amdkube::prefetch;

static std::atomic<int> g_kfd_hook_calls{0};
static void kfd_hook() { g_kfd_hook_calls.fetch_add(1); }

extern "C" FILE* fopen(const char* path, const char* mode) { return iotrace::traced_fopen(path, mode); }
extern "C" int fclose(FILE* f) { return iotrace::traced_fclose(f); }
extern "C" DIR* opendir(const char* path) { return iotrace::traced_opendir(path); }
extern "C" int open(const char* path, int flags, ...) {
  va_list ap;
  va_start(ap, flags);
  const int fd = iotrace::traced_open(path, flags, ap, kfd_hook);
  va_end(ap);
  return fd;
}

namespace {

int g_failed = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

const char* const kFile = "/proc/self/stat";        // always there, and in a group of its own
const char* const kMissing = "/nonexistent-io-trace/file";

struct Counts {
  uint64_t fopens, fopen_ns, opens, open_ns, opendirs, opendir_ns;
};
Counts counts(int g) {
  const iotrace::Acc& a = iotrace::g_acc[g];
  return {a.fopens.load(), a.fopen_ns.load(), a.opens.load(), a.open_ns.load(), a.opendirs.load(), a.opendir_ns.load()};
}
uint64_t calls(const Counts& c) { return c.fopens + c.opens + c.opendirs; }
uint64_t all_calls() {
  uint64_t n = 0;
  for (int g = 0; g < iotrace::kGroups; ++g) n += calls(counts(g));
  return n;
}

std::string report_text(int64_t begin, int64_t end) {
  char buf[4096] = {0};
  FILE* f = fmemopen(buf, sizeof buf, "w");
  iotrace::report(f, begin, end);
  std::fclose(f);
  return buf;
}

std::vector<std::string> lines_of(const std::string& text) {
  std::vector<std::string> out;
  for (size_t at = 0; at < text.size();) {
    const size_t nl = text.find('\n', at);
    out.push_back(text.substr(at, nl - at));
    at = nl == std::string::npos ? text.size() : nl + 1;
  }
  return out;
}

// one round of every kind of call on paths that exist
void open_and_close_each(int rounds) {
  for (int i = 0; i < rounds; ++i) {
    if (FILE* f = fopen(kFile, "r")) fclose(f);
    const int fd = open("/dev/null", O_RDONLY);
    if (fd >= 0) close(fd);
    if (DIR* d = opendir("/proc/self")) closedir(d);
  }
}

void test_group_of() {
  using namespace iotrace;
  EXPECT(group_of("/sys/devices/virtual/kfd/kfd/topology/nodes/1/properties") == kTopology);
  EXPECT(group_of("/proc/cpuinfo") == kProc);
  EXPECT(group_of("/sys/devices/system/node/node0/cpu0/cache/index0/level") == kSysSystem);
  EXPECT(group_of("/sys/class/drm/renderD128") == kDrmPci && group_of("/sys/bus/pci/devices") == kDrmPci);
  EXPECT(group_of("/sys/devices/pci0000:00/0000:00:01.0/vendor") == kDrmPci && group_of("/sys/dev/char/226:128") == kDrmPci);
  EXPECT(group_of("/dev/kfd") == kDev && group_of("/dev/dri/renderD128") == kDev);
  EXPECT(group_of("/usr/share/libdrm/amdgpu.ids") == kOther && group_of("/sys/module/amdgpu") == kOther);
  EXPECT(group_of("/proc") == kOther && group_of("") == kOther && group_of(nullptr) == kOther);
}

// before anything was counted: the exact lines, and no split of the window without an open of /dev/kfd
void test_report_of_nothing() {
  std::string want;
  const char* names[] = {"kfd-topology", "/proc", "/sys/devices/system", "drm+pci", "/dev", "other"};
  for (const char* name : names)
    want += "[trace] io " + std::string(name) + std::string(19 - std::strlen(name), ' ') +
            " fopen=0 fopen_ms=0.000 open=0 open_ms=0.000 opendir=0 opendir_ms=0.000\n";
  EXPECT(report_text(1000, 2000) == want);
  char buf[128] = {0};
  FILE* f = fmemopen(buf, sizeof buf, "w");
  iotrace::print_phase(f, "hsa_init", 12.3456);
  iotrace::print_phase(f, "init:post-wait", 1234.5);
  std::fclose(f);
  EXPECT(std::string(buf) == "[trace] hsa_init         12.346 ms\n[trace] init:post-wait 1234.500 ms\n");
}

void test_outside_the_window_nothing_is_counted() {
  EXPECT(!iotrace::tracing());
  open_and_close_each(3);
  EXPECT(fopen(kMissing, "r") == nullptr && opendir(kMissing) == nullptr && open(kMissing, O_RDONLY) < 0);
  EXPECT(all_calls() == 0);
  // a window opened with tracing off is no window
  iotrace::window_begin(false, true);
  EXPECT(!iotrace::tracing() && !iotrace::g_paths.load());
  open_and_close_each(1);
  iotrace::window_end();
  EXPECT(all_calls() == 0);
}

void test_counts_equal_calls_per_group() {
  using namespace iotrace;
  // one path per group; whether it exists does not matter to the count
  const char* paths[kGroups] = {"/sys/devices/virtual/kfd/kfd/topology/generation_id", "/proc/self/stat",
                                "/sys/devices/system/cpu/online", "/sys/class/drm/version", "/dev/null", "/etc/hostname"};
  Counts before[kGroups];
  for (int g = 0; g < kGroups; ++g) before[g] = counts(g);
  window_begin(true, false);
  EXPECT(tracing());
  for (int g = 0; g < kGroups; ++g) {
    for (int i = 0; i < g + 1; ++i)
      if (FILE* f = fopen(paths[g], "r")) fclose(f);
    for (int i = 0; i < g + 2; ++i) {
      const int fd = open(paths[g], O_RDONLY);
      if (fd >= 0) close(fd);
    }
    for (int i = 0; i < g + 3; ++i)
      if (DIR* d = opendir(paths[g])) closedir(d);
  }
  // the prefetch helper's own reads are left out
  std::thread([] {
    prefetch::t_in_helper = true;
    EXPECT(!tracing());
    open_and_close_each(2);
  }).join();
  window_end();
  EXPECT(!tracing());
  for (int g = 0; g < kGroups; ++g) {
    const Counts c = counts(g);
    EXPECT(c.fopens - before[g].fopens == uint64_t(g + 1) && c.opens - before[g].opens == uint64_t(g + 2) &&
           c.opendirs - before[g].opendirs == uint64_t(g + 3));
    EXPECT(c.fopen_ns > before[g].fopen_ns && c.open_ns > before[g].open_ns && c.opendir_ns > before[g].opendir_ns);
  }
}

// a failing call leaves errno as libc set it, inside the window and outside
void test_errno_is_libcs() {
  using namespace iotrace;
  errno = 0;
  EXPECT(prefetch::next_fopen()(kMissing, "r") == nullptr);
  const int fopen_errno = errno;
  errno = 0;
  EXPECT(next(g_opendir, "opendir")(kFile) == nullptr);   // not a directory
  const int opendir_errno = errno;
  errno = 0;
  EXPECT(next(g_open, "open")(kMissing, O_RDONLY) < 0);
  const int open_errno = errno;
  errno = 0;
  EXPECT(next(g_open, "open")("/dev/kfd", O_RDONLY | O_DIRECTORY) < 0);
  const int kfd_errno = errno;
  EXPECT(fopen_errno == ENOENT && opendir_errno == ENOTDIR && open_errno == ENOENT && (kfd_errno == ENOTDIR || kfd_errno == ENOENT));
  const Counts dev_before = counts(kDev);
  for (bool inside : {false, true}) {
    if (inside) window_begin(true, false);
    const int hook_calls = g_kfd_hook_calls.load();
    errno = 0;
    EXPECT(fopen(kMissing, "r") == nullptr && errno == fopen_errno);
    errno = 0;
    EXPECT(opendir(kFile) == nullptr && errno == opendir_errno);
    errno = 0;
    EXPECT(open(kMissing, O_RDONLY) < 0 && errno == open_errno);
    EXPECT(g_kfd_hook_calls.load() == hook_calls);
    // the hook runs once the open of /dev/kfd has returned, traced or not, and errno survives it
    errno = 0;
    EXPECT(open("/dev/kfd", O_RDONLY | O_DIRECTORY) < 0 && errno == kfd_errno);
    EXPECT(g_kfd_hook_calls.load() == hook_calls + 1);
    if (inside) window_end();
  }
  EXPECT(counts(kDev).opens == dev_before.opens + 1);   // the one inside the window
  // that open, the first of /dev/kfd inside a window, is where report() splits the window
  const int64_t enter = g_kfd_enter_ns.load(), ret = g_kfd_return_ns.load();
  EXPECT(enter > 0 && ret >= enter);
  window_begin(true, false);
  open("/dev/kfd", O_RDONLY | O_DIRECTORY);
  window_end();
  EXPECT(g_kfd_enter_ns.load() == enter && g_kfd_return_ns.load() == ret);   // later ones do not move it
}

// sysfs formats its answer in the read: a stdio file's time runs from fopen to fclose
void test_stdio_time_is_charged_at_fclose() {
  using namespace iotrace;
  window_begin(true, false);
  const Counts c0 = counts(kProc);
  FILE* f = fopen(kFile, "r");
  EXPECT(f != nullptr);
  const Counts c1 = counts(kProc);
  EXPECT(c1.fopens == c0.fopens + 1 && c1.fopen_ns == c0.fopen_ns);
  char buf[64];
  EXPECT(std::fread(buf, 1, sizeof buf, f) > 0);
  EXPECT(counts(kProc).fopen_ns == c0.fopen_ns);
  fclose(f);
  const Counts c2 = counts(kProc);
  EXPECT(c2.fopens == c1.fopens && c2.fopen_ns > c0.fopen_ns);
  // a failed fopen has no fclose: charged at once
  const Counts o0 = counts(kOther);
  EXPECT(fopen(kMissing, "r") == nullptr);
  EXPECT(counts(kOther).fopens == o0.fopens + 1 && counts(kOther).fopen_ns > o0.fopen_ns);
  window_end();
  // a file opened before the window has no span: closing it inside charges nothing
  const Counts c3 = counts(kProc);
  FILE* early = fopen(kFile, "r");
  window_begin(true, false);
  fclose(early);
  window_end();
  EXPECT(counts(kProc).fopen_ns == c3.fopen_ns && counts(kProc).fopens == c3.fopens);
  for (const Span& s : g_spans) EXPECT(s.f == nullptr);
}

// the table holds 64 files: further ones are counted, and silently not timed
void test_more_than_64_open_files() {
  using namespace iotrace;
  window_begin(true, false);
  const Counts c0 = counts(kProc);
  std::vector<FILE*> files;
  for (int i = 0; i < 70; ++i) files.push_back(fopen(kFile, "r"));
  int held = 0;
  for (FILE* f : files) EXPECT(f != nullptr);
  for (const Span& s : g_spans) held += s.f != nullptr;
  EXPECT(held == 64 && counts(kProc).fopens == c0.fopens + 70 && counts(kProc).fopen_ns == c0.fopen_ns);
  for (int i = 64; i < 70; ++i) fclose(files[i]);                       // the untracked ones
  EXPECT(counts(kProc).fopen_ns == c0.fopen_ns);
  uint64_t last = c0.fopen_ns;
  for (int i = 0; i < 64; ++i) {                                         // each of the first 64 is charged
    fclose(files[i]);
    const uint64_t now = counts(kProc).fopen_ns;
    EXPECT(now > last);
    last = now;
  }
  for (const Span& s : g_spans) EXPECT(s.f == nullptr);
  // and the freed slots are used again
  FILE* f = fopen(kFile, "r");
  EXPECT(g_spans[0].f == f);
  fclose(f);
  window_end();
}

void test_two_threads() {
  using namespace iotrace;
  const Counts p0 = counts(kProc), d0 = counts(kDev);
  window_begin(true, false);
  std::thread a(open_and_close_each, 200), b(open_and_close_each, 200);
  a.join();
  b.join();
  window_end();
  const Counts p1 = counts(kProc), d1 = counts(kDev);
  EXPECT(p1.fopens == p0.fopens + 400 && p1.opendirs == p0.opendirs + 400 && d1.opens == d0.opens + 400);
  for (const Span& s : g_spans) EXPECT(s.f == nullptr);
}

// one io line per group in the fixed order, after the three parts of the window
void test_report() {
  using namespace iotrace;
  const int64_t enter = g_kfd_enter_ns.load(), ret = g_kfd_return_ns.load();
  const std::vector<std::string> lines = lines_of(report_text(enter - 2000000, ret + 3000000));
  EXPECT(lines.size() == 3 + kGroups);
  if (lines.size() != 3 + kGroups) return;
  EXPECT(lines[0] == "[trace] init:pre-open     2.000 ms");
  EXPECT(lines[1].rfind("[trace] init:kfd-wait  ", 0) == 0 && lines[1].size() == std::strlen("[trace] init:pre-open     2.000 ms"));
  EXPECT(lines[2] == "[trace] init:post-wait    3.000 ms");
  for (int g = 0; g < kGroups; ++g) {
    char name[32];
    unsigned long long fopens = 0, opens = 0, opendirs = 0;
    double fopen_ms = -1, open_ms = -1, opendir_ms = -1;
    EXPECT(std::sscanf(lines[3 + g].c_str(), "[trace] io %31s fopen=%llu fopen_ms=%lf open=%llu open_ms=%lf opendir=%llu opendir_ms=%lf",
                       name, &fopens, &fopen_ms, &opens, &open_ms, &opendirs, &opendir_ms) == 7);
    const Counts c = counts(g);
    EXPECT(std::string(name) == kGroupName[g] && fopens == c.fopens && opens == c.opens && opendirs == c.opendirs);
    EXPECT(fopen_ms >= 0 && open_ms >= 0 && opendir_ms >= 0);
  }
}

int list_paths() {
  iotrace::window_begin(true, true);
  if (FILE* f = fopen(kFile, "r")) fclose(f);
  fopen(kMissing, "r");
  if (DIR* d = opendir("/proc/self")) closedir(d);
  opendir(kMissing);
  const int fd = open("/dev/null", O_RDONLY);   // an open is counted, never listed
  if (fd >= 0) close(fd);
  iotrace::window_end();
  fopen(kMissing, "r");                          // outside the window: not listed
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "paths")) return list_paths();
  test_group_of();
  test_report_of_nothing();
  test_outside_the_window_nothing_is_counted();
  test_counts_equal_calls_per_group();
  test_errno_is_libcs();
  test_stdio_time_is_charged_at_fclose();
  test_more_than_64_open_files();
  test_two_threads();
  test_report();
  if (g_failed) {
    std::printf("FAIL: %d check(s)\n", g_failed);
    return 1;
  }
  std::printf("OK io_trace: groups, window, counts, errno, stdio spans, span table, threads, report\n");
  return 0;
}
