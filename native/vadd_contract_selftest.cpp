// Self-test of kernels/vadd_contract.h on the CPU (no HIP, no HSA): the parser, the inputs, the
// verification and the grid against transcriptions of the two copies the header replaced
// (rocm-vector-add's and hsa-vector-add's), and every printer against the literal lines those programs
// printed. The verification differs from the two copies in one way, on purpose: a NaN difference counts. Built plain and with ASan/UBSan (native/build.py), run by tests/test_vadd_contract.py.
// Prints "OK ..." and exits 0, or says what failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

#include "../kernels/vadd_contract.h"

using namespace amdkube;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

// ---- the parser
static VaddOptions parse(std::initializer_list<const char*> args) {
  std::vector<char*> argv{const_cast<char*>("prog")};
  for (const char* a : args) argv.push_back(const_cast<char*>(a));
  return vadd_parse_args(static_cast<int>(argv.size()), argv.data());
}

static bool same(const VaddOptions& a, const VaddOptions& b) {
  return a.n == b.n && a.print_uuid == b.print_uuid && a.json == b.json && a.expect_devices == b.expect_devices &&
         a.fast_exit == b.fast_exit && a.no_prefetch == b.no_prefetch;
}

static void test_parser() {
  const VaddOptions none = parse({});
  CHECK(none.n == 50000 && !none.print_uuid && !none.json && none.expect_devices == -1 && !none.fast_exit && !none.no_prefetch);
  CHECK(parse({"-n", "1025"}).n == 1025);
  CHECK(parse({"--elements", "3"}).n == 3);
  CHECK(parse({"-n", "0"}).n == 0);                       // the programs refuse it, each in its own words
  CHECK(parse({"-n", "12abc"}).n == 12);                  // strtoull: leading digits
  CHECK(parse({"-n", "abc"}).n == 0);
  CHECK(parse({"--print-uuid"}).print_uuid && parse({"--json"}).json);
  CHECK(parse({"--expect-devices", "2"}).expect_devices == 2);
  CHECK(parse({"--expect-devices", "x"}).expect_devices == 0);   // atoi
  CHECK(parse({"--fast-exit"}).fast_exit && parse({"--no-prefetch"}).no_prefetch);
  const VaddOptions all = parse({"--no-prefetch", "--json", "-n", "7", "--fast-exit", "--expect-devices", "1", "--print-uuid"});
  CHECK(all.n == 7 && all.print_uuid && all.json && all.expect_devices == 1 && all.fast_exit && all.no_prefetch);
  // a value flag that is the last argument is ignored
  CHECK(same(parse({"-n"}), none) && same(parse({"--elements"}), none) && same(parse({"--expect-devices"}), none));
  CHECK(parse({"--json", "-n"}).n == 50000 && parse({"--json", "-n"}).json);
  // unknown flags and stray words are ignored
  CHECK(same(parse({"--frobnicate", "12", "-x", "--elements=5"}), none));
  // a value flag takes whatever follows it, a flag included
  CHECK(parse({"-n", "--json"}).n == 0 && !parse({"-n", "--json"}).json);
  CHECK(!parse({"-n", "--fast-exit"}).fast_exit);
  // ... except that --no-prefetch is seen wherever it stands (hsa-vector-add's main scanned for it by itself)
  CHECK(parse({"-n", "--no-prefetch"}).no_prefetch && parse({"-n", "--no-prefetch"}).n == 0);
  CHECK(parse({"-n", "5", "-n", "9"}).n == 9);
}

// ---- the inputs: the loop both programs carried, word for word
static void old_fill(std::vector<float>& ha, std::vector<float>& hb, size_t n) {
  uint32_t s = 12345u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    ha[i] = static_cast<float>(s >> 8) / 16777216.0f;
    s = s * 1664525u + 1013904223u;
    hb[i] = static_cast<float>(s >> 8) / 16777216.0f;
  }
}

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

static void test_inputs() {
  for (size_t n : {1, 3, 255, 1025, 50000}) {
    std::vector<float> a(n + 1, -7.0f), b(n + 1, -7.0f), oa(n), ob(n);
    vadd_fill_inputs(a.data(), b.data(), n);
    old_fill(oa, ob, n);
    CHECK(std::memcmp(a.data(), oa.data(), n * sizeof(float)) == 0 && std::memcmp(b.data(), ob.data(), n * sizeof(float)) == 0);
    CHECK(a[n] == -7.0f && b[n] == -7.0f);   // nothing past n
    // as the parent's programs produced them
    CHECK(bits(a[0]) == 0x3ca72380u && bits(b[0]) == 0x3c878f40u);
    if (n == 50000) CHECK(bits(a[49999]) == 0x3e74d5d4u && bits(b[49999]) == 0x3e20bfecu);
  }
}

// ---- the verification: the two forms it replaced
static size_t old_hip_count(const float* ha, const float* hb, const float* hc, size_t n) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) {
    float d = hc[i] - (ha[i] + hb[i]);
    if (d > 1e-5f || d < -1e-5f) ++bad;
  }
  return bad;
}

static size_t old_hsa_count(const float* ha, const float* hb, const float* hc, size_t n) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i)
    if (std::fabs(ha[i] + hb[i] - hc[i]) > 1e-5f) ++bad;
  return bad;
}

static size_t count3(const std::vector<float>& a, const std::vector<float>& b, const std::vector<float>& c, size_t expect) {
  const size_t got = vadd_count_mismatches(a.data(), b.data(), c.data(), a.size());
  CHECK(got == old_hip_count(a.data(), b.data(), c.data(), a.size()));
  CHECK(got == old_hsa_count(a.data(), b.data(), c.data(), a.size()));
  CHECK(got == expect);
  return got;
}

static void test_verification() {
  const float inf = std::numeric_limits<float>::infinity();
  const size_t n = 1025;
  std::vector<float> a(n), b(n), c(n);
  vadd_fill_inputs(a.data(), b.data(), n);
  for (size_t i = 0; i < n; ++i) c[i] = a[i] + b[i];
  count3(a, b, c, 0);                                                   // exact sums
  for (float e : {2e-5f, -2e-5f}) {                                     // an error of 2e-5, either sign
    std::vector<float> x = c;
    x[0] += e, x[511] += e, x[n - 1] += e;
    count3(a, b, x, 3);
  }
  // just under the bound passes, just over it fails; around 0.5 a float step is 6e-8, so both are exact enough
  count3({0.25f, 0.25f}, {0.25f, 0.25f}, {0.5f + 0.99e-5f, 0.5f - 0.99e-5f}, 0);
  count3({0.25f, 0.25f}, {0.25f, 0.25f}, {0.5f + 1.01e-5f, 0.5f - 1.01e-5f}, 2);
  count3({0.0f, -0.0f, 0.0f, -0.0f}, {0.0f, -0.0f, -0.0f, 0.0f}, {-0.0f, 0.0f, 0.0f, -0.0f}, 0);   // signed zeros are equal
  count3({0.5f, 0.5f}, {0.25f, 0.25f}, {inf, -inf}, 2);                 // an infinite result is a mismatch
  count3({0.0f}, {0.0f}, {1.0f}, 1);
  count3({}, {}, {}, 0);
}

// The one intended difference from the two loops: a difference that is NaN counts, 1 per element. Those
// loops compared "> 1e-5", which is false for NaN, so they return 0 on every input here.
static void count_nan(const std::vector<float>& a, const std::vector<float>& b, const std::vector<float>& c, size_t expect) {
  CHECK(vadd_count_mismatches(a.data(), b.data(), c.data(), a.size()) == expect);
  CHECK(old_hip_count(a.data(), b.data(), c.data(), a.size()) == 0);
  CHECK(old_hsa_count(a.data(), b.data(), c.data(), a.size()) == 0);
}

static void test_nan_counts() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  float ff;
  std::memset(&ff, 0xff, sizeof ff);
  CHECK(ff != ff);
  count_nan({0.5f}, {0.25f}, {nan}, 1);                   // NaN in c
  count_nan({0.5f}, {0.25f}, {-nan}, 1);
  count_nan({0.5f}, {0.25f}, {ff}, 1);                    // the 0xff fill: an element the GPU never wrote
  count_nan({nan}, {0.25f}, {0.75f}, 1);                  // a NaN input
  count_nan({0.25f}, {nan}, {nan}, 1);                    // ... even where c is the NaN the GPU would give
  count_nan({inf}, {0.25f}, {inf}, 1);                    // inf - inf is NaN too
  count_nan({-inf}, {0.25f}, {-inf}, 1);
  // among good elements each is counted once, wherever it stands: a whole run whose c stayed at the fill
  const size_t n = 1025;
  std::vector<float> a(n), b(n), c(n);
  vadd_fill_inputs(a.data(), b.data(), n);
  for (size_t i = 0; i < n; ++i) c[i] = a[i] + b[i];
  std::vector<float> x = c;
  x[0] = ff, x[512] = nan, x[n - 1] = ff;
  count_nan(a, b, x, 3);
  x[7] += 2e-5f;                                          // next to an ordinary mismatch, which all three see
  CHECK(vadd_count_mismatches(a.data(), b.data(), x.data(), n) == 4);
  CHECK(old_hip_count(a.data(), b.data(), x.data(), n) == 1 && old_hsa_count(a.data(), b.data(), x.data(), n) == 1);
  std::memset(c.data(), 0xff, n * sizeof(float));
  count_nan(a, b, c, n);
}

// ---- the grid: the two formulas it replaced
static int old_hip_grid(size_t items, int cu_count, int per_cu) {
  size_t want = (items + 255) / 256;
  size_t cap = static_cast<size_t>(cu_count > 0 ? cu_count : 256) * per_cu;
  if (want < 1) want = 1;
  return static_cast<int>(want < cap ? want : cap);
}

static uint32_t old_hsa_groups(uint64_t floats, uint32_t cus) {
  const uint32_t kWG = 256;
  const uint64_t want = (floats / 4 + kWG - 1) / kWG;
  const uint64_t cap = static_cast<uint64_t>(cus ? cus : 256) * 64;
  return static_cast<uint32_t>(want < 1 ? 1 : (want < cap ? want : cap));
}

static void test_grid() {
  static_assert(VADD_WG == 256 && VADD_BLOCKS_PER_CU == 64, "the kernels' launch bounds and the tuned cap");
  for (int cus : {0, 1, 256})
    for (size_t items = 0; items <= 5000; ++items) {
      for (int per_cu : {8, 32, 64, 128}) CHECK(stream_grid(items, cus, per_cu) == old_hip_grid(items, cus, per_cu));
      CHECK(stream_grid(items, cus) == old_hip_grid(items, cus, 8));
      // hsa-vector-add passes whole 16-byte words: floats / 4
      for (size_t floats = 4 * items; floats < 4 * items + 4; ++floats)
        CHECK(static_cast<uint32_t>(stream_grid(floats / 4, cus, VADD_BLOCKS_PER_CU)) == old_hsa_groups(floats, cus));
    }
  // the cap at cu_count * per_cu, and 256 CUs assumed where the count is unknown
  for (size_t items : {size_t(1) << 22, size_t(1) << 40}) {
    CHECK(stream_grid(items, 1, 64) == 64 && stream_grid(items, 256, 64) == 16384 && stream_grid(items, 0, 64) == 16384);
    CHECK(static_cast<uint32_t>(stream_grid(items, 256, 64)) == old_hsa_groups(4 * items, 256));
    CHECK(static_cast<uint32_t>(stream_grid(items, 0, 64)) == old_hsa_groups(4 * items, 0));
    CHECK(static_cast<uint32_t>(stream_grid(items, 1, 64)) == old_hsa_groups(4 * items, 1));
  }
  CHECK(stream_grid(0, 256, 64) == 1 && stream_grid(256, 256, 64) == 1 && stream_grid(257, 256, 64) == 2);
  // the two programs' item counts part at n = 1025: 257 words rounded up, 256 rounded down
  CHECK(stream_grid((1025 + 3) / 4, 256, 64) == 2 && stream_grid(1025 / 4, 256, 64) == 1);
}

// ---- the printers, against the lines of the two programs
template <typename Print>
static std::string printed(Print print) {
  char buf[1024] = {0};
  FILE* f = fmemopen(buf, sizeof buf, "w");
  print(f);
  std::fclose(f);
  return buf;
}

static void test_printers() {
  const VaddGpu g{"AMD Instinct MI355X", "gfx950:sramecc+:xnack-", "0000:05:00.0", "GPU-0123456789abcdef", 256, 1};
  const VaddGpu unnamed{"", "gfx950:sramecc+:xnack-", "0000:05:00.0", "GPU-0123456789abcdef", 256, 8};
  CHECK(printed([&](FILE* f) { vadd_print_identity(f, g); }) ==
        "GPU 0: AMD Instinct MI355X gfx950:sramecc+:xnack- bus=0000:05:00.0 uuid=GPU-0123456789abcdef cus=256 visible=1\n");
  CHECK(printed([&](FILE* f) { vadd_print_identity(f, unnamed); }) ==
        "GPU 0: AMD Instinct GPU gfx950:sramecc+:xnack- bus=0000:05:00.0 uuid=GPU-0123456789abcdef cus=256 visible=8\n");
  CHECK(std::string(VADD_FALLBACK_NAME) == "AMD Instinct GPU");
  CHECK(printed([&](FILE* f) { vadd_print_header(f, 50000); }) == "[Vector addition of 50000 elements]\n");
  CHECK(printed([&](FILE* f) { vadd_print_json(f, 0, 50000, 0.12345, g); }) ==
        "{\"ok\":true,\"n\":50000,\"kernel_ms\":0.1235,\"uuid\":\"GPU-0123456789abcdef\",\"bus\":\"0000:05:00.0\","
        "\"arch\":\"gfx950:sramecc+:xnack-\",\"visible\":1}\n");
  CHECK(printed([&](FILE* f) { vadd_print_json(f, 3, 1025, 12.5, g, ",\"runtime\":\"hsa\",\"prefetch\":true"); }) ==
        "{\"ok\":false,\"n\":1025,\"kernel_ms\":12.5000,\"uuid\":\"GPU-0123456789abcdef\",\"bus\":\"0000:05:00.0\","
        "\"arch\":\"gfx950:sramecc+:xnack-\",\"visible\":1,\"runtime\":\"hsa\",\"prefetch\":true}\n");
  int rc = -1;
  CHECK(printed([&](FILE* f) { rc = vadd_print_verdict(f, 0); }) == "Test PASSED\n" && rc == 0);
  CHECK(printed([&](FILE* f) { rc = vadd_print_verdict(f, 17); }) == "Result verification failed (17 mismatches)\nTest FAILED\n" &&
        rc == 1);
  CHECK(printed([&](FILE* f) { rc = vadd_print_no_gpu(f); }) == "no GPU visible to this container\n" && rc == 2);
  CHECK(printed([&](FILE* f) { rc = vadd_print_no_gpu(f, "hsa_init: HSA_STATUS_ERROR_OUT_OF_RESOURCES: it failed"); }) ==
        "no GPU visible to this container (hsa_init: HSA_STATUS_ERROR_OUT_OF_RESOURCES: it failed)\n" && rc == 2);
  // the device-count checks: none visible, not the expected number, and the ways on
  CHECK(printed([&](FILE* f) { rc = vadd_check_device_count(f, 0, -1); }) == "no GPU visible to this container\n" && rc == 2);
  CHECK(printed([&](FILE* f) { rc = vadd_check_device_count(f, 0, 0); }) == "no GPU visible to this container\n" && rc == 2);
  CHECK(printed([&](FILE* f) { rc = vadd_check_device_count(f, 1, 2); }) == "expected 2 visible GPU(s), found 1\n" && rc == 3);
  CHECK(printed([&](FILE* f) { rc = vadd_check_device_count(f, 8, 1); }) == "expected 1 visible GPU(s), found 8\n" && rc == 3);
  CHECK(printed([&](FILE* f) { rc = vadd_check_device_count(f, 1, -1); }).empty() && rc == -1);
  CHECK(printed([&](FILE* f) { rc = vadd_check_device_count(f, 2, 2); }).empty() && rc == -1);
  CHECK(VADD_PASSED == 0 && VADD_MISMATCHES == 1 && VADD_NO_GPU == 2 && VADD_WRONG_DEVICE_COUNT == 3 && VADD_ERROR == 4);
}

int main() {
  test_parser();
  test_inputs();
  test_verification();
  test_nan_counts();
  test_grid();
  test_printers();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK vadd_contract: parser, inputs, verification, nan counts, grid, printers\n");
  return 0;
}
