// xgmi-probe: RCCL-over-xGMI validation of the GPU set a pod was given.
//
// The reference has no collective or interconnect awareness at all. For
// topology-aware placement amdkube needs ground truth: this probe runs, over every GPU
// visible to the pod (one process, one communicator via ncclCommInitAll), an all-reduce
// bus-bandwidth sweep and a pairwise hipMemcpyPeer matrix. Before timing anything it checks
// the collective's RESULT (kernels/xgmi_pattern.h, xgmi_verify.h): rank i fills element e with
// (i+1) + 0.5*term(seed, e), where term is a hash of the seed and the 64-bit element index in [0, 4096),
// and after a sum all-reduce every rank must hold 0.5*n*(n+1) + 0.5*n*term(seed, e) in every element.
// The value says where it belongs, so a chunk of the result that lands in another chunk's place shows,
// whatever the distance. Every value and partial sum is a multiple of 0.5 of at most 133,120 for up to
// 64 ranks, far below 2^23, so the fp32 sum is exact in any reduction order and the check compares with !=.
// --selftest-flips N flips the low mantissa bit of N elements of the result (flip i on rank i % n, at the
// positions flip_positions(seed, N, elements) of check_core.h) before the count, which must then report
// exactly N.
// On an 8x MI355X node every GPU pair has one direct xGMI link (7 links x ~153 GB/s per GPU), so a ring all-reduce over k
// GPUs is per-link bound; the probe reports algbw and busbw = algbw * 2(k-1)/k.
// It also prints, per rank, the PCI bus id and UUID of the GPU the communicator opened, so the
// placement the scheduler bound (spec.extendedResources[].assigned → amd.com/pci-bus) can be
// checked against what RCCL actually ran on inside the pod.
//   xgmi-probe [--max-mib M] [--iters K] [--no-p2p] [--seed S] [--selftest-flips N]
// M in [1, 65536], K in [1, 10000], N in [0, 64], each a plain decimal number; S below 2^32, decimal or 0x hex
// (default 0x5eed). Prints one JSON line; "verify" has elements, ranks, wrong, seed, selftest_flips and
// first_errors (at most 16 of {rank, index, got, want}, got and want as raw fp32 bits).
// Exit 0 clean, 2 a bad argument (judged before anything touches the GPU), 4 a runtime error, 5 wrong elements.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include <sstream>

#include "xgmi_verify.h"

#define CHECK_HIP(x)                                                                          \
  do {                                                                                        \
    hipError_t e = (x);                                                                       \
    if (e != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e)); \
  } while (0)
#define CHECK_NCCL(x)                                                                             \
  do {                                                                                            \
    ncclResult_t r = (x);                                                                         \
    if (r != ncclSuccess) throw std::runtime_error(std::string(#x) + ": " + ncclGetErrorString(r)); \
  } while (0)

// s as a whole number in [lo, hi]: decimal digits only, or with `hex` also 0x and hex digits; no sign, no
// blanks, nothing after it. At most 12 digits, so the conversion cannot overflow.
static bool number(const char* s, bool hex, unsigned long long lo, unsigned long long hi, unsigned long long* out) {
  int base = 10;
  if (hex && s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) {
    base = 16;
    s += 2;
  }
  const size_t len = std::strlen(s);
  if (len == 0 || len > 12) return false;
  for (const char* c = s; *c; ++c) {
    const bool digit = *c >= '0' && *c <= '9';
    const bool letter = base == 16 && ((*c >= 'a' && *c <= 'f') || (*c >= 'A' && *c <= 'F'));
    if (!digit && !letter) return false;
  }
  *out = std::strtoull(s, nullptr, base);
  return *out >= lo && *out <= hi;
}

int main(int argc, char** argv) {
  unsigned long long max_mib = 256, iters_arg = 10, seed_arg = 0x5eedu, flips_arg = 0;
  bool p2p = true;
  auto bad_arg = [](const char* what, const char* v) {
    std::fprintf(stderr, "xgmi-probe: bad argument %s %s\n", what, v ? v : "(missing)");
    return 2;
  };
  const struct {
    const char* flag;
    bool hex;
    unsigned long long lo, hi, *out;
  } valued[] = {{"--max-mib", false, 1, 65536, &max_mib},
                {"--iters", false, 1, 10000, &iters_arg},
                {"--seed", true, 0, 0xffffffffull, &seed_arg},
                {"--selftest-flips", false, 0, amdkube::XGMI_MAX_FLIPS, &flips_arg}};
  for (int i = 1; i < argc; ++i) {
    const char* f = argv[i];
    if (!std::strcmp(f, "--no-p2p")) {
      p2p = false;
      continue;
    }
    const auto* spec = &valued[0];
    while (spec != std::end(valued) && std::strcmp(f, spec->flag)) ++spec;
    if (spec == std::end(valued)) return bad_arg(f, "(unknown flag)");
    const char* v = i + 1 < argc ? argv[++i] : nullptr;
    if (!v || !number(v, spec->hex, spec->lo, spec->hi, spec->out)) return bad_arg(f, v);
  }
  const int iters = static_cast<int>(iters_arg), flips = static_cast<int>(flips_arg);
  const uint32_t seed = static_cast<uint32_t>(seed_arg);
  try {
    int n = 0;
    CHECK_HIP(hipGetDeviceCount(&n));
    if (n < 1) throw std::runtime_error("no GPUs visible");
    std::ostringstream js;   // printed once at the end: RCCL writes its banner to stdout at init
    char tmp[256];
    std::snprintf(tmp, sizeof tmp, "{\"gpus\":%d,\"devices\":[", n);
    js << tmp;
    for (int i = 0; i < n; ++i) {
      char bus[64] = {0};
      CHECK_HIP(hipDeviceGetPCIBusId(bus, sizeof bus, i));
      hipUUID u;
      CHECK_HIP(hipDeviceGetUuid(&u, i));
      char hex[33];
      for (int b = 0; b < 16; ++b) std::snprintf(hex + 2 * b, 3, "%02x", static_cast<unsigned char>(u.bytes[b]));
      std::snprintf(tmp, sizeof tmp, "%s{\"rank\":%d,\"bus\":\"%s\",\"uuid\":\"%s\"}", i ? "," : "", i, bus, hex);
      js << tmp;
    }
    js << "],";
    std::vector<ncclComm_t> comms(n);
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) devs[i] = i;
    CHECK_NCCL(ncclCommInitAll(comms.data(), n, devs.data()));
    std::vector<float*> buf(n);
    std::vector<hipStream_t> st(n);
    const size_t max_bytes = max_mib << 20;
    for (int i = 0; i < n; ++i) {
      CHECK_HIP(hipSetDevice(i));
      CHECK_HIP(hipMalloc(&buf[i], max_bytes));
      CHECK_HIP(hipMemset(buf[i], 0, max_bytes));
      CHECK_HIP(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    }
    // correctness: rank-dependent values, sum all-reduce, every element checked on every rank
    const size_t vcount = (max_bytes < (64u << 20) ? max_bytes : (64u << 20)) / sizeof(float);
    unsigned long long wrong_total = 0;
    {
      amdkube::xgmi_check_ranks(n);
      for (int i = 0; i < n; ++i) {
        CHECK_HIP(hipSetDevice(i));
        amdkube::xgmi_fill_device(buf[i], vcount, i, seed, amdkube::XGMI_GRID, st[i]);
      }
      CHECK_NCCL(ncclGroupStart());
      for (int i = 0; i < n; ++i) CHECK_NCCL(ncclAllReduce(buf[i], buf[i], vcount, ncclFloat, ncclSum, comms[i], st[i]));
      CHECK_NCCL(ncclGroupEnd());
      // the self-test: flip f goes to rank f % n, so every rank's count is exercised
      const std::vector<uint32_t> flip_at = amdkube::flip_positions(seed, flips, vcount);
      std::ostringstream recs;
      int n_recs = 0;
      for (int i = 0; i < n; ++i) {
        CHECK_HIP(hipSetDevice(i));
        std::vector<uint32_t> mine;
        for (int f = i; f < flips; f += n) mine.push_back(flip_at[f]);
        amdkube::xgmi_flip_device(buf[i], vcount, mine, st[i]);
        const amdkube::XgmiCount c = amdkube::xgmi_count_wrong_device(buf[i], vcount, n, seed, amdkube::XGMI_GRID, st[i]);
        wrong_total += c.wrong;
        for (const amdkube::XgmiRecord& e : c.records) {
          if (n_recs == amdkube::XGMI_RECORDS) break;
          std::snprintf(tmp, sizeof tmp, "%s{\"rank\":%d,\"index\":%llu,\"got\":%u,\"want\":%u}", n_recs++ ? "," : "", i, e.index,
                        e.got, e.want);
          recs << tmp;
        }
      }
      std::snprintf(tmp, sizeof tmp, "\"verify\":{\"elements\":%zu,\"ranks\":%d,\"wrong\":%llu,\"seed\":%u,\"selftest_flips\":%d,",
                    vcount, n, wrong_total, seed, flips);
      js << tmp << "\"first_errors\":[" << recs.str() << "]},";
      for (int i = 0; i < n; ++i) {
        CHECK_HIP(hipSetDevice(i));
        CHECK_HIP(hipMemset(buf[i], 0, max_bytes));
      }
    }
    js << "\"allreduce\":[";
    bool first = true;
    for (size_t bytes = 1 << 20; bytes <= max_bytes; bytes <<= 2) {
      size_t count = bytes / sizeof(float);
      auto run = [&]() {
        CHECK_NCCL(ncclGroupStart());
        for (int i = 0; i < n; ++i) CHECK_NCCL(ncclAllReduce(buf[i], buf[i], count, ncclFloat, ncclSum, comms[i], st[i]));
        CHECK_NCCL(ncclGroupEnd());
      };
      run();
      for (int i = 0; i < n; ++i) {
        CHECK_HIP(hipSetDevice(i));
        CHECK_HIP(hipStreamSynchronize(st[i]));
      }
      auto t0 = std::chrono::steady_clock::now();
      for (int it = 0; it < iters; ++it) run();
      for (int i = 0; i < n; ++i) {
        CHECK_HIP(hipSetDevice(i));
        CHECK_HIP(hipStreamSynchronize(st[i]));
      }
      double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / iters;
      double alg = bytes / s / 1e9;
      double bus = n > 1 ? alg * 2.0 * (n - 1) / n : alg;
      std::snprintf(tmp, sizeof tmp, "%s{\"bytes\":%zu,\"us\":%.1f,\"algbw_gbps\":%.2f,\"busbw_gbps\":%.2f}", first ? "" : ",",
                    bytes, s * 1e6, alg, bus);
      js << tmp;
      first = false;
    }
    js << "],\"p2p_gbps\":[";
    for (int i = 0; i < n; ++i) {
      js << (i ? ",[" : "[");
      for (int j = 0; j < n; ++j) {
        double gbps = 0;
        if (p2p && i != j) {
          int can = 0;
          CHECK_HIP(hipDeviceCanAccessPeer(&can, i, j));
          if (can) {
            CHECK_HIP(hipSetDevice(i));
            hipDeviceEnablePeerAccess(j, 0);
            (void)hipGetLastError();
            size_t bytes = max_bytes;
            CHECK_HIP(hipMemcpyPeer(buf[j], j, buf[i], i, bytes));
            CHECK_HIP(hipDeviceSynchronize());
            auto t0 = std::chrono::steady_clock::now();
            for (int it = 0; it < 3; ++it) CHECK_HIP(hipMemcpyPeer(buf[j], j, buf[i], i, bytes));
            CHECK_HIP(hipDeviceSynchronize());
            double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / 3;
            gbps = bytes / s / 1e9;
          }
        }
        std::snprintf(tmp, sizeof tmp, "%s%.1f", j ? "," : "", gbps);
        js << tmp;
      }
      js << "]";
    }
    js << "]}";
    std::fflush(stdout);
    std::printf("%s\n", js.str().c_str());
    for (int i = 0; i < n; ++i) {
      ncclCommDestroy(comms[i]);
      hipSetDevice(i);
      hipFree(buf[i]);
      hipStreamDestroy(st[i]);
    }
    if (wrong_total) {
      std::fprintf(stderr, "xgmi-probe: all-reduce returned %llu wrong elements\n", wrong_total);
      return 5;
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "xgmi-probe: %s\n", e.what());
    return 4;
  }
}
