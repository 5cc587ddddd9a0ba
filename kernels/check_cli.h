// The command line of the check programs (cu-check, lane-check, atomic-check, hbm-check) and the pieces of their
// JSON line that are the same in all of them. Plain C++17 with no HIP include: native/check_core_selftest.cpp
// checks the parser on the CPU, plain and under ASan/UBSan. The flags are judged before anything touches the GPU.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>

#include "check_core.h"

namespace amdkube {

// The flags every check program takes: --ms D (not hbm-check), --rounds R, --device D, --seed S and
// --selftest-flips N. parse() returns 0, or 2 with the line for stderr in `err`.
struct CheckCli {
  const char* prog;
  long max_flips;
  long max_rounds = 2000000000;
  bool takes_ms = true;
  double ms = 200;
  long rounds = 0, device = 0, flips = 0;
  uint32_t seed = 0x5eedu;
  std::string err;

  static constexpr int unknown = -1;  // a program's value(): the flag is not one of mine

  int fail(const std::string& what) {
    err = std::string(prog) + ": " + what + "\n";
    return 2;
  }
  int bad_arg(const char* what, const char* v) { return fail(std::string("bad argument ") + what + " " + (v ? v : "(missing)")); }
  // the whole string, base 0: 0x10 is 16
  static bool integer(const char* s, long* out) {
    char* end = nullptr;
    *out = std::strtol(s, &end, 0);
    return end != s && *end == 0;
  }
  static bool integer(const char* s, long* out, long lo, long hi) { return integer(s, out) && *out >= lo && *out <= hi; }
  // the whole string; the callers' range tests are written so that a NaN fails them
  static bool real(const char* s, double* out) {
    char* end = nullptr;
    *out = std::strtod(s, &end);
    return end != s && *end == 0;
  }

  // `bools` are the program's flags without a value, recognised before a value is fetched. Every other flag
  // takes one; value(flag, v) handles the program's own: 0 taken, `unknown`, or what bad_arg / fail returned.
  // A std::invalid_argument thrown by it is a failure with its text.
  template <class Value>
  int parse(int argc, char** argv, std::initializer_list<std::pair<const char*, bool*>> bools, Value&& value) {
    for (int i = 1; i < argc; ++i) {
      const char* f = argv[i];
      bool is_bool = false;
      for (const auto& b : bools)
        if (!std::strcmp(f, b.first)) *b.second = is_bool = true;
      if (is_bool) continue;
      const char* v = i + 1 < argc ? argv[++i] : nullptr;
      if (!v) return bad_arg(f, v);
      if (takes_ms && !std::strcmp(f, "--ms")) {
        if (!real(v, &ms) || !(ms > 0)) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--rounds")) {
        if (!integer(v, &rounds, 1, max_rounds)) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--device")) {
        if (!integer(v, &device) || device < 0) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--seed")) {  // negative and overflowing values wrap
        char* end = nullptr;
        seed = static_cast<uint32_t>(std::strtoul(v, &end, 0));
        if (end == v || *end) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--selftest-flips")) {
        if (!integer(v, &flips, 0, max_flips)) return bad_arg(f, v);
      } else {
        int rc;
        try {
          rc = value(f, v);
        } catch (const std::invalid_argument& e) {
          return fail(e.what());
        }
        if (rc == unknown) return bad_arg(f, "(unknown flag)");
        if (rc) return rc;
      }
    }
    return 0;
  }
  // the exit code of a refused command line, its line written to stderr
  int refuse() const {
    std::fputs(err.c_str(), stderr);
    return 2;
  }
};

// what runs once the flags are accepted: body()'s exit code, or 4 with the text of what it threw
template <class Body>
inline int check_run(const char* prog, Body&& body) {
  try {
    return body();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s: %s\n", prog, e.what());
    return 4;
  }
}

// ---- the JSON line: its head, and the members that more than one program prints
inline void print_head(int device, const std::string& uuid, const std::string& arch) {
  std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\"", device, uuid.c_str(), arch.c_str());
}

inline void print_units(int mask, const char* const* names, int n) {
  std::printf(",\"units\":[");
  bool first = true;
  for (int u = 0; u < n; ++u)
    if (mask & (1 << u)) {
      std::printf("%s\"%s\"", first ? "" : ",", names[u]);
      first = false;
    }
  std::printf("]");
}

inline void print_location(const CuLocation& l) {
  std::printf("\"xcc\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d", l.xcc, l.se, l.sh, l.cu);
}

inline void print_bad_cus(const std::vector<CuBadCu>& bad) {
  std::printf(",\"bad_cus\":[");
  for (size_t i = 0; i < bad.size(); ++i) {
    std::printf("%s{", i ? "," : "");
    print_location(bad[i].where);
    std::printf(",\"errors\":%llu}", bad[i].errors);
  }
  std::printf("]");
}

}  // namespace amdkube
