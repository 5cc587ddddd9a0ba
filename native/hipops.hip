// In-process HIP validation ops (pybind11 module amdkube._native._hipops).
//
// The AMD device plugin uses these as its health probe (HBM pattern check before a GPU
// is advertised Healthy) and the GPU test tier uses them to check the kernels against a
// host fp32 reference. Kernels live in kernels/ (gpu_common.h and the check headers, shared with the pod binaries).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "../kernels/cu_check.h"
#include "../kernels/hbm_check.h"
#include "../kernels/mfma_check_lp.h"

namespace py = pybind11;

// the result of a check run, with its rate under `rate_key`
static py::dict check_result(const amdkube::MfmaCheckResult& r, const char* rate_key) {
  py::list recs;
  for (const amdkube::MfmaCheckRecord& e : r.first_errors) {
    py::dict d;
    d["block"] = e.block;
    d["row"] = e.row;
    d["col"] = e.col;
    d["round"] = e.round;
    d["got"] = e.got;
    d["want"] = e.want;
    recs.append(d);
  }
  py::dict o;
  o["ok"] = r.errors == 0;
  o["errors"] = r.errors;
  o["rounds"] = r.rounds;
  o["blocks"] = r.blocks;
  o["k"] = r.k;
  o["ms"] = r.ms;
  o[rate_key] = r.tflops;
  o["first_errors"] = recs;
  return o;
}

static py::dict cu_location(const amdkube::CuLocation& l) {
  py::dict d;
  d["xcc"] = l.xcc;
  d["se"] = l.se;
  d["sh"] = l.sh;
  d["cu"] = l.cu;
  return d;
}

// the result of a per-CU check run (kernels/cu_check.h)
static py::dict cu_check_result(const amdkube::CuCheckResult& r) {
  py::dict o, by_unit;
  py::list units, locations, bad, recs;
  for (int u = 0; u < 3; ++u) {
    if (r.units & (1 << u)) units.append(amdkube::CU_UNIT_NAMES[u]);
    by_unit[amdkube::CU_UNIT_NAMES[u]] = r.errors_by_unit[u];
  }
  for (const amdkube::CuLocation& l : r.locations) locations.append(cu_location(l));
  for (const amdkube::CuCheckBadCu& b : r.bad_cus) {
    py::dict d = cu_location(b.where);
    d["errors"] = b.errors;
    bad.append(d);
  }
  for (const amdkube::CuCheckRecord& e : r.first_errors) {
    py::dict d = cu_location(amdkube::cu_decode_location(e.hw_id, e.xcc_id));
    d["unit"] = amdkube::CU_UNIT_NAMES[e.unit < 3 ? e.unit : 0];
    d["block"] = e.block;
    d["round"] = e.round;
    d["pass"] = e.pass;
    d["index"] = e.index;
    d["got"] = e.got;
    d["want"] = e.want;
    recs.append(d);
  }
  o["ok"] = r.errors == 0;
  o["errors"] = r.errors;
  o["errors_by_unit"] = by_unit;
  o["units"] = units;
  o["rounds"] = r.rounds;
  o["blocks"] = r.blocks;
  o["launches"] = r.launches;
  o["ms"] = r.ms;
  o["lds_gbps"] = r.lds_gbps;
  o["valu_gops"] = r.valu_gops;
  o["cus"] = r.cus;
  o["cus_covered"] = r.cus_covered;
  o["xccs"] = r.xccs;
  o["locations"] = locations;
  // raw HW_ID and XCC_ID words of every workgroup of the timed launch
  o["block_loc"] = py::array_t<uint32_t>({static_cast<py::ssize_t>(r.blocks), static_cast<py::ssize_t>(2)}, r.block_loc.data());
  o["bad_cus"] = bad;
  o["first_errors"] = recs;
  return o;
}

// the counters and records of an HBM check or of one march launch (kernels/hbm_check.h)
static void hbm_check_counts(const amdkube::HbmCheckResult& r, const char* records_key, py::dict& o) {
  py::list recs;
  for (const amdkube::HbmCheckRecord& e : r.first_errors) {
    py::dict d = cu_location(amdkube::cu_decode_location(e.hw_id, e.xcc_id));
    d["round"] = e.round;
    d["pass"] = e.pass;
    d["chunk"] = e.chunk;
    d["slot"] = e.slot;
    d["word"] = e.word;
    d["got"] = e.got;
    d["want"] = e.want;
    d["again"] = e.again;
    d["hw_id"] = e.hw_id;
    d["xcc_id"] = e.xcc_id;
    recs.append(d);
  }
  o["errors"] = r.errors;
  o["bit_errors"] = r.bit_errors;
  o["transient"] = r.transient;
  o["persistent"] = r.persistent;
  o["records_dropped"] = r.records_dropped;
  o[records_key] = recs;
}

template <class T>
using array_in = py::array_t<T, py::array::c_style | py::array::forcecast>;
using bytes_in = array_in<uint8_t>;
template <class T>
static std::vector<T> to_vec(const array_in<T>& x) {
  return std::vector<T>(x.data(), x.data() + x.size());
}

// fn() with the GIL released
template <class F>
static auto nogil(F&& fn) {
  py::gil_scoped_release release;
  return fn();
}

// (A, B, C) of one workgroup of a matrix-core check
static py::tuple tile_tuple(const amdkube::MfmaCheckTile& t) {
  return py::make_tuple(py::array_t<float>({amdkube::MFMA_TILE, t.k}, t.a.data()),
                        py::array_t<float>({t.k, amdkube::MFMA_TILE}, t.b.data()),
                        py::array_t<float>({amdkube::MFMA_TILE, amdkube::MFMA_TILE}, t.c.data()));
}

PYBIND11_MODULE(_hipops, m) {
  m.doc() = "amdkube HIP (gfx950) validation kernels: vector add, HBM probe, HBM check, MFMA burn, MFMA check, CU check";
  m.def("device_count", []() {
    int n = 0;
    AK_HIP(hipGetDeviceCount(&n));
    return n;
  });
  m.def(
      "device_info",
      [](int dev) {
        amdkube::DevInfo d = amdkube::dev_info(dev);
        py::dict o;
        o["device"] = d.device;
        o["name"] = d.name;
        o["arch"] = d.arch;
        o["pci_bus_id"] = d.pci_bus_id;
        o["uuid"] = d.uuid;
        o["total_mem"] = d.total_mem;
        o["cu_count"] = d.cu_count;
        return o;
      },
      py::arg("device") = 0);
  m.def(
      "vector_add",
      [](size_t n, int dev) {
        const amdkube::VaddResult r = nogil([&] { return amdkube::run_vector_add(n, dev); });
        py::dict o;
        o["ok"] = r.ok;
        o["kernel_ms"] = r.kernel_ms;
        o["mismatches"] = r.mismatches;
        return o;
      },
      py::arg("n") = 50000, py::arg("device") = 0);
  m.def(
      "hbm_probe",
      [](size_t mib, int iters, int dev) {
        const amdkube::HbmResult r = nogil([&] { return amdkube::run_hbm_probe(mib << 20, iters, dev); });
        py::dict o;
        o["bytes"] = r.bytes;
        o["iters"] = r.iters;
        o["write_gbps"] = r.write_gbps;
        o["read_gbps"] = r.read_gbps;
        o["copy_gbps"] = r.copy_gbps;
        o["verify_gbps"] = r.verify_gbps;
        o["errors"] = r.errors;
        return o;
      },
      py::arg("mib") = 1024, py::arg("iters") = 5, py::arg("device") = 0);
  // caller-supplied data (numpy arrays, e.g. torch.Tensor.numpy()) → the same kernels
  m.def(
      "vector_add_arrays",
      [](array_in<float> a, array_in<float> b, int dev, int grid) {
        const std::vector<float> va = to_vec(a), vb = to_vec(b);
        const std::vector<float> vc = nogil([&] { return amdkube::vector_add_host(va, vb, dev, grid); });
        return py::array_t<float>(vc.size(), vc.data());
      },
      py::arg("a"), py::arg("b"), py::arg("device") = 0, py::arg("grid") = 0);
  // grid: workgroups to launch, 0 for the production grid (kernels/gpu_common.h, host_grid)
  m.def(
      "hbm_pattern",
      [](size_t n16, uint32_t seed, int dev, int grid) {
        const std::vector<uint32_t> w = nogil([&] { return amdkube::hbm_pattern_host(n16, seed, dev, grid); });
        return py::array_t<uint32_t>(w.size(), w.data());
      },
      py::arg("n16"), py::arg("seed") = 0x5eedu, py::arg("device") = 0, py::arg("grid") = 0);
  m.def(
      "hbm_verify_words",
      [](array_in<uint32_t> words, uint32_t seed, int dev, int grid) {
        const std::vector<uint32_t> w = to_vec(words);
        return nogil([&] { return amdkube::hbm_verify_host(w, seed, dev, grid); });
      },
      py::arg("words"), py::arg("seed") = 0x5eedu, py::arg("device") = 0, py::arg("grid") = 0);
  m.def(
      "hbm_read_words",
      [](array_in<uint32_t> words, int grid, int dev) {
        const std::vector<uint32_t> w = to_vec(words);
        return nogil([&] { return amdkube::hbm_read_host(w, grid, dev); });
      },
      py::arg("words"), py::arg("grid") = 0, py::arg("device") = 0);
  m.def(
      "hbm_copy_words",
      [](array_in<uint32_t> words, int dev, int grid) {
        const std::vector<uint32_t> w = to_vec(words);
        const std::vector<uint32_t> o = nogil([&] { return amdkube::hbm_copy_host(w, dev, grid); });
        return py::array_t<uint32_t>(o.size(), o.data());
      },
      py::arg("words"), py::arg("device") = 0, py::arg("grid") = 0);
  // hsa-vector-add's kernels, from the code object it embeds (co_path: amdkube/_native/lib/vadd_gfx950.co)
  m.def(
      "hsa_vadd_arrays",
      [](const std::string& co_path, array_in<float> a, array_in<float> b, int groups, int dev) {
        const std::vector<float> va = to_vec(a), vb = to_vec(b);
        const std::vector<float> vc = nogil([&] { return amdkube::co_vadd_host(co_path, va, vb, groups, dev); });
        return py::array_t<float>(vc.size(), vc.data());
      },
      py::arg("co_path"), py::arg("a"), py::arg("b"), py::arg("groups"), py::arg("device") = 0);
  m.def(
      "hsa_copy_array",
      [](const std::string& co_path, array_in<float> src, int groups, int dev) {
        const std::vector<float> vs = to_vec(src);
        const std::vector<float> vo = nogil([&] { return amdkube::co_copy_host(co_path, vs, groups, dev); });
        return py::array_t<float>(vo.size(), vo.data());
      },
      py::arg("co_path"), py::arg("src"), py::arg("groups"), py::arg("device") = 0);
  m.def(
      "mfma_tile",
      [](array_in<uint16_t> a_bits, array_in<uint16_t> b_bits, int k, int dev) {
        const std::vector<uint16_t> a = to_vec(a_bits), b = to_vec(b_bits);
        const std::vector<float> c = nogil([&] { return amdkube::mfma_tile_host(a, b, k, dev); });
        return py::array_t<float>({32, 32}, c.data());
      },
      py::arg("a_bits"), py::arg("b_bits"), py::arg("k"), py::arg("device") = 0);
  m.def(
      "mfma_gemm",
      [](array_in<uint16_t> a_bits, array_in<uint16_t> b_bits, int mm, int nn, int k, int dev) {
        const std::vector<uint16_t> a = to_vec(a_bits), b = to_vec(b_bits);
        const std::vector<float> c = nogil([&] { return amdkube::mfma_gemm_host(a, b, mm, nn, k, dev); });
        return py::array_t<float>({mm, nn}, c.data());
      },
      py::arg("a_bits"), py::arg("b_bits"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("device") = 0);
  m.def(
      "mfma_check",
      [](int rounds, double ms, int dev, uint32_t seed, int flips) {
        return check_result(nogil([&] { return amdkube::run_mfma_check(rounds, ms, dev, seed, flips); }), "bf16_tflops");
      },
      py::arg("rounds") = 0, py::arg("ms") = 50.0, py::arg("device") = 0, py::arg("seed") = 0x5eedu,
      py::arg("selftest_flips") = 0);
  m.def(
      "mfma_check_tile",
      [](int block, uint32_t seed, int dev) {
        return tile_tuple(nogil([&] { return amdkube::mfma_check_tile_host(block, seed, dev); }));
      },
      py::arg("block"), py::arg("seed") = 0x5eedu, py::arg("device") = 0);
  // the low-precision matrix-core paths (kernels/mfma_check_lp.h): dtype is fp8, mxfp8 or mxfp4
  m.def(
      "mfma_gemm_lp",
      [](const std::string& dtype, bytes_in a_codes, bytes_in b_codes, bytes_in a_scales, bytes_in b_scales, int mm, int nn,
         int k, int dev) {
        const int fmt = amdkube::mfma_lp_fmt(dtype);
        const std::vector<uint8_t> a = to_vec(a_codes), b = to_vec(b_codes), sa = to_vec(a_scales), sb = to_vec(b_scales);
        const std::vector<float> c = nogil([&] { return amdkube::mfma_gemm_lp_host(fmt, a, b, sa, sb, mm, nn, k, dev); });
        return py::array_t<float>({mm, nn}, c.data());
      },
      py::arg("dtype"), py::arg("a_codes"), py::arg("b_codes"), py::arg("a_scales"), py::arg("b_scales"), py::arg("m"),
      py::arg("n"), py::arg("k"), py::arg("device") = 0);
  m.def(
      "mfma_check_lp",
      [](const std::string& dtype, int rounds, double ms, int dev, uint32_t seed, int flips) {
        const int fmt = amdkube::mfma_lp_fmt(dtype);
        py::dict o = check_result(nogil([&] { return amdkube::run_mfma_check_lp(fmt, rounds, ms, dev, seed, flips); }), "tflops");
        o["dtype"] = dtype;
        return o;
      },
      py::arg("dtype"), py::arg("rounds") = 0, py::arg("ms") = 50.0, py::arg("device") = 0, py::arg("seed") = 0x5eedu,
      py::arg("selftest_flips") = 0);
  m.def(
      "mfma_check_lp_tile",
      [](const std::string& dtype, int block, uint32_t seed, int dev) {
        const int fmt = amdkube::mfma_lp_fmt(dtype);
        return tile_tuple(nogil([&] { return amdkube::mfma_check_lp_tile_host(fmt, block, seed, dev); }));
      },
      py::arg("dtype"), py::arg("block"), py::arg("seed") = 0x5eedu, py::arg("device") = 0);
  // the per-CU check (kernels/cu_check.h): units is a mask over lds = 1, valu = 2, trans = 4
  m.def(
      "cu_check",
      [](int rounds, double ms, int dev, uint32_t seed, int flips, int units) {
        return cu_check_result(nogil([&] { return amdkube::run_cu_check(rounds, ms, dev, seed, flips, units); }));
      },
      py::arg("rounds") = 0, py::arg("ms") = 50.0, py::arg("device") = 0, py::arg("seed") = 0x5eedu,
      py::arg("selftest_flips") = 0, py::arg("units") = 7);
  m.def(
      "cu_check_dump",
      [](int block, uint32_t seed, int dev) {
        const amdkube::CuCheckDump d = nogil([&] { return amdkube::cu_check_dump_host(block, seed, dev); });
        const py::ssize_t T = amdkube::CU_CHECK_THREADS;
        py::dict o;
        o["hw_id"] = d.hw_id;
        o["xcc_id"] = d.xcc_id;
        o["lds"] = py::array_t<uint32_t>(d.lds.size(), d.lds.data());
        o["valu_ops"] = py::array_t<uint32_t>({T, static_cast<py::ssize_t>(amdkube::CU_CHECK_VALU_OPS)}, d.valu_ops.data());
        o["valu_f32"] = py::array_t<float>({T, static_cast<py::ssize_t>(4)}, d.valu_f32.data());
        o["valu_f64"] = py::array_t<double>({T, static_cast<py::ssize_t>(3)}, d.valu_f64.data());
        o["valu_int"] = py::array_t<uint64_t>({T, static_cast<py::ssize_t>(4)},
                                              reinterpret_cast<const uint64_t*>(d.valu_int.data()));
        const std::vector<py::ssize_t> ts = {T, amdkube::CU_CHECK_TRANS_FUNCS, amdkube::CU_CHECK_TRANS_SETS};
        o["trans_in"] = py::array_t<float>(ts, d.trans_in.data());
        o["trans_out"] = py::array_t<float>(ts, d.trans_out.data());
        return o;
      },
      py::arg("block"), py::arg("seed") = 0x5eedu, py::arg("device") = 0);
  // the HBM march (kernels/hbm_check.h): mib == 0 and free_fraction == 0 mean "not given"
  m.def(
      "hbm_check",
      [](long long mib, double free_fraction, long long chunk_mib, int rounds, uint32_t seed, int flips, int hold_ms, int dev) {
        const amdkube::HbmCheckResult r =
            nogil([&] { return amdkube::run_hbm_check(mib, free_fraction, chunk_mib, rounds, seed, flips, hold_ms, dev); });
        py::dict o;
        py::list bad;
        for (const amdkube::HbmBadPage& b : r.bad_pages) {
          py::dict d;
          d["offset"] = b.offset;
          d["chunk"] = b.chunk;
          d["errors"] = b.errors;
          bad.append(d);
        }
        o["ok"] = r.errors == 0;
        o["bytes"] = r.bytes;
        o["chunks"] = r.chunks;
        o["rounds"] = r.rounds;
        o["hold_ms"] = r.hold_ms;
        o["ms"] = r.ms;
        o["alloc_ms"] = r.alloc_ms;
        o["march_gbps"] = r.march_gbps;
        hbm_check_counts(r, "first_errors", o);
        o["bad_pages"] = bad;
        o["bad_pages_total"] = r.bad_pages_total;
        return o;
      },
      py::arg("mib") = 1024, py::arg("free_fraction") = 0.0, py::arg("chunk_mib") = 1024, py::arg("rounds") = 1,
      py::arg("seed") = 0x5eedu, py::arg("selftest_flips") = 0, py::arg("hold_ms") = 0, py::arg("device") = 0);
  m.def(
      "hbm_march_pass",
      [](array_in<uint32_t> words, uint32_t seed, uint32_t inv, bool down, bool write, int dev, int grid) {
        const std::vector<uint32_t> w = to_vec(words);
        const amdkube::HbmMarchPassResult r = nogil([&] { return amdkube::hbm_march_pass_host(w, seed, inv, down, write, dev, grid); });
        py::dict o;
        o["words"] = py::array_t<uint32_t>(r.words.size(), r.words.data());
        o["page_errors"] = py::array_t<uint32_t>(r.page_errors.size(), r.page_errors.data());
        hbm_check_counts(r.counts, "records", o);
        return o;
      },
      py::arg("words"), py::arg("seed"), py::arg("inv"), py::arg("down"), py::arg("write"), py::arg("device") = 0,
      py::arg("grid") = 0);
  m.def(
      "mfma_burn",
      [](double ms, int dev) {
        const amdkube::BurnResult r = nogil([&] { return amdkube::run_mfma_burn(ms, dev); });
        py::dict o;
        o["ms"] = r.ms;
        o["iters"] = r.iters;
        o["blocks"] = r.blocks;
        o["bf16_tflops"] = r.tflops;
        return o;
      },
      py::arg("ms") = 100.0, py::arg("device") = 0);
}
