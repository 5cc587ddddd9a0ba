// amd-smi shim: the MI355X-native replacement for the reference's NVML cgo binding
// (vendor/github.com/mindprince/gonvml/bindings.go:35-431: dlopen libnvidia-ml, device
// count / UUID / name / memory / utilization / power) and for what cAdvisor's accelerator
// collector reads through it (vendor/github.com/google/cadvisor/accelerators/nvidia.go).
//
// Exposed to Python with pybind11 as amdkube._native._amdsmi. Everything the device
// plugin, the exporter and the scheduler's topology scorer need comes from libamd_smi:
//   list_gpus()    identity + static attributes (uuid, bdf, kfd/render ids, gfx target,
//                  CUs, VRAM, NUMA node, xGMI hive, partition modes)
//   sample(i)      dynamic metrics (VRAM used, gfx/umc activity, power, temperature, ECC)
//   topology()     N x N link matrix {type, hops, weight, p2p}
//   link_metrics(i) per-link xGMI bit rate / bandwidth / read+write KB counters
//   processes(i)   per-process VRAM and engine time (container GPU accounting), meaningful
//                  where process_accounting() is true
//   start_sampler / average_activity / stop_sampler
//                  background gfx/umc activity sampling (native/sampler_core.h) and its mean
//                  over a window: gonvml AverageGPUUtilization (bindings.go:218-260), which
//                  cAdvisor reports as the 10 s DutyCycle (accelerators/nvidia.go:216-252)
// Every query is individually fault tolerant: an unsupported field is simply absent, so a
// partitioned or virtualised GPU still enumerates. The GIL is released around library
// calls (some sysfs-backed queries take milliseconds).
#include <amd_smi/amdsmi.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "sampler_core.h"

namespace py = pybind11;

namespace {

std::mutex g_mu;
bool g_inited = false;
std::vector<amdsmi_processor_handle> g_gpus;

std::string status_str(amdsmi_status_t s) {
  const char* msg = nullptr;
  if (amdsmi_status_code_to_string(s, &msg) == AMDSMI_STATUS_SUCCESS && msg) return msg;
  return "amdsmi status " + std::to_string(static_cast<int>(s));
}

void check(amdsmi_status_t s, const char* what) {
  if (s != AMDSMI_STATUS_SUCCESS) throw std::runtime_error(std::string(what) + ": " + status_str(s));
}

amdsmi_processor_handle gpu(size_t i) {
  if (!g_inited) throw std::runtime_error("amdsmi not initialised (call init())");
  if (i >= g_gpus.size()) throw std::out_of_range("gpu index out of range");
  return g_gpus[i];
}

std::string bdf_str(amdsmi_bdf_t b) {
  char buf[32];
  std::snprintf(buf, sizeof(buf), "%04llx:%02x:%02x.%x", static_cast<unsigned long long>(b.domain_number),
                static_cast<unsigned>(b.bus_number), static_cast<unsigned>(b.device_number),
                static_cast<unsigned>(b.function_number));
  return buf;
}

// KFD encodes gfx targets as major*10000 + minor*100 + stepping (90500 -> gfx950).
std::string gfx_name(uint64_t v) {
  if (v == 0 || v == 0xFFFFFFFFFFFFFFFFull) return "";
  char buf[32];
  if (v >= 10000) {
    std::snprintf(buf, sizeof(buf), "gfx%llu%llx%llx", static_cast<unsigned long long>(v / 10000),
                  static_cast<unsigned long long>((v / 100) % 100), static_cast<unsigned long long>(v % 100));
  } else {
    std::snprintf(buf, sizeof(buf), "gfx%llx", static_cast<unsigned long long>(v));
  }
  return buf;
}

void init(uint64_t flags) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_inited) return;
  amdsmi_status_t s;
  {
    py::gil_scoped_release nogil;
    s = amdsmi_init(flags);
  }
  check(s, "amdsmi_init");
  g_inited = true;
  g_gpus.clear();
  uint32_t nsock = 0;
  check(amdsmi_get_socket_handles(&nsock, nullptr), "amdsmi_get_socket_handles");
  std::vector<amdsmi_socket_handle> socks(nsock);
  check(amdsmi_get_socket_handles(&nsock, socks.data()), "amdsmi_get_socket_handles");
  for (auto sh : socks) {
    uint32_t np = 0;
    if (amdsmi_get_processor_handles(sh, &np, nullptr) != AMDSMI_STATUS_SUCCESS) continue;
    std::vector<amdsmi_processor_handle> ps(np);
    if (amdsmi_get_processor_handles(sh, &np, ps.data()) != AMDSMI_STATUS_SUCCESS) continue;
    for (auto p : ps) {
      processor_type_t t;
      if (amdsmi_get_processor_type(p, &t) == AMDSMI_STATUS_SUCCESS && t == AMDSMI_PROCESSOR_TYPE_AMD_GPU)
        g_gpus.push_back(p);
    }
  }
}

amdkube::ActivitySampler& sampler() {
  static amdkube::ActivitySampler s;
  return s;
}

void stop_sampler() {
  py::gil_scoped_release nogil;  // joins the sampler thread
  sampler().stop();
}

void shutdown() {
  stop_sampler();  // its thread calls into the library
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_inited) return;
  amdsmi_shut_down();
  g_inited = false;
  g_gpus.clear();
}

size_t count() {
  if (!g_inited) throw std::runtime_error("amdsmi not initialised (call init())");
  return g_gpus.size();
}

py::dict sample(size_t i);

py::dict describe(size_t i) {
  auto h = gpu(i);
  py::dict d;
  d["index"] = i;
  amdsmi_bdf_t bdf;
  std::string uuid;
  {
    char buf[AMDSMI_GPU_UUID_SIZE + 1] = {0};
    unsigned int len = AMDSMI_GPU_UUID_SIZE;
    if (amdsmi_get_gpu_device_uuid(h, &len, buf) == AMDSMI_STATUS_SUCCESS) uuid = buf;
  }
  d["uuid"] = uuid;
  if (amdsmi_get_gpu_device_bdf(h, &bdf) == AMDSMI_STATUS_SUCCESS) d["bdf"] = bdf_str(bdf);
  amdsmi_asic_info_t asic;
  std::memset(&asic, 0, sizeof(asic));
  if (amdsmi_get_gpu_asic_info(h, &asic) == AMDSMI_STATUS_SUCCESS) {
    d["market_name"] = std::string(asic.market_name);
    d["vendor_id"] = asic.vendor_id;
    d["device_id"] = asic.device_id;
    d["rev_id"] = asic.rev_id;
    d["serial"] = std::string(asic.asic_serial);
    if (asic.oam_id != 0xFFFFFFFFu) d["oam_id"] = asic.oam_id;
    if (asic.num_of_compute_units != 0xFFFFFFFFu) d["num_cu"] = asic.num_of_compute_units;
    std::string g = gfx_name(asic.target_graphics_version);
    if (!g.empty()) d["gfx_target"] = g;
  }
  amdsmi_board_info_t board;
  std::memset(&board, 0, sizeof(board));
  if (amdsmi_get_gpu_board_info(h, &board) == AMDSMI_STATUS_SUCCESS) {
    d["product_name"] = std::string(board.product_name);
    d["model_number"] = std::string(board.model_number);
  }
  amdsmi_enumeration_info_t en;
  std::memset(&en, 0, sizeof(en));
  if (amdsmi_get_gpu_enumeration_info(h, &en) == AMDSMI_STATUS_SUCCESS) {
    d["render_minor"] = en.drm_render;
    d["card_minor"] = en.drm_card;
    d["hsa_id"] = en.hsa_id;
    d["hip_id"] = en.hip_id;
    d["hip_uuid"] = std::string(en.hip_uuid);
  }
  amdsmi_kfd_info_t kfd;
  std::memset(&kfd, 0, sizeof(kfd));
  if (amdsmi_get_gpu_kfd_info(h, &kfd) == AMDSMI_STATUS_SUCCESS) {
    if (kfd.kfd_id != 0xFFFFFFFFFFFFFFFFull) d["kfd_id"] = kfd.kfd_id;
    if (kfd.node_id != 0xFFFFFFFFu) d["kfd_node_id"] = kfd.node_id;
    if (kfd.current_partition_id != 0xFFFFFFFFu) d["partition_id"] = kfd.current_partition_id;
  }
  uint64_t total = 0;
  if (amdsmi_get_gpu_memory_total(h, AMDSMI_MEM_TYPE_VRAM, &total) == AMDSMI_STATUS_SUCCESS) d["vram_total_bytes"] = total;
  uint32_t numa = 0;
  if (amdsmi_topo_get_numa_node_number(h, &numa) == AMDSMI_STATUS_SUCCESS) d["numa_node"] = numa;
  amdsmi_xgmi_info_t xg;
  std::memset(&xg, 0, sizeof(xg));
  if (amdsmi_get_xgmi_info(h, &xg) == AMDSMI_STATUS_SUCCESS) {
    d["xgmi_hive_id"] = xg.xgmi_hive_id;
    d["xgmi_node_id"] = xg.xgmi_node_id;
    d["xgmi_lanes"] = xg.xgmi_lanes;
  }
  char part[64] = {0};
  if (amdsmi_get_gpu_compute_partition(h, part, sizeof(part)) == AMDSMI_STATUS_SUCCESS) d["compute_partition"] = std::string(part);
  char mpart[64] = {0};
  if (amdsmi_get_gpu_memory_partition(h, mpart, sizeof(mpart)) == AMDSMI_STATUS_SUCCESS) d["memory_partition"] = std::string(mpart);
  d.attr("update")(sample(i));
  return d;
}

py::dict sample(size_t i) {
  auto h = gpu(i);
  py::dict d;
  uint64_t used = 0;
  amdsmi_engine_usage_t act;
  amdsmi_power_info_t pw;
  int64_t temp = 0, temp_mem = 0;
  amdsmi_error_count_t ec;
  amdsmi_status_t s_used, s_act, s_pw, s_t, s_tm, s_ec;
  {
    py::gil_scoped_release nogil;
    s_used = amdsmi_get_gpu_memory_usage(h, AMDSMI_MEM_TYPE_VRAM, &used);
    if (s_used != AMDSMI_STATUS_SUCCESS || used == 0) {
      // that query reads the driver's sysfs counter, and where the file is missing (a VM guest)
      // it succeeds with 0, which a GPU with a loaded driver never has in use: ask the DRM
      // device itself (whole MiB)
      amdsmi_vram_usage_t vu;
      std::memset(&vu, 0, sizeof(vu));
      if (amdsmi_get_gpu_vram_usage(h, &vu) == AMDSMI_STATUS_SUCCESS) {
        used = static_cast<uint64_t>(vu.vram_used) << 20;
        s_used = AMDSMI_STATUS_SUCCESS;
      }
    }
    std::memset(&act, 0, sizeof(act));
    s_act = amdsmi_get_gpu_activity(h, &act);
    std::memset(&pw, 0, sizeof(pw));
    s_pw = amdsmi_get_power_info(h, &pw);
    s_t = amdsmi_get_temp_metric(h, AMDSMI_TEMPERATURE_TYPE_HOTSPOT, AMDSMI_TEMP_CURRENT, &temp);
    s_tm = amdsmi_get_temp_metric(h, AMDSMI_TEMPERATURE_TYPE_VRAM, AMDSMI_TEMP_CURRENT, &temp_mem);
    std::memset(&ec, 0, sizeof(ec));
    s_ec = amdsmi_get_gpu_total_ecc_count(h, &ec);
  }
  if (s_used == AMDSMI_STATUS_SUCCESS) d["vram_used_bytes"] = used;
  if (s_act == AMDSMI_STATUS_SUCCESS) {
    if (act.gfx_activity != 0xFFFFFFFFu) d["gfx_activity"] = act.gfx_activity;
    if (act.umc_activity != 0xFFFFFFFFu) d["umc_activity"] = act.umc_activity;
    if (act.mm_activity != 0xFFFFFFFFu) d["mm_activity"] = act.mm_activity;
  }
  if (s_pw == AMDSMI_STATUS_SUCCESS) {
    uint32_t p = pw.current_socket_power != 0xFFFFFFFFu ? pw.current_socket_power : pw.average_socket_power;
    if (p != 0xFFFFFFFFu) d["power_watts"] = p;
    if (pw.power_limit != 0xFFFFFFFFu) d["power_limit_watts"] = pw.power_limit;
  }
  if (s_t == AMDSMI_STATUS_SUCCESS) d["temperature_c"] = temp;
  if (s_tm == AMDSMI_STATUS_SUCCESS) d["temperature_mem_c"] = temp_mem;
  if (s_ec == AMDSMI_STATUS_SUCCESS) {
    d["ecc_correctable"] = ec.correctable_count;
    d["ecc_uncorrectable"] = ec.uncorrectable_count;
    d["ecc_deferred"] = ec.deferred_count;
  }
  return d;
}

// RAS state beyond the ECC totals: xGMI error status and link state, retired/pending bad pages,
// the bad-page threshold and which blocks have ECC enabled. Each query's status is reported (`*_status`)
// so callers can tell "no errors" from "not supported here" or "needs root".
py::dict ras(size_t i) {
  auto h = gpu(i);
  py::dict d;
  amdsmi_xgmi_status_t xs = AMDSMI_XGMI_STATUS_NO_ERRORS;
  uint32_t nbad = 0, nres = 0, thr = 0;
  uint64_t ecc_mask = 0;
  std::vector<amdsmi_retired_page_record_t> recs;
  amdsmi_status_t s_x, s_b, s_r, s_t, s_e, s_bb = AMDSMI_STATUS_SUCCESS;
  amdsmi_error_count_t xe;
  amdsmi_status_t s_xe;
  amdsmi_xgmi_link_status_t xl;
  amdsmi_status_t s_xl;
  {
    py::gil_scoped_release nogil;
    s_x = amdsmi_gpu_xgmi_error_status(h, &xs);
    s_b = amdsmi_get_gpu_bad_page_info(h, &nbad, nullptr);
    if (s_b == AMDSMI_STATUS_SUCCESS && nbad > 0) {
      recs.resize(nbad);
      s_bb = amdsmi_get_gpu_bad_page_info(h, &nbad, recs.data());
      recs.resize(s_bb == AMDSMI_STATUS_SUCCESS ? nbad : 0);
    }
    s_r = amdsmi_get_gpu_memory_reserved_pages(h, &nres, nullptr);
    s_t = amdsmi_get_gpu_bad_page_threshold(h, &thr);
    s_e = amdsmi_get_gpu_ecc_enabled(h, &ecc_mask);
    std::memset(&xe, 0, sizeof(xe));
    s_xe = amdsmi_get_gpu_ecc_count(h, AMDSMI_GPU_BLOCK_XGMI_WAFL, &xe);
    std::memset(&xl, 0, sizeof(xl));
    s_xl = amdsmi_get_gpu_xgmi_link_status(h, &xl);
  }
  auto st = [](amdsmi_status_t s) {
    const char* msg = nullptr;
    amdsmi_status_code_to_string(s, &msg);
    return std::string(msg ? msg : "?");
  };
  d["xgmi_error_status"] = st(s_x);
  if (s_x == AMDSMI_STATUS_SUCCESS) d["xgmi_error"] = static_cast<int>(xs);
  d["bad_pages_status"] = st(s_b == AMDSMI_STATUS_SUCCESS ? s_bb : s_b);
  if (s_b == AMDSMI_STATUS_SUCCESS) {
    int reserved = 0, pending = 0, unreservable = 0;
    for (auto& r : recs) {
      if (r.status == AMDSMI_MEM_PAGE_STATUS_RESERVED) ++reserved;
      else if (r.status == AMDSMI_MEM_PAGE_STATUS_PENDING) ++pending;
      else ++unreservable;
    }
    d["bad_pages"] = nbad;
    d["bad_pages_retired"] = reserved;
    d["bad_pages_pending"] = pending;
    d["bad_pages_unreservable"] = unreservable;
  }
  d["reserved_pages_status"] = st(s_r);
  if (s_r == AMDSMI_STATUS_SUCCESS) d["reserved_pages"] = nres;
  d["bad_page_threshold_status"] = st(s_t);
  if (s_t == AMDSMI_STATUS_SUCCESS) d["bad_page_threshold"] = thr;
  d["ecc_enabled_status"] = st(s_e);
  if (s_e == AMDSMI_STATUS_SUCCESS) d["ecc_enabled_blocks"] = ecc_mask;
  d["xgmi_ecc_status"] = st(s_xe);
  if (s_xe == AMDSMI_STATUS_SUCCESS) {
    d["xgmi_ecc_correctable"] = xe.correctable_count;
    d["xgmi_ecc_uncorrectable"] = xe.uncorrectable_count;
  }
  // the per-link state of the GPU metrics table: it answers where the driver exposes neither RAS
  // file above (a VM guest with the GPU passed through)
  d["xgmi_links_status"] = st(s_xl);
  if (s_xl == AMDSMI_STATUS_SUCCESS) {
    int up = 0, down = 0;
    for (uint32_t k = 0; k < xl.total_links && k < AMDSMI_MAX_NUM_XGMI_LINKS; ++k) {
      if (xl.status[k] == AMDSMI_XGMI_LINK_UP) ++up;
      else if (xl.status[k] == AMDSMI_XGMI_LINK_DOWN) ++down;
    }
    d["xgmi_links_up"] = up;
    d["xgmi_links_down"] = down;
  }
  return d;
}

py::list list_gpus() {
  py::list out;
  for (size_t i = 0; i < count(); ++i) out.append(describe(i));
  return out;
}

const char* link_name(amdsmi_link_type_t t) {
  switch (t) {
    case AMDSMI_LINK_TYPE_INTERNAL: return "internal";
    case AMDSMI_LINK_TYPE_PCIE: return "pcie";
    case AMDSMI_LINK_TYPE_XGMI: return "xgmi";
    case AMDSMI_LINK_TYPE_NOT_APPLICABLE: return "n/a";
    default: return "unknown";
  }
}

py::list topology() {
  size_t n = count();
  py::list rows;
  for (size_t i = 0; i < n; ++i) {
    py::list row;
    for (size_t j = 0; j < n; ++j) {
      py::dict e;
      if (i == j) {
        e["type"] = "self";
        e["hops"] = 0;
        e["weight"] = 0;
        e["p2p"] = true;
      } else {
        uint64_t hops = 0, weight = 0;
        amdsmi_link_type_t t = AMDSMI_LINK_TYPE_UNKNOWN;
        bool p2p = false;
        if (amdsmi_topo_get_link_type(g_gpus[i], g_gpus[j], &hops, &t) == AMDSMI_STATUS_SUCCESS) {
          e["type"] = link_name(t);
          e["hops"] = hops;
        } else {
          e["type"] = "unknown";
        }
        if (amdsmi_topo_get_link_weight(g_gpus[i], g_gpus[j], &weight) == AMDSMI_STATUS_SUCCESS) e["weight"] = weight;
        uint64_t bw_min = 0, bw_max = 0;   // the driver's xGMI link limits (1-hop xGMI pairs only)
        if (amdsmi_get_minmax_bandwidth_between_processors(g_gpus[i], g_gpus[j], &bw_min, &bw_max) ==
                AMDSMI_STATUS_SUCCESS && bw_max > 0) {
          e["min_bw_mbps"] = bw_min;
          e["max_bw_mbps"] = bw_max;
        }
        if (amdsmi_is_P2P_accessible(g_gpus[i], g_gpus[j], &p2p) == AMDSMI_STATUS_SUCCESS) e["p2p"] = p2p;
      }
      row.append(e);
    }
    rows.append(row);
  }
  return rows;
}

py::list link_metrics(size_t i) {
  auto h = gpu(i);
  amdsmi_link_metrics_t lm;
  std::memset(&lm, 0, sizeof(lm));
  py::list out;
  if (amdsmi_get_link_metrics(h, &lm) != AMDSMI_STATUS_SUCCESS) return out;
  for (uint32_t k = 0; k < lm.num_links && k < AMDSMI_MAX_NUM_XGMI_PHYSICAL_LINK; ++k) {
    py::dict e;
    e["peer_bdf"] = bdf_str(lm.links[k].bdf);
    e["bit_rate_gbps"] = lm.links[k].bit_rate;
    e["max_bandwidth_gbps"] = lm.links[k].max_bandwidth;
    e["type"] = link_name(lm.links[k].link_type);
    e["read_kb"] = lm.links[k].read;
    e["write_kb"] = lm.links[k].write;
    out.append(e);
  }
  return out;
}

// amd-smi builds its process list from KFD's per-process directory. A driver that does not expose
// it (a VM guest) makes every list come back empty with SUCCESS, which is not "no process holds
// memory": callers ask here first whether the list means anything.
bool process_accounting() {
  struct stat st;
  return stat("/sys/class/kfd/kfd/proc", &st) == 0 && S_ISDIR(st.st_mode);
}

py::list processes(size_t i) {
  auto h = gpu(i);
  uint32_t n = 0;
  py::list out;
  if (amdsmi_get_gpu_process_list(h, &n, nullptr) != AMDSMI_STATUS_SUCCESS || n == 0) return out;
  std::vector<amdsmi_proc_info_t> procs(n);
  if (amdsmi_get_gpu_process_list(h, &n, procs.data()) != AMDSMI_STATUS_SUCCESS) return out;
  for (uint32_t k = 0; k < n; ++k) {
    py::dict e;
    e["pid"] = procs[k].pid;
    e["name"] = std::string(procs[k].name);
    e["vram_bytes"] = procs[k].memory_usage.vram_mem;
    e["gfx_ns"] = procs[k].engine_usage.gfx;
    e["cu_occupancy"] = procs[k].cu_occupancy;
    out.append(e);
  }
  return out;
}

// Starts (or restarts) the background sampler over every enumerated GPU.
void start_sampler(double period_ms, size_t capacity) {
  if (!g_inited) throw std::runtime_error("amdsmi not initialised (call init())");
  if (!(period_ms > 0)) throw std::invalid_argument("period_ms must be > 0");
  std::vector<amdsmi_processor_handle> handles = g_gpus;  // the thread owns its copy
  auto src = [handles](size_t d, amdkube::ActivitySample* out) {
    amdsmi_engine_usage_t act;
    std::memset(&act, 0, sizeof(act));
    if (amdsmi_get_gpu_activity(handles[d], &act) != AMDSMI_STATUS_SUCCESS || act.gfx_activity == 0xFFFFFFFFu) return false;
    out->gfx = act.gfx_activity;
    if (act.umc_activity != 0xFFFFFFFFu) {
      out->umc = act.umc_activity;
      out->has_umc = true;
    }
    return true;
  };
  py::gil_scoped_release nogil;
  sampler().start(handles.size(), src, static_cast<int64_t>(period_ms * 1e6), capacity);
}

// Mean activity of GPU i over the last window_s seconds; None when no sample falls inside.
py::object average_activity(size_t i, double window_s) {
  gpu(i);
  const int64_t since = amdkube::steady_now_ns() - static_cast<int64_t>(window_s * 1e9);
  auto a = sampler().average(i, since);
  if (a.samples == 0) return py::none();
  py::dict d;
  d["gfx_activity"] = a.gfx;
  if (a.umc_samples) d["umc_activity"] = a.umc;
  d["samples"] = a.samples;
  d["span_s"] = static_cast<double>(a.last_ns - a.first_ns) / 1e9;
  return d;
}

py::dict sampler_state() {
  py::dict d;
  d["running"] = sampler().running();
  d["ticks"] = sampler().ticks();
  d["devices"] = sampler().devices();
  return d;
}

}  // namespace

PYBIND11_MODULE(_amdsmi, m) {
  m.doc() = "amd-smi shim for amdkube (MI355X device discovery, health, topology, metrics)";
  m.def("init", &init, py::arg("flags") = static_cast<uint64_t>(AMDSMI_INIT_AMD_GPUS));
  m.def("shutdown", &shutdown);
  m.def("count", &count);
  m.def("describe", &describe);
  m.def("list_gpus", &list_gpus);
  m.def("sample", &sample);
  m.def("ras", &ras);
  m.def("topology", &topology);
  m.def("link_metrics", &link_metrics);
  m.def("processes", &processes);
  m.def("process_accounting", &process_accounting);
  m.def("start_sampler", &start_sampler, py::arg("period_ms") = 100.0, py::arg("capacity") = 1024);
  m.def("stop_sampler", &stop_sampler);
  m.def("average_activity", &average_activity, py::arg("index"), py::arg("window_s") = 10.0);
  m.def("sampler_state", &sampler_state);
}
