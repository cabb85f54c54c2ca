// profile.hip -- optional live timing of every contraction launch with HIP events on the launch stream: the bracket the
// launchers put around their kernels, the srgan_profile_* entry points and the per-shape text report.  No kernel.
// (bench.py: roofline.achieved = sum of logical 2*M*N*K over launches / sum of their event-timed durations)
#include "common.h"
#include "launchers.h"
#include <string.h>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace srgan {

struct ProfileRecord { int32_t M, N, K, kind, bm, bn, split, akf, bkf; double bytes; int32_t precision; };
// Algorithmic HBM bytes of one contraction launch: every operand element once, 4 B each.  `taps` = how many times the
// gather visits one element of the big operand (9 for a 3x3 kernel, R*S of a strided one divided over its classes).
static double algorithmic_bytes(double M, double N, double K, LaunchKind kind) {
  if (kind == KIND_CONV3X3_LDS) return 4.0 * (M * N + M * K + (K / 9.0) * N);     // K = CI * 9 taps over one input plane
  if (kind == KIND_CONV3X3_WGRAD) return 4.0 * (M * N + M * K + (N / 9.0) * K);   // N = CI * 9
  return 4.0 * (M * N + M * K + K * N);
}
struct ProfileState {
  std::atomic<bool> enabled{false};
  std::mutex mutex;                   // guards every other member (launches may come from several host threads)
  std::vector<hipEvent_t> events;     // two per slot: start, stop
  std::vector<ProfileRecord> records; // one per slot (M < 0: begun, not ended)
  size_t slots = 0;
  double flops = 0.0, mfma_flops = 0.0, bytes = 0.0;
  int64_t launches = 0;
};
static ProfileState g_profile;

// Event bracket around one contraction launch (called from the launchers' translation units).  begin() reserves a slot
// and records its start event on the launch stream; returns -1 when profiling is off.
int profile_bracket_begin(hipStream_t stream) {
  if (!g_profile.enabled.load(std::memory_order_acquire)) return -1;
  hipEvent_t start;
  int slot;
  {
    std::lock_guard<std::mutex> lock(g_profile.mutex);
    slot = (int)g_profile.slots++;
    while (g_profile.events.size() < 2 * g_profile.slots) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) { --g_profile.slots; return -1; }
      g_profile.events.push_back(e);
    }
    g_profile.records.resize(g_profile.slots, ProfileRecord{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0});
    start = g_profile.events[2 * slot];
  }
  if (hipEventRecord(start, stream) != hipSuccess) return -1;
  return slot;
}

// Both bracket ends: files the record, adds its 2 M N K to the totals (`mfma`: also to the MFMA FLOPs) and records the stop event.
static int bracket_end(int slot, hipStream_t stream, const ProfileRecord& record, bool mfma) {
  if (slot < 0) return SRGAN_OK;
  hipEvent_t stop;
  {
    std::lock_guard<std::mutex> lock(g_profile.mutex);
    if ((size_t)slot >= g_profile.slots) return SRGAN_OK;          // the region was closed in between
    stop = g_profile.events[2 * slot + 1];
    const double f = 2.0 * (double)record.M * (double)record.N * (double)record.K;
    g_profile.records[slot] = record;
    g_profile.flops += f;
    if (mfma) g_profile.mfma_flops += f;
    g_profile.bytes += record.bytes;
    g_profile.launches += 1;
  }
  SRGAN_HIP(hipEventRecord(stop, stream));
  return SRGAN_OK;
}

int profile_bracket_end(int slot, hipStream_t stream, int64_t M, int64_t N, int64_t K, LaunchKind kind, int bm, int bn, int split,
                        int akf, int bkf, int64_t b_unique, int precision) {
  const double bytes = b_unique > 0 ? 4.0 * ((double)M * N + (double)M * K + (double)b_unique)
                                    : algorithmic_bytes((double)M, (double)N, (double)K, kind);
  return bracket_end(slot, stream, ProfileRecord{(int32_t)M, (int32_t)N, (int32_t)K, (int32_t)kind, bm, bn, split, akf, bkf, bytes, precision},
                     !launch_kind_is_valu(kind));
}

// The same bracket end for a launch that states its own algorithmic bytes (the 16-bit kernels of blocked16*.hip and the
// batch-norm kernels).
int profile_bracket_end_bytes(int slot, hipStream_t stream, int64_t M, int64_t N, int64_t K, LaunchKind kind, int bm, int bn, int split,
                              double bytes, int precision) {
  return bracket_end(slot, stream, ProfileRecord{(int32_t)M, (int32_t)N, (int32_t)K, (int32_t)kind, bm, bn, split, 0, 0, bytes, precision}, true);
}

}  // namespace srgan

// ------------------------------------------------------------------------------------------- C ABI
using namespace srgan;

extern "C" {

int srgan_profile_begin(void) {
  std::lock_guard<std::mutex> lock(g_profile.mutex);
  g_profile.slots = 0;
  g_profile.records.clear();
  g_profile.flops = g_profile.mfma_flops = g_profile.bytes = 0.0;
  g_profile.launches = 0;
  g_profile.enabled.store(true, std::memory_order_release);
  return SRGAN_OK;
}

int srgan_profile_end(double* kernel_ms, double* flops, double* mfma_flops, int64_t* launches) {
  g_profile.enabled.store(false, std::memory_order_release);
  std::lock_guard<std::mutex> lock(g_profile.mutex);
  double total = 0.0;
  for (size_t i = 0; i < g_profile.slots; ++i) {
    if (g_profile.records[i].M < 0) continue;
    SRGAN_HIP(hipEventSynchronize(g_profile.events[2 * i + 1]));
    float ms = 0.f;
    SRGAN_HIP(hipEventElapsedTime(&ms, g_profile.events[2 * i], g_profile.events[2 * i + 1]));
    total += ms;
  }
  if (kernel_ms) *kernel_ms = total;
  if (flops) *flops = g_profile.flops;
  if (mfma_flops) *mfma_flops = g_profile.mfma_flops;
  if (launches) *launches = g_profile.launches;
  return SRGAN_OK;
}

int srgan_profile_bytes(double* algorithmic_bytes_total) {
  std::lock_guard<std::mutex> lock(g_profile.mutex);
  if (algorithmic_bytes_total) *algorithmic_bytes_total = g_profile.bytes;
  return SRGAN_OK;
}

// The part of the profiled region that ran with bf16 / fp16 MFMA operands: its logical FLOPs and its summed kernel time.
int srgan_profile_mixed(double* flops, double* kernel_ms) {
  std::lock_guard<std::mutex> lock(g_profile.mutex);
  double f = 0.0, total = 0.0;
  for (size_t i = 0; i < g_profile.slots; ++i) {
    const ProfileRecord& r = g_profile.records[i];
    if (r.M < 0 || r.precision == 0) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_profile.events[2 * i], g_profile.events[2 * i + 1]) != hipSuccess) continue;
    total += ms;
    f += 2.0 * (double)r.M * (double)r.N * (double)r.K;
  }
  if (flops) *flops = f;
  if (kernel_ms) *kernel_ms = total;
  return SRGAN_OK;
}

// Per-shape breakdown of the last profiled region as text lines "M N K kind bm bn split akf bkf count ms bytes" (kind: the
// numbers of LaunchKind in launchers.h -- 0 gg_direct, 1 gg_mfma, 2 conv3x3_lds, 3 pointwise, 4 conv3x3_wgrad, 5 gg_rows,
// 6 pointwise_wgrad, 8 pointwise_ksplit, 9 gg_dot, 10 stem7x7_fwd, 11 stem7x7_wgrad, 12 stem7x7_bwd_data, 13 pointwise_ring,
// 14 hconv3x3, 15 hwgrad3x3, 16 hgemm, 17 hlinear_wgrad, 18 hconv4x4s2, 19 hwgrad4x4s2, 20 bn_stats, 21 bn_fwd, 22 bn_bwd_reduce,
// 23 bn_bwd_apply, 24 h_frozen_norm_bwd; bytes = algorithmic HBM bytes of all `count` launches; call after srgan_profile_end).
// Returns the number of bytes needed.
int64_t srgan_profile_report(char* buffer, int64_t capacity) {
  struct Key { int32_t v[9]; bool operator<(const Key& o) const { return memcmp(v, o.v, sizeof(v)) < 0; } };
  struct Acc { int64_t count = 0; double ms = 0.0, bytes = 0.0; };
  std::map<Key, Acc> table;
  std::lock_guard<std::mutex> lock(g_profile.mutex);
  for (size_t i = 0; i < g_profile.slots; ++i) {
    const ProfileRecord& r = g_profile.records[i];
    if (r.M < 0) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_profile.events[2 * i], g_profile.events[2 * i + 1]) != hipSuccess) continue;
    Key k{{r.M, r.N, r.K, r.kind, r.bm, r.bn, r.split, r.akf, r.bkf}};
    Acc& a = table[k];
    a.count += 1;
    a.ms += ms;
    a.bytes += r.bytes;
  }
  std::string out;
  char line[200];
  for (const auto& kv : table) {
    const int32_t* v = kv.first.v;
    snprintf(line, sizeof(line), "%d %d %d %d %d %d %d %d %d %lld %.4f %.0f\n", v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7],
             v[8], (long long)kv.second.count, kv.second.ms, kv.second.bytes);
    out += line;
  }
  if (buffer && capacity > 0) {
    const size_t n = out.size() < (size_t)capacity - 1 ? out.size() : (size_t)capacity - 1;
    memcpy(buffer, out.data(), n);
    buffer[n] = 0;
  }
  return (int64_t)out.size() + 1;
}

}  // extern "C"
