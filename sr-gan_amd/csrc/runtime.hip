// runtime.hip -- the library's process-wide host state: the thread-local error string, the registry of caller-owned workspaces
// (one per device and stream) and the capability report.  No kernel.
#include "common.h"
#include "split_finish.h"
#include <stdarg.h>
#include <string.h>
#include <map>
#include <mutex>
#include <utility>

namespace srgan {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

const char* last_error() { return g_error; }

// Partial sums that a second small kernel combines go through a workspace the CALLER owns (srgan_set_workspace: one
// block per (device, stream), at least srgan_workspace_bytes() long; launches on one stream are ordered, so reuse is
// safe): the K-slices of split-K launches with a tiny output (M*N < 512 outputs x at most 1024 slices x 4 B = 2 MiB) and
// the per-workgroup batch-norm parameter sums of the fused data-gradient epilogues (2 x column blocks x channels x 4 B =
// at most 1/32 of the gradient tensor's bytes: 64 MiB covers tensors of up to 2^29 elements; larger ones report "unsupported"
// from srgan_conv2d_bnrelu_supported and take the two-kernel form).  The library never allocates device memory.
constexpr size_t WORKSPACE_BYTES = (size_t)256 << 20;     // (round 5: 256 MiB -- the partial tiles of every K split / grouped weight gradient live here)
struct WorkspaceSlot { float* ptr = nullptr; size_t bytes = 0; int index = -1; };
static std::mutex g_workspace_mutex;
static std::map<std::pair<int, hipStream_t>, WorkspaceSlot> g_workspaces;
static int g_workspace_count[16] = {};        // ticket sets handed out, per device (the ticket arrays are per-device symbols)

// Unregistering (ptr == NULL) keeps the slot and its ticket-set index: a stream that registers again -- a caller that tears its
// workspace down between phases -- gets the SAME set back, so the 64 sets per device are not used up by re-registration (ADVICE
// r5: the index used to be re-drawn, and past 64 the ordered finish silently fell back to fp32 atomics).  A stream beyond the
// 64th of a device has index >= SPLIT_TICKET_SETS and srgan_split_is_ordered() reports 0 for it.
int workspace_register(float* ptr, size_t bytes, hipStream_t stream) {
  int device = 0;
  SRGAN_HIP(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_workspace_mutex);
  WorkspaceSlot& slot = g_workspaces[{device, stream}];
  slot.ptr = ptr; slot.bytes = ptr ? bytes : 0;
  if (slot.index < 0 && ptr != nullptr) slot.index = g_workspace_count[device & 15]++;
  return SRGAN_OK;
}

// A small integer per registered (device, stream): kernels that keep a few words of device-global state between the
// workgroups of ONE launch (reduce.hip's row tickets) index it by this, so that streams never share a set.
int workspace_index(hipStream_t stream) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return -1;
  std::lock_guard<std::mutex> lock(g_workspace_mutex);
  auto found = g_workspaces.find({device, stream});
  return (found == g_workspaces.end() || found->second.ptr == nullptr) ? -1 : found->second.index;
}

size_t workspace_capacity() { return WORKSPACE_BYTES; }

float* partial_workspace(size_t bytes, hipStream_t stream) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(g_workspace_mutex);
  auto found = g_workspaces.find({device, stream});
  if (found == g_workspaces.end() || found->second.ptr == nullptr || found->second.bytes < bytes) return nullptr;
  return found->second.ptr;
}

}  // namespace srgan

// ------------------------------------------------------------------------------------------- C ABI
using namespace srgan;

extern "C" {

const char* srgan_last_error(void) { return last_error(); }

int64_t srgan_workspace_bytes(void) { return (int64_t)WORKSPACE_BYTES; }

int srgan_set_workspace(void* workspace, int64_t bytes, void* stream) {
  SRGAN_REQUIRE(workspace == nullptr || bytes >= (int64_t)WORKSPACE_BYTES, SRGAN_EINVAL,
                "srgan_set_workspace: at least srgan_workspace_bytes() bytes");
  SRGAN_REQUIRE(((uintptr_t)workspace & 15) == 0, SRGAN_EINVAL, "srgan_set_workspace: 16-byte alignment");
  return workspace_register((float*)workspace, (size_t)(bytes > 0 ? bytes : 0), (hipStream_t)stream);
}

// 1 when a K split on this stream is finished in a fixed order through the registered workspace (split_finish.h): such a
// launch stores whole sums -- no zero-filled output needed, the same bits every run; 0: fp32 atomics into a zeroed output.
int srgan_split_is_ordered(void* stream) {
  if (split_atomics_forced()) return 0;
  const int set = workspace_index((hipStream_t)stream);
  return set >= 0 && set < SPLIT_TICKET_SETS ? 1 : 0;
}

int srgan_capabilities(srgan_capabilities_t* out, int32_t out_bytes) {
  SRGAN_REQUIRE(out != nullptr && out_bytes >= (int32_t)sizeof(srgan_capabilities_t), SRGAN_EINVAL,
                "srgan_capabilities: output struct");
  memset(out, 0, sizeof(*out));
  out->abi_version = srgan_version();
  out->struct_bytes = (int32_t)sizeof(*out);
  snprintf(out->arch, sizeof(out->arch), "gfx950");
  out->dtypes = SRGAN_DTYPE_F32 | SRGAN_DTYPE_BF16 | SRGAN_DTYPE_F16;
  out->features = SRGAN_FEATURE_FUSED_BNRELU | SRGAN_FEATURE_SPLITK_WORKSPACE | SRGAN_FEATURE_LIVE_PROFILE |
                  SRGAN_FEATURE_BLOCKED16 | SRGAN_FEATURE_BATCHED_SHADOWS | SRGAN_FEATURE_CROWD_FULL_IMAGE |
                  SRGAN_FEATURE_IMAGE_BATCHES | SRGAN_FEATURE_BATCH_NORM_TRAIN | SRGAN_FEATURE_BLOCKED_BATCH_NORM |
                  SRGAN_FEATURE_BLOCKED_FROZEN_NORM | SRGAN_FEATURE_DEVICE_DRAWS | SRGAN_FEATURE_IMAGE_SUMMARIES |
                  SRGAN_FEATURE_DISTRIBUTION_SUMMARIES | SRGAN_FEATURE_CONV3X3_WEIGHT_IMAGE |
                  SRGAN_FEATURE_DROPOUT | SRGAN_FEATURE_FEATURE_LOSSES | SRGAN_FEATURE_CROWD_EVALUATION |
                  SRGAN_FEATURE_SUMMARY_HISTOGRAM | SRGAN_FEATURE_REGRESSION_EVALUATION |
                  SRGAN_FEATURE_CROWD_PATCH_DRAWS | SRGAN_FEATURE_EPOCH_ORDER;
  out->workspace_bytes = (int64_t)WORKSPACE_BYTES;
  out->max_tensor_elements = ((int64_t)1 << 31) - 1;
  return SRGAN_OK;
}

}  // extern "C"
