// epoch_order.hip -- the epoch order of the resident image loaders (age, driving: data.py ResidentImageLoader) drawn ON the
// device.  Frame i of epoch e owns the 64-bit key (w1 << 32) | w0 of Philox block i of the loader's draw, with
// the EPOCH in the counter's iteration word; the order is the stable argsort of the keys.  The stream is defined in
// include/srgan_hip.h (srgan_epoch_order).
//
// One launch ranks all n keys: a workgroup owns 256 frames (one per thread) and walks ALL n keys in LDS tiles that its threads
// compute (or load: srgan_argsort_u64, the same body over keys in memory); a thread counts the keys that sort in front of its
// own -- smaller, or equal with a lower index -- and stores order[rank] = its frame.  The ranks of n keys under a total order
// are a permutation of 0 .. n - 1, so every slot is written exactly once: no atomics, no workspace, no keys buffer, the same
// bits on every call.  O(n^2) comparisons: fine for a database of some 10^4 frames once per epoch, capped at
// SRGAN_EPOCH_ORDER_MAX.
//
// The inner loop reads tile[j] at a wave-uniform address: an LDS broadcast (one ds_read_b128 = two keys for all 64 lanes, no
// bank conflict), and per key one 64-bit compare and one add.  The tie rule costs nothing there: a tile that lies wholly in
// front of the workgroup's frames counts `<=`, a tile wholly behind them `<`, and only the one tile that holds the workgroup's
// own frames compares indices (TILE is a multiple of 256, so those frames sit in one tile).
#include "common.h"
#include "philox.h"

namespace srgan {
namespace {

constexpr int ORDER_THREADS = 256;
constexpr int ORDER_TILE = 2048;      // keys per LDS tile: 16 KiB, a multiple of ORDER_THREADS
constexpr int ORDER_UNROLL = 8;       // the inner loop's step; a partial tile is padded to it with keys that never count

struct PhiloxKeys {                   // key i = (w1 << 32) | w0 of block i of `draw` in "iteration" `epoch`
  uint32_t draw, epoch, seed_lo, seed_hi;
  __device__ __forceinline__ uint64_t operator()(int i) const {
    uint32_t w[4];
    draw_block_words((uint64_t)i, draw, epoch, seed_lo, seed_hi, w);
    return ((uint64_t)w[1] << 32) | w[0];
  }
};

struct StoredKeys {
  const uint64_t* keys;
  __device__ __forceinline__ uint64_t operator()(int i) const { return keys[i]; }
};

enum { TILE_BEFORE, TILE_OWN, TILE_AFTER };

// The keys of tile[0 .. count) that sort in front of (own, i); `count` is a multiple of ORDER_UNROLL.
template <int WHERE>
__device__ __forceinline__ int count_in_front(const uint64_t* tile, int count, int base, uint64_t own, int i) {
  int rank = 0;
  for (int j = 0; j < count; j += ORDER_UNROLL) {
#pragma unroll
    for (int u = 0; u < ORDER_UNROLL; ++u) {
      const uint64_t k = tile[j + u];
      if (WHERE == TILE_BEFORE) rank += (k <= own) ? 1 : 0;
      else if (WHERE == TILE_AFTER) rank += (k < own) ? 1 : 0;
      else rank += (k < own || (k == own && base + j + u < i)) ? 1 : 0;
    }
  }
  return rank;
}

template <typename Keys>
__device__ __forceinline__ void rank_and_store(const Keys& key, int n, int32_t* __restrict__ order) {
  __shared__ __attribute__((aligned(16))) uint64_t tile[ORDER_TILE];
  const int first = (int)blockIdx.x * ORDER_THREADS;         // the workgroup's frames: [first, first + 256)
  const int i = first + (int)threadIdx.x;
  const uint64_t own = i < n ? key(i) : 0;
  int rank = 0;
  for (int base = 0; base < n; base += ORDER_TILE) {
    const int count = min(ORDER_TILE, n - base);
    const int padded = (count + ORDER_UNROLL - 1) / ORDER_UNROLL * ORDER_UNROLL;      // <= ORDER_TILE
    __syncthreads();                                         // the previous tile has been read by every wave
    for (int j = (int)threadIdx.x; j < padded; j += ORDER_THREADS)
      tile[j] = j < count ? key(base + j) : ~(uint64_t)0;    // padding: index >= n > i and never < own, so it never counts
    __syncthreads();
    if (base + ORDER_TILE <= first) rank += count_in_front<TILE_BEFORE>(tile, padded, base, own, i);       // (a full tile)
    else if (base >= first + ORDER_THREADS) rank += count_in_front<TILE_AFTER>(tile, padded, base, own, i);
    else rank += count_in_front<TILE_OWN>(tile, padded, base, own, i);
  }
  if (i < n) order[rank] = i;                                // rank < n: at most the n - 1 other keys sort in front
}

__global__ __launch_bounds__(ORDER_THREADS) void epoch_order_kernel(int n, uint32_t batches, int conditional, uint32_t draw,
                                                                    const uint32_t* __restrict__ state,
                                                                    int32_t* __restrict__ order) {
  const uint32_t t = state[2];
  if (conditional && t % batches != 0) return;               // uniform over the grid: not an epoch start, nothing is touched
  rank_and_store(PhiloxKeys{draw, t / batches, state[0], state[1]}, n, order);
}

__global__ __launch_bounds__(ORDER_THREADS) void argsort_u64_kernel(const uint64_t* __restrict__ keys, int n,
                                                                    int32_t* __restrict__ order) {
  rank_and_store(StoredKeys{keys}, n, order);
}

// One thread per row of the window [first_row, first_row + rows) of batch t % batches.
__global__ __launch_bounds__(256) void epoch_batch_indices_kernel(const int32_t* __restrict__ order, int B_global,
                                                                  uint32_t batches, int first_row, int rows,
                                                                  const uint32_t* __restrict__ state,
                                                                  int32_t* __restrict__ table) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= rows) return;
  table[i] = order[(int)(state[2] % batches) * B_global + first_row + i];      // < batches * B_global <= n
}

}  // namespace
}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_epoch_order(int32_t n, int32_t batches, int32_t conditional, int32_t draw, const uint32_t* state, int32_t* order,
                      void* stream) {
  SRGAN_REQUIRE(state && order, SRGAN_EINVAL, "srgan_epoch_order pointers");
  SRGAN_REQUIRE(n >= 1 && batches >= 1 && draw >= 0 && (conditional == 0 || conditional == 1), SRGAN_EINVAL,
                "srgan_epoch_order: n, batches, draw, conditional");
  SRGAN_REQUIRE(n <= SRGAN_EPOCH_ORDER_MAX, SRGAN_ERANGE, "srgan_epoch_order: n above SRGAN_EPOCH_ORDER_MAX");
  hipLaunchKernelGGL(epoch_order_kernel, dim3((n + ORDER_THREADS - 1) / ORDER_THREADS), dim3(ORDER_THREADS), 0,
                     (hipStream_t)stream, (int)n, (uint32_t)batches, (int)conditional, (uint32_t)draw, state, order);
  return launch_status();
}

int srgan_argsort_u64(const uint64_t* keys, int32_t n, int32_t* order, void* stream) {
  SRGAN_REQUIRE(keys && order, SRGAN_EINVAL, "srgan_argsort_u64 pointers");
  SRGAN_REQUIRE(n >= 1, SRGAN_EINVAL, "srgan_argsort_u64: n");
  SRGAN_REQUIRE(n <= SRGAN_EPOCH_ORDER_MAX, SRGAN_ERANGE, "srgan_argsort_u64: n above SRGAN_EPOCH_ORDER_MAX");
  hipLaunchKernelGGL(argsort_u64_kernel, dim3((n + ORDER_THREADS - 1) / ORDER_THREADS), dim3(ORDER_THREADS), 0,
                     (hipStream_t)stream, keys, (int)n, order);
  return launch_status();
}

int srgan_epoch_batch_indices(const int32_t* order, int32_t n, int32_t B_global, int32_t batches, int32_t first_row,
                              int32_t rows, const uint32_t* state, int32_t* table, void* stream) {
  SRGAN_REQUIRE(order && state && table, SRGAN_EINVAL, "srgan_epoch_batch_indices pointers");
  SRGAN_REQUIRE(n >= 1 && B_global >= 1 && batches >= 1 && (int64_t)batches * B_global <= n, SRGAN_EINVAL,
                "srgan_epoch_batch_indices: n, B_global, batches");
  SRGAN_REQUIRE(rows >= 0 && first_row >= 0 && (int64_t)first_row + rows <= B_global, SRGAN_EINVAL,
                "srgan_epoch_batch_indices: the window [first_row, first_row + rows) of the global batch");
  SRGAN_REQUIRE(n <= SRGAN_EPOCH_ORDER_MAX, SRGAN_ERANGE, "srgan_epoch_batch_indices: n above SRGAN_EPOCH_ORDER_MAX");
  if (rows == 0) return SRGAN_OK;
  hipLaunchKernelGGL(epoch_batch_indices_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, order,
                     (int)B_global, (uint32_t)batches, (int)first_row, (int)rows, state, table);
  return launch_status();
}

}  // extern "C"
