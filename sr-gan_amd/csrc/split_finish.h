// split_finish.h -- the ORDERED finish of a contraction whose K range is split over several workgroups.
//
// Until round 4 the K slices of a split launch met in the output through fp32 atomics (plus a zero-fill launch in front):
// the sum's order was the order in which the workgroups happened to arrive, two runs of one schedule differed at rounding
// level, and a pre-activation within rounding of zero then flipped its ReLU mask -- the gradient penalty of two runs moved
// by up to 6e-4 (profiles/r04h_*, gpurun_out/r5c: the drift disappears with every K split switched off).  The reference's
// CPU path is bitwise repeatable.
//
// Here every workgroup of an output tile leaves its partial accumulators in the caller's workspace (thread-linear layout:
// element i of thread t at [i * THREADS + t], so the stores and the later loads are coalesced and need no index math), waits
// until the stores are acknowledged, and takes a ticket of its tile; the workgroup that draws the LAST ticket re-reads all
// `splits` partials in slice order 0, 1, 2, ... and goes on to the kernel's ordinary epilogue with the total -- one launch,
// no zero-fill launch, no atomics on data, and the same bits on every run, whatever else is in flight.
//
// Memory model (gfx942 / gfx950, eight XCDs with an L2 each): the partials are written with agent-scope relaxed atomic
// stores (global_store_dword ... sc1: write-through) and read with agent-scope relaxed atomic loads (sc1); store and ticket
// live in different L2 channels, so the ticket's fetch_add must not be ISSUED before the stores are acknowledged:
// s_waitcnt vmcnt(0) in every thread, then the workgroup barrier, then thread 0 takes the ticket (ADVICE r4 on reduce.hip:
// a workgroup-scope release fence emits no instruction, the ISA had the atomic straight behind the store; stores count in
// vmcnt on gfx9).  Without the wait the last workgroup -- possibly on another XCD -- could draw the final ticket and still
// read the previous launch's partial.  No fences: these atomics act at the memory side and are coherent across the eight
// L2s by themselves, while a device-scope FENCE writes back / invalidates a whole L2 per workgroup (measured on the
// penalty's norms: 76 us for a 30 us reduction).  The tickets are device globals, one array per kernel family
// and one row per registered (device, stream) workspace -- launches on one stream are ordered, streams do not share a row --
// and the last workgroup puts its tile's ticket back to zero.
//
// Four device functions walk this protocol, and no kernel walks it by hand:
//   split_finish_ordered   many values per thread per output tile (the accumulators of a contraction split along K)
//   ordered_row_finish     a few scalars that thread 0 holds (parameter sums, loss sums), the legacy tree of block_sum_256
//   ordered_lane_finish    V values, thread i holds value i (per-channel sums / moments of a channel group), one barrier
//   counters_complete_after_adds   integer counters the workgroups add to with atomics: only the ticket, no partials
#pragma once
#include <map>
#include <mutex>
#include <utility>
#include "common.h"

namespace srgan {

constexpr int SPLIT_TICKET_SETS = 64;       // registered (device, stream) workspaces that can use the ordered finish
constexpr int SPLIT_TICKET_TILES = 2048;    // output tiles per launch (split launches are the FEW-tile launches)

// The middle of the protocol, called by ALL threads of a workgroup straight after their partial stores; true in the workgroup
// that drew the last of `parts` tickets (all its threads).
__device__ __forceinline__ bool last_ticket_after_stores(unsigned int* ticket, int parts) {
  __shared__ int drew_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every partial of this thread is acknowledged ...
  __syncthreads();                                          // ... and so is every thread's, before the ticket is taken
  if (threadIdx.x == 0) drew_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(parts - 1);
  __syncthreads();
  return drew_last;
}

// The meeting for INTEGER counters that the workgroups of a launch add to with agent-scope atomics: integer sums do not depend
// on the order, so there are no partials to keep and re-read, only the question of who is last.  Called by ALL threads of a
// workgroup straight after their atomic adds, in the RETURNING form with the values consumed (an add has been performed when
// its value is back, and s_waitcnt vmcnt(0) then covers it).  True in every thread of the workgroup that drew the last of
// `parts` tickets, the ticket already back at zero: the counters hold the totals, to be read with agent-scope atomic loads.
// parts == 1: true without a ticket (`ticket` may be NULL).
__device__ __forceinline__ bool counters_complete_after_adds(unsigned int* ticket, int parts) {
  if (parts == 1) {
    __syncthreads();
    return true;
  }
  if (!last_ticket_after_stores(ticket, parts)) return false;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// COUNT accumulator floats per thread, THREADS threads per workgroup.  `get(i)` / `set(i, v)` access accumulator i.
// `ws_tile` = this output tile's region of the workspace: [splits][COUNT * THREADS] floats.  Returns true in the
// workgroup that holds the tile's total afterwards (all its threads), false in the others (which are done).
template <int COUNT, int THREADS, typename Get, typename Set>
__device__ __forceinline__ bool split_finish_ordered(float* ws_tile, int split, int splits, unsigned int* ticket, Get get, Set set) {
  const int tid = (int)threadIdx.x;
  float* mine = ws_tile + (int64_t)split * (COUNT * THREADS) + tid;
#pragma unroll
  for (int i = 0; i < COUNT; ++i) __hip_atomic_store(mine + i * THREADS, get(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!last_ticket_after_stores(ticket, splits)) return false;
  // (slices outermost: the element loop unrolls completely -- the accumulators stay in registers -- and COUNT loads are in
  // flight per slice; every element is still summed in slice order 0, 1, 2, ...)
  const float* all = ws_tile + tid;
  float total[COUNT];
#pragma unroll
  for (int i = 0; i < COUNT; ++i) total[i] = __hip_atomic_load(all + i * THREADS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int s = 1; s < splits; ++s) {
    const float* slice = all + (int64_t)s * (COUNT * THREADS);
#pragma unroll
    for (int i = 0; i < COUNT; ++i) total[i] += __hip_atomic_load(slice + i * THREADS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int i = 0; i < COUNT; ++i) set(i, total[i]);
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// The same idea for a few SCALARS per workgroup that several workgroups add into one output row (the two parameter sums of
// a batch-norm backward per channel, a per-example loss sum).  Called by ALL 256 threads of the workgroup; thread 0 holds the
// workgroup's V values.  `partial_row` = the row's [parts][V] slots in the workspace, `ticket` = the row's ticket.  Returns true
// in thread 0 of the workgroup that drew the last ticket, with v = the sum over all parts: thread t adds the parts t, t + 256,
// ... and the 256 sums meet in the fixed tree of block_sum_256 -- the same order on every run, and no thread walks the parts
// alone (a single thread reading 768 parts one acknowledged load at a time cost 2 ms per launch).  The caller then adds v to
// the output: one adder per row and launch, no atomics on data.
template <int V>
__device__ __forceinline__ bool ordered_row_finish(float (&v)[V], float* partial_row, int part, int parts, unsigned int* ticket,
                                                   float* scratch4) {
  if (parts == 1) return threadIdx.x == 0;
  __shared__ int row_finish_last;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < V; ++i) __hip_atomic_store(partial_row + part * V + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    row_finish_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(parts - 1);
  }
  __syncthreads();
  if (!row_finish_last) return false;
  float mine[V];
#pragma unroll
  for (int i = 0; i < V; ++i) mine[i] = 0.f;
  for (int s = (int)threadIdx.x; s < parts; s += 256)
#pragma unroll
    for (int i = 0; i < V; ++i) mine[i] += __hip_atomic_load(partial_row + s * V + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    __syncthreads();                      // (scratch4 is reused)
    const float total = block_sum_256(mine[i], scratch4);
    if (threadIdx.x == 0) v[i] = total;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return threadIdx.x == 0;
}

// The same for V values of which thread i < V holds value i (the sums or moments of a channel group, one channel per
// thread), all V side by side: V barriers in a row in the last workgroup cost more than its loads.  Called by ALL 256 threads.
// Ops names the value type and its fixed trees: Value (a struct of floats, or float), combine(a, b), wave(v) -- the 64
// lanes' values, valid in lane 0 -- and four(w0, w1, w2, w3); Value{} is the neutral element.  LaneSums below is the plain
// fp32 sum, (w0 + w1) + (w2 + w3) over wave_sum -- NOT the tree of block_sum_256; bn_train.h has the one for Moments.
// `row` = the row's [parts][V] values in the workspace, `scratch` = [4][V] values of LDS that no thread still reads.
// Returns true in every thread of the workgroup that holds the totals afterwards (value i in thread i), false in the others:
// thread t combines the parts t, t + 256, ... of all V values (the V loads of a part in flight together), every value
// goes through one wave tree, and after ONE barrier thread i combines the four waves of value i.
struct LaneSums {
  using Value = float;
  static __device__ __forceinline__ float combine(float a, float b) { return a + b; }
  static __device__ __forceinline__ float wave(float v) { return wave_sum(v); }
  static __device__ __forceinline__ float four(float w0, float w1, float w2, float w3) { return (w0 + w1) + (w2 + w3); }
};

template <typename Ops, int V>
__device__ __forceinline__ bool ordered_lane_finish(typename Ops::Value& mine, float* row, int part, int parts, unsigned int* ticket,
                                                    typename Ops::Value (*scratch)[V]) {
  using Value = typename Ops::Value;
  constexpr int K = sizeof(Value) / sizeof(float);          // floats per value
  struct Words { float f[K]; };
  static_assert(sizeof(Words) == sizeof(Value), "a value is a whole number of floats");
  if (parts == 1) return true;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < V) {
    const Words w = __builtin_bit_cast(Words, mine);
#pragma unroll
    for (int k = 0; k < K; ++k) __hip_atomic_store(row + (part * V + tid) * K + k, w.f[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!last_ticket_after_stores(ticket, parts)) return false;
  Value total[V];
#pragma unroll
  for (int i = 0; i < V; ++i) total[i] = Value{};
  for (int s = tid; s < parts; s += 256) {
    Words theirs[V];
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
      for (int k = 0; k < K; ++k) theirs[i].f[k] = __hip_atomic_load(row + (s * V + i) * K + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int i = 0; i < V; ++i) total[i] = Ops::combine(total[i], __builtin_bit_cast(Value, theirs[i]));
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const Value w = Ops::wave(total[i]);
    if (lane == 0) scratch[wave][i] = w;
  }
  __syncthreads();
  if (tid < V) mine = Ops::four(scratch[0][tid], scratch[1][tid], scratch[2][tid], scratch[3][tid]);
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

constexpr int ROW_FINISH_ROWS = 4096;       // output rows (channels / examples) per launch that can use ordered_row_finish

// Host side: the workspace region and the ticket row of a split launch, or nullptr when the ordered finish cannot be used
// (no workspace registered for the stream, too many tiles / bytes, or SRGAN_ATOMIC_SPLIT=1: the round-4 atomics).
// (runtime.hip: the registry of caller-owned workspaces, one per device and stream; workspace_capacity() = the bytes
// srgan_set_workspace asks for)
float* partial_workspace(size_t bytes, hipStream_t stream);
int workspace_index(hipStream_t stream);
int workspace_register(float* ptr, size_t bytes, hipStream_t stream);
size_t workspace_capacity();

// The device address of a ticket array (per device: the symbol has one copy on each).  The cache is keyed by the SYMBOL'S
// ADDRESS, not by its type: several translation units declare arrays of one type (unsigned[64 * 2048]), and a cache per template
// instantiation handed whichever array was resolved first to all of them (benign while launches on a stream are
// ordered, wrong as a statement).  Guarded by a mutex: host threads may launch for the first time together.
template <typename Symbol>
inline unsigned int* device_tickets(const Symbol& symbol) {
  static std::mutex guard;
  static std::map<std::pair<const void*, int>, unsigned int*> cache;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(guard);
  const std::pair<const void*, int> key{static_cast<const void*>(&symbol), device};
  auto found = cache.find(key);
  if (found != cache.end()) return found->second;
  void* address = nullptr;
  if (hipGetSymbolAddress(&address, HIP_SYMBOL(symbol)) != hipSuccess) return nullptr;
  return cache[key] = static_cast<unsigned int*>(address);
}

inline bool split_atomics_forced() {
  static const bool forced = getenv("SRGAN_ATOMIC_SPLIT") != nullptr;
  return forced;
}

// `offset_bytes`: the part of the workspace the launch already uses for something else (packed weights).
inline float* split_workspace(int64_t tiles, int splits, int64_t floats_per_tile_and_split, size_t offset_bytes, hipStream_t stream,
                              int* ticket_set) {
  if (split_atomics_forced() || tiles > SPLIT_TICKET_TILES || splits < 2) return nullptr;
  const int set = workspace_index(stream);
  if (set < 0 || set >= SPLIT_TICKET_SETS) return nullptr;
  offset_bytes = (offset_bytes + 255) & ~(size_t)255;
  const size_t bytes = offset_bytes + (size_t)tiles * splits * floats_per_tile_and_split * sizeof(float);
  float* base = partial_workspace(bytes, stream);
  if (!base) return nullptr;
  *ticket_set = set;
  return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + offset_bytes);
}

// Host side of ordered_row_finish: the [rows][parts][V] region and the launch's ticket row (tickets: a device array of
// SPLIT_TICKET_SETS * ROW_FINISH_ROWS of the caller's translation unit), or nullptr (no workspace / too many rows / atomics forced).
template <typename Symbol>
inline float* row_finish_workspace(int64_t rows, int parts, int values, const Symbol& tickets, hipStream_t stream, unsigned int** ticket_row) {
  if (split_atomics_forced() || rows > ROW_FINISH_ROWS || parts < 1) return nullptr;
  const int set = workspace_index(stream);
  if (set < 0 || set >= SPLIT_TICKET_SETS) return nullptr;
  float* base = partial_workspace((size_t)rows * parts * values * sizeof(float), stream);
  unsigned int* all = base ? device_tickets(tickets) : nullptr;
  if (!base || !all) return nullptr;
  *ticket_row = all + (size_t)set * ROW_FINISH_ROWS;
  return base;
}

// The grid of a kernel whose workgroups own `per` of N images of one row each and meet through one of the two finishes above.
struct RowFinishGrid {
  int per = 1, parts = 1;                   // images per workgroup, workgroups per row (the grid's y)
  float* partial = nullptr;                 // [rows][parts][values] floats of the workspace, with the launch's ticket row
  unsigned int* tickets = nullptr;
};

// Fills in `parts`, `partial` and `tickets` for grid->per images per workgroup and `values` floats per part.  Without a
// workspace for the stream (or with the atomics forced) one workgroup takes the whole row: per = N, parts = 1.
template <typename Symbol>
inline int row_finish_grid(int64_t rows, int N, int values, const Symbol& tickets, hipStream_t stream, const char* what, RowFinishGrid* grid) {
  grid->parts = (N + grid->per - 1) / grid->per;
  grid->partial = grid->parts > 1 ? row_finish_workspace(rows, grid->parts, values, tickets, stream, &grid->tickets) : nullptr;
  if (!grid->partial) { grid->per = N; grid->parts = 1; }
  SRGAN_REQUIRE(grid->parts <= 65535, SRGAN_ERANGE, what);
  return SRGAN_OK;
}

}  // namespace srgan
