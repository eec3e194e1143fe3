// CDNA4 (gfx950 / MI355X) kernels for the columnar keyed-stream fast path.
//
// Replaces the per-item Python/Rust hot loops of the reference
// (reference src/operators.rs stateful_batch + windowing.py fold logic)
// with single-pass device kernels over columnar event batches:
//
//   * k_window_agg_insert: fused {window-id computation, open-address
//     hash insert into HBM-resident keyed window state, watermark
//     (max-timestamp) tracking} — one read of the event batch.
//   * k_close_extract: scan the table, emit (key, window, value)
//     triples for windows below the close horizon, compacted via
//     wave-ballot + one atomic per wave.
//   * k_bucket_hist / k_bucket_scatter: key-hash bucketing producing
//     per-destination contiguous segments for the RCCL all-to-allv
//     exchange across workers-as-GPUs.
//
// Design notes (see /opt/skills/guides/cdna_hip_programming.md):
//   - wave width 64 everywhere; ballots are 64-bit.
//   - memory-bound kernels: grid-stride loops, ≤2048 blocks.
//   - atomics are device-scope by default on CDNA, which is what we
//     need since per-XCD L2s are not coherent; the insert loop only
//     trusts plain loads for values that can never change once set
//     (slot keys are write-once between clears).
//   - optional wave-level duplicate aggregation (`DEDUP`) cuts atomic
//     contention when key cardinality is low (e.g. 2-key
//     benchmark_windowing workload).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <pybind11/stl.h>
#include <ATen/hip/HIPContext.h>

#include <chrono>
#include <type_traits>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>

#define WAVE 64
#define EMPTY_SLOT 0xFFFFFFFFFFFFFFFFULL

#define HIP_CHECK(expr)                                               \
  do {                                                                \
    hipError_t _e = (expr);                                           \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e)); \
  } while (0)

static inline int n_blocks(int64_t n, int block) {
  int64_t b = (n + block - 1) / block;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

// Scatter-variant selection for the radix window path (A/B-able via
// env until the measured default settles; see profiles/).
enum ScatterKind { SCAT_FIXED = 0, SCAT_DIRECT = 1, SCAT_STAGED = 2 };

static ScatterKind scatter_kind_env() {
  if (const char* s = std::getenv("BYTEWAX_SCATTER")) {
    if (s[0] == 'd') return SCAT_DIRECT;
    if (s[0] == 'f') return SCAT_FIXED;
    if (s[0] == 's') return SCAT_STAGED;
  }
  if (const char* sd = std::getenv("BYTEWAX_SCATTER_DIRECT")) {
    if (atoi(sd) != 0) return SCAT_DIRECT;
  }
  return SCAT_STAGED;
}

// Write-combined staged variant ("staged2"): only consulted where it
// is implemented (COUNT, tumbling, no late tracking).  An explicit
// BYTEWAX_SCATTER=staged selects the plain staged kernel.
#define SCATTER_STAGED2_DEFAULT true
static bool scatter_staged2_env() {
  const char* s = std::getenv("BYTEWAX_SCATTER");
  if (s == nullptr) return SCATTER_STAGED2_DEFAULT;
  return std::strncmp(s, "staged2", 7) == 0;
}

// LDS-deduped region join (BYTEWAX_JOIN_LDS=0 falls back to the
// per-event region kernel for A/B).
static bool join_lds_env() {
  const char* s = std::getenv("BYTEWAX_JOIN_LDS");
  return s == nullptr || s[0] != '0';
}

// Extra segment coarsening: scatter segments cover 2^coarse table
// regions each (longer runs per segment; the agg kernel stages
// 2^(region_bits+coarse) LDS slots per block).
static int scatter_coarse_bits(ScatterKind kind) {
  if (const char* cb = std::getenv("BYTEWAX_SCATTER_COARSE_BITS")) {
    int v = atoi(cb);
    if (v >= 0 && v <= 4) return v;
  }
  return kind == SCAT_STAGED ? 2 : 0;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  // splitmix64 finalizer.
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// Table slot addressing.  Two layouts share one code path:
//   region_bits == 0: classic whole-table linear probing.
//   region_bits  > 0: the table is partitioned into `nslots >>
//     region_bits` contiguous *regions*; a key's region comes from the
//     low hash bits and probing stays inside the region.  This is the
//     layout the radix-partitioned LDS aggregation path flushes into
//     (one workgroup owns one region → L2-local updates).
__device__ __forceinline__ uint64_t region_of(
    uint64_t h64, uint64_t mask, int region_bits) {
  return (h64 & mask) >> region_bits;
}

// Insert `inc` into the open-address table for `packed`, creating the
// slot if needed.  Table size is a power of two (`mask = nslots-1`).
// Returns false if the table (region) is full.
__device__ __forceinline__ bool hash_add(
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int region_bits,
    uint64_t packed,
    unsigned long long inc) {
  uint64_t h64 = mix64(packed);
  uint64_t h, probe_mask, base;
  if (region_bits == 0) {
    base = 0;
    probe_mask = mask;
    h = h64 & mask;
  } else {
    base = region_of(h64, mask, region_bits) << region_bits;
    probe_mask = (1ULL << region_bits) - 1;
    h = (h64 >> 32) & probe_mask;
  }
  for (uint64_t probes = 0; probes <= probe_mask; ++probes) {
    uint64_t slot = base | h;
    uint64_t cur = tkeys[slot];
    if (cur == packed) {
      atomicAdd(&tvals[slot], inc);
      return true;
    }
    if (cur == EMPTY_SLOT) {
      // Plain load may be stale across XCDs; the CAS is the truth.
      uint64_t prev = atomicCAS(
          (unsigned long long*)&tkeys[slot], EMPTY_SLOT, packed);
      if (prev == EMPTY_SLOT || prev == packed) {
        atomicAdd(&tvals[slot], inc);
        return true;
      }
      // Someone else claimed the slot with a different key; keep
      // probing.
    }
    h = (h + 1) & probe_mask;
  }
  return false;
}

__global__ void k_bump(int64_t* p, int64_t v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *p += v;
}

// Aggregation modes baked at compile time per kernel instantiation.
enum AggMode { AGG_COUNT = 0, AGG_SUM = 1,
               // Scatter-only mode for the fused session path:
               // packed = key (no window), value = absolute ts.
               AGG_TS = 2 };

__device__ __forceinline__ uint64_t find_slot(
    uint64_t* __restrict__ tkeys, uint64_t mask, uint64_t packed);
__device__ __forceinline__ uint64_t find_slot_r(
    uint64_t* __restrict__ tkeys, uint64_t mask, int region_bits,
    uint64_t packed);

// Late-event side output of the tumbling/sliding insert kernels (the
// `LATE` instantiations).  An event with absolute `t < late_cutoff`
// joins no window: its (key, t, val) row is appended to the late
// buffer instead and the event is dropped from everything downstream
// of the timestamp read (histograms, table, watermark).  The cursor
// `late_n` is never reset here: rows accumulate across inserts until
// the host drains them.
//
// Append is wave-aggregated like k_close_extract: ballot, one
// atomicAdd per wave by the first late lane, popcount rank.  Safe
// under divergence (tile tails, grid-stride tails): only active lanes
// vote and the leader is by construction an active lane.  The two
// radix scatters aggregate once more per workgroup: the waves reserve
// on an LDS counter and one thread moves the block's total to
// `late_n`, so even a stream with a sparse sprinkle of late events
// (most waves holding one) sends one global atomic per tile / block
// to that single address instead of one per wave.  A row that would
// land at or past `late_cap` sets ERR_LATE_OVERFLOW; the host keeps an
// upper bound on undrained rows so this is a guard only.  `error_flag`
// is a bit set: bit 0 (table / spill overflow) is OR-ed in everywhere,
// never stored over the word, so the two causes stay distinct.
#define ERR_LATE_OVERFLOW 2
#define NO_LATE_ARGS                                                \
  (int64_t)0, (int32_t*)nullptr, (int64_t*)nullptr,                 \
      (int64_t*)nullptr, (int*)nullptr, (int64_t)0

// Wave-aggregated reservation on `counter` (global or LDS): the
// position of this lane among the takers; meaningful only where
// `take`.
__device__ __forceinline__ int wave_reserve(bool take, int* counter) {
  unsigned long long ball = __ballot(take);
  if (ball == 0) return 0;
  int lane = threadIdx.x & (WAVE - 1);
  int lead = __ffsll(ball) - 1;
  int base = 0;
  if (lane == lead) base = atomicAdd(counter, __popcll(ball));
  base = __shfl(base, lead);
  return base + __popcll(ball & ((1ULL << lane) - 1ULL));
}

template <bool HAS_VAL>
__device__ __forceinline__ void late_store(
    int64_t idx, int32_t key, int64_t t, int64_t v,
    int32_t* __restrict__ late_keys, int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals, int64_t late_cap,
    int* __restrict__ error_flag) {
  if (idx >= 0 && idx < late_cap) {
    late_keys[idx] = key;
    late_ts[idx] = t;
    if (HAS_VAL) late_vals[idx] = v;
  } else {
    atomicOr(error_flag, ERR_LATE_OVERFLOW);
  }
}

template <bool HAS_VAL>
__device__ __forceinline__ void late_append(
    bool is_late, int32_t key, int64_t t, int64_t v,
    int32_t* __restrict__ late_keys, int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals, int* __restrict__ late_n,
    int64_t late_cap, int* __restrict__ error_flag) {
  int pos = wave_reserve(is_late, late_n);
  if (is_late) {
    late_store<HAS_VAL>(pos, key, t, v, late_keys, late_ts, late_vals,
                        late_cap, error_flag);
  }
}

template <int MODE, bool DEDUP, typename TS = int64_t, bool LATE = false>
__global__ void k_window_agg_insert(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,  // nullptr for COUNT
    int64_t n,
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int64_t align_ms,
    int64_t len_ms,
    int64_t off_ms,  // window stride; == len_ms for tumbling, < len_ms
                     // for sliding (an event lands in ceil(len/off)
                     // windows)
    int64_t ts_base,  // added to every timestamp (columnar sources can
                      // reuse one template batch across steps)
    int region_bits,  // table layout (see hash_add)
    unsigned long long* __restrict__ max_ts,  // device scalar (atomicMax)
    int* __restrict__ error_flag,
    const int64_t* __restrict__ ts_base_dev,  // extra device-side
                      // offset, lets a captured hipGraph be replayed
                      // with advancing timestamps (see k_bump)
    int64_t late_cutoff,  // LATE only (see late_append)
    int32_t* __restrict__ late_keys,
    int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals,  // unused for COUNT
    int* __restrict__ late_n,
    int64_t late_cap) {
  static_assert(!(LATE && DEDUP), "late tracking excludes the dedup path");
  if (ts_base_dev != nullptr) ts_base += *ts_base_dev;
  int lane = threadIdx.x & (WAVE - 1);
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  // Wave-uniform iteration: every lane of a wave runs every loop
  // iteration (masked by `valid`) so cross-lane ops in the DEDUP path
  // never read from exited lanes.
  int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = first; i - lane < n; i += stride) {
    bool valid = i < n;
    int64_t t = valid ? ((int64_t)ts[i] + ts_base) : 0;
    if constexpr (LATE) {
      // Before the sliding expansion: a late event joins none of its
      // windows, open or not.
      bool is_late = valid && t < late_cutoff;
      int64_t lv = 0;
      if (MODE == AGG_SUM && is_late) lv = vals[i];
      late_append<MODE == AGG_SUM>(
          is_late, is_late ? keys[i] : 0, t, lv, late_keys, late_ts,
          late_vals, late_n, late_cap, error_flag);
      if (is_late) {
        valid = false;
        t = 0;
      }
    }
    if (t > local_max) local_max = t;
    uint64_t packed = 0;
    unsigned long long inc = 0;
    if (valid) {
      int64_t win = (t - align_ms) / off_ms;
      packed = ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
      inc = (MODE == AGG_COUNT) ? 1ULL : (unsigned long long)vals[i];
      if (off_ms < len_ms) {
        // Sliding: also insert into the earlier windows this event
        // overlaps ([win_lo, win)).  The newest window is handled by
        // the shared code below so the DEDUP wave-aggregation path
        // stays correct for tumbling.  Floor division (C trunc would
        // drop the earliest window for events within `len` of align).
        int64_t num = t - align_ms - len_ms;
        int64_t win_lo = num / off_ms;
        if (num % off_ms != 0 && num < 0) win_lo -= 1;
        win_lo += 1;
        for (int64_t wn = win_lo; wn < win; ++wn) {
          uint64_t p2 =
              ((uint64_t)(uint32_t)(int32_t)wn << 32) | (uint32_t)keys[i];
          if (!hash_add(tkeys, tvals, mask, region_bits, p2, inc)) {
            atomicOr(error_flag, 1);
          }
        }
      }
    }

    bool ok = true;
    if (DEDUP) {
      // Wave-aggregate duplicate (key, window) pairs: one atomic per
      // distinct pair per wave.  Worth it only for low-cardinality
      // keys; high-cardinality batches use the plain path.
      unsigned long long remaining = __ballot(valid);
      bool leader = false;
      unsigned long long agg = 0;
      while (remaining) {
        int l = __ffsll((unsigned long long)remaining) - 1;
        uint64_t lk = (uint64_t)__shfl((long long)packed, l);
        unsigned long long match =
            __ballot(valid && packed == lk);
        if (MODE == AGG_COUNT) {
          if (lane == l) {
            leader = true;
            agg = __popcll(match);
          }
        } else {
          // Segmented sum over matching lanes: XOR butterfly gives
          // every lane (incl. the leader) the full total.
          unsigned long long contrib =
              (valid && packed == lk) ? inc : 0ULL;
          for (int off = WAVE / 2; off > 0; off >>= 1) {
            contrib += (unsigned long long)__shfl_xor(
                (long long)contrib, off);
          }
          if (lane == l) {
            leader = true;
            agg = contrib;
          }
        }
        remaining &= ~match;
      }
      if (leader) ok = hash_add(tkeys, tvals, mask, region_bits, packed, agg);
    } else if (valid) {
      ok = hash_add(tkeys, tvals, mask, region_bits, packed, inc);
    }
    if (!ok) atomicOr(error_flag, 1);
  }
  // Wave-reduce the max timestamp, one atomic per wave.
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// ---------------------------------------------------------------------------
// Radix-partitioned LDS-staged aggregation (the high-cardinality fast
// path).  Instead of one random device-scope atomic per event into an
// L2-missing table, events are first partitioned into contiguous
// per-region segments (two streaming passes), then one workgroup
// aggregates each region's events in an LDS-resident open-address
// table (LDS atomics) and flushes distinct keys once into the region's
// contiguous slice of the HBM table — turning ~N random global
// atomics into ~distinct-keys L2-local ones.
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// Radix v2 (experimental, COUNT mode): two-level scheme that writes
// full 64-byte lines.
//
//   Pass A (k_scatter_coarse): events scatter into 256 *coarse*
//   buckets, staged through LDS in block-synchronous tiles so every
//   global write is one aligned 64 B line (8 packed events); partial
//   groups at block end go to a per-bucket residual area (unaligned,
//   ~5% of events).
//
//   Pass B (k_agg_cached): per coarse-bucket slice, aggregate through
//   a 4096-entry LDS cache; collisions and the final flush go through
//   hash_add into the bucket's contiguous span of table regions
//   (cache-local by construction).
// ---------------------------------------------------------------------------

#define V2_COARSE 256
#define V2_STAGE 32  // staged events per coarse bucket per tile

__global__ __launch_bounds__(512) void k_scatter_coarse(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ ts,
    int64_t n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    uint64_t mask,
    int region_bits,
    int64_t cap_c,      // aligned-area capacity per coarse bucket (mult of 8)
    int64_t res_cap,    // residual-area capacity per coarse bucket
    int* __restrict__ gcur,     // [V2_COARSE] aligned-area cursors
    int* __restrict__ gres,     // [V2_COARSE] residual-area cursors
    uint64_t* __restrict__ ev,      // [V2_COARSE * cap_c]
    uint64_t* __restrict__ ev_res,  // [V2_COARSE * res_cap]
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag) {
  __shared__ uint64_t stage[V2_COARSE][V2_STAGE];
  __shared__ int lcnt[V2_COARSE];
  int nb = (int)(((mask + 1) >> region_bits));
  int shift = 0;  // region index -> coarse bucket shift
  while ((nb >> shift) > V2_COARSE) ++shift;
  for (int b = threadIdx.x; b < V2_COARSE; b += blockDim.x) lcnt[b] = 0;
  __syncthreads();

  const int TILE = 8;  // events per thread per tile
  int64_t chunk = (int64_t)blockDim.x * TILE;
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t gstride = (int64_t)gridDim.x * chunk;
  int64_t local_max = 0;
  for (int64_t tile0 = start; tile0 < n; tile0 += gstride) {
    for (int t = 0; t < TILE; ++t) {
      int64_t i = tile0 + (int64_t)t * blockDim.x + threadIdx.x;
      if (i < n) {
        int64_t tm = ts[i] + ts_base;
        if (tm > local_max) local_max = tm;
        int64_t win = (tm - align_ms) / len_ms;
        uint64_t packed =
            ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
        int cb = (int)(region_of(mix64(packed), mask, region_bits) >> shift);
        int r = atomicAdd(&lcnt[cb], 1);
        if (r < V2_STAGE) {
          stage[cb][r] = packed;
        } else {
          // Tile-local stage overflow: straight to the residual area.
          int rp = atomicAdd(&gres[cb], 1);
          if (rp < res_cap) {
            ev_res[(int64_t)cb * res_cap + rp] = packed;
          } else {
            atomicOr(error_flag, 1);
          }
        }
      }
    }
    __syncthreads();
    // Flush complete 8-groups; keep the remainder staged.
    for (int b = threadIdx.x; b < V2_COARSE; b += blockDim.x) {
      int c = lcnt[b];
      if (c > V2_STAGE) c = V2_STAGE;
      int groups = c / 8;
      for (int g = 0; g < groups; ++g) {
        int base8 = atomicAdd(&gcur[b], 8);
        if (base8 + 8 <= cap_c) {
          uint64_t* dst = ev + (int64_t)b * cap_c + base8;
          #pragma unroll
          for (int q = 0; q < 8; ++q) dst[q] = stage[b][g * 8 + q];
        } else {
          for (int q = 0; q < 8; ++q) {
            int rp = atomicAdd(&gres[b], 1);
            if (rp < res_cap) {
              ev_res[(int64_t)b * res_cap + rp] = stage[b][g * 8 + q];
            } else {
              atomicOr(error_flag, 1);
            }
          }
        }
      }
      int rem = c - groups * 8;
      for (int q = 0; q < rem; ++q) {
        stage[b][q] = stage[b][groups * 8 + q];
      }
      lcnt[b] = rem;
    }
    __syncthreads();
  }
  // Final residual flush.
  for (int b = threadIdx.x; b < V2_COARSE; b += blockDim.x) {
    int c = lcnt[b];
    if (c > V2_STAGE) c = V2_STAGE;
    for (int q = 0; q < c; ++q) {
      int rp = atomicAdd(&gres[b], 1);
      if (rp < res_cap) {
        ev_res[(int64_t)b * res_cap + rp] = stage[b][q];
      } else {
        atomicOr(error_flag, 1);
      }
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

#define V2_CACHE 4096  // LDS cache entries in pass B

__global__ __launch_bounds__(256) void k_agg_cached(
    const uint64_t* __restrict__ ev,
    const uint64_t* __restrict__ ev_res,
    const int* __restrict__ gcur,
    const int* __restrict__ gres,
    int64_t cap_c,
    int64_t res_cap,
    int slices,  // blocks per coarse bucket
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int region_bits,
    int* __restrict__ error_flag) {
  __shared__ uint64_t ckeys[V2_CACHE];
  __shared__ unsigned long long cvals[V2_CACHE];
  for (int s = threadIdx.x; s < V2_CACHE; s += blockDim.x) {
    ckeys[s] = EMPTY_SLOT;
    cvals[s] = 0;
  }
  __syncthreads();
  int cb = blockIdx.x % V2_COARSE;
  int slice = blockIdx.x / V2_COARSE;

  auto agg_one = [&](uint64_t packed) {
    uint64_t h64 = mix64(packed);
    int lh = (int)((h64 >> 20) & (V2_CACHE - 1));
    // Two-probe LDS cache; collisions go straight to the table.
    for (int p = 0; p < 2; ++p) {
      uint64_t cur = ckeys[lh];
      if (cur == packed) {
        atomicAdd(&cvals[lh], 1ULL);
        return;
      }
      if (cur == EMPTY_SLOT) {
        uint64_t prev = atomicCAS(
            (unsigned long long*)&ckeys[lh], EMPTY_SLOT, packed);
        if (prev == EMPTY_SLOT || prev == packed) {
          atomicAdd(&cvals[lh], 1ULL);
          return;
        }
      }
      lh = (lh + 1) & (V2_CACHE - 1);
    }
    if (!hash_add(tkeys, tvals, mask, region_bits, packed, 1ULL)) {
      atomicOr(error_flag, 1);
    }
  };

  int c = gcur[cb];
  if (c > cap_c) c = (int)cap_c;
  for (int j = slice * (int)blockDim.x + threadIdx.x; j < c;
       j += slices * (int)blockDim.x) {
    agg_one(ev[(int64_t)cb * cap_c + j]);
  }
  int cr = gres[cb];
  if (cr > res_cap) cr = (int)res_cap;
  for (int j = slice * (int)blockDim.x + threadIdx.x; j < cr;
       j += slices * (int)blockDim.x) {
    agg_one(ev_res[(int64_t)cb * res_cap + j]);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < V2_CACHE; s += blockDim.x) {
    if (ckeys[s] != EMPTY_SLOT) {
      if (!hash_add(tkeys, tvals, mask, region_bits, ckeys[s], cvals[s])) {
        atomicOr(error_flag, 1);
      }
    }
  }
}

// One-pass variant: events scatter into fixed-capacity per-region
// buffers (capacity `cap` each, laid out at region*cap), which removes
// the separate counting pass and the offsets scan.  A block's chunk
// that would overflow its region's buffer goes to the overflow spill
// (aggregated by k_radix_agg's caller via the contended-direct path —
// statistically empty for uniform keys at cap = 2x mean).
// GCN has no integer divide; `x / len_ms` compiles to a ~60-cycle
// sequence and the scatter does it twice per event.  The host
// precomputes a Granlund-Montgomery magic multiplier instead:
// win = mulhi64(x, m2) is exact for 0 <= x < maxfast (m2 == 0 or
// x outside the window falls back to the hardware-free division).
// Oldest window overlapping t for a sliding windower: the window ids
// are strides of `off`; an event at t lands in ids
// [floor((t-align-len)/off)+1, (t-align)/off].
__device__ __forceinline__ int64_t win_lo_of(
    int64_t t, int64_t align_ms, int64_t len_ms, int64_t off_ms) {
  int64_t num = t - align_ms - len_ms;
  int64_t fl = num >= 0 ? num / off_ms : -((-num + off_ms - 1) / off_ms);
  return fl + 1;
}

__device__ __forceinline__ int64_t win_of(
    int64_t t, int64_t align_ms, int64_t len_ms, uint64_t m2,
    uint64_t maxfast) {
  int64_t x = t - align_ms;
  if (m2 != 0 && (uint64_t)x < maxfast) {
    return (int64_t)__umul64hi((uint64_t)x, m2);
  }
  return x / len_ms;  // same truncation semantics as before
}

// Host side of the magic divider: p = 60 covers numerators < 2^60/e
// (ms-scale timestamps are < 2^43).  Power-of-two lengths reduce to a
// plain mulhi shift; len <= 1 disables the fast path.
static inline void magic_div_u64(
    int64_t d, uint64_t* m2, uint64_t* maxfast) {
  *m2 = 0;
  *maxfast = 0;
  if (d <= 1) return;
  if ((d & (d - 1)) == 0) {
    int s = 0;
    while ((int64_t(1) << s) < d) ++s;
    *m2 = (uint64_t)1 << (64 - s);
    *maxfast = ~(uint64_t)0;
    return;
  }
  const unsigned p = 60;
  unsigned __int128 one = 1;
  uint64_t M = (uint64_t)(((one << p) + (uint64_t)d - 1) / (uint64_t)d);
  uint64_t e = (uint64_t)((unsigned __int128)M * (uint64_t)d - (one << p));
  *m2 = M << 4;  // M < 2^60 for d >= 2, so the shift is exact
  *maxfast = e ? (uint64_t)((one << p) / e) : ~(uint64_t)0;
}

// 32-bit window arithmetic for a launch of int32 deltas from one
// host-known base (tumbling windows).  With a window id W chosen by the
// host and c = ts_base - align_ms - W * len_ms, an event's window is
// W + floor(y / len_ms), y = delta + c, whenever 0 <= y < 2^32 and the
// event does not lie before align_ms (where win_of truncates towards
// zero instead).  The host turns those conditions into one delta range
// [dlo, dlo + dspan) and passes the round-up divider of Granlund and
// Montgomery (1994, fig. 4.1), which is exact for every 32-bit
// numerator and every divisor 1 <= len_ms < 2^32:
//   t = mulhi(dm, y);  q = (t + ((y - t) >> sh1)) >> sh2.
struct Win32 {
  uint32_t dlo;    // first delta of the fast range
  uint32_t dspan;  // its size; 0 sends every event to the generic path
  uint32_t c;      // c mod 2^32
  uint32_t wlo;    // W mod 2^32 (`packed` keeps 32 bits of the window)
  uint32_t qoff;   // hashed entries store q - qoff (entry base W + qoff)
  uint32_t dm;
  int sh1, sh2;
};

__device__ __forceinline__ uint32_t win32_div(uint32_t y, const Win32& w) {
  uint32_t t = __umulhi(w.dm, y);
  return (t + ((y - t) >> w.sh1)) >> w.sh2;
}

// Hashed scatter entries, the second `ev_packed` format, written by
// k_radix_scatter_staged2<.., true> and read by
// k_radix_agg_count<.., .., true> only:
//   bits 63..32  key32
//   bits 31..13  window delta against the call's entry base (19 bits)
//   bits 12..0   (mix64(packed) >> 32) & 0x1FFF
// The aggregation takes its LDS slot from the low bits (its tables have
// at most 2^13 slots) and never hashes an entry it can count in LDS.
// The largest delta is not used, so no entry equals the all-ones pad.
#define ENTRY_SLOT_BITS 13
#define ENTRY_SLOT_MASK 0x1FFFull
#define ENTRY_DELTA_MASK 0x7FFFFu
#define ENTRY_DELTA_LIMIT 0x7FFFFu  // deltas 0 .. LIMIT - 1 are stored
// "Classic entries" in place of an entry base.
#define ENTRY_W_CLASSIC INT64_MIN

__device__ __forceinline__ uint32_t entry_delta(uint64_t entry) {
  return ((uint32_t)entry >> ENTRY_SLOT_BITS) & ENTRY_DELTA_MASK;
}

__device__ __forceinline__ uint64_t entry_classic(
    uint64_t entry, uint32_t wlo) {
  return ((uint64_t)(wlo + entry_delta(entry)) << 32) | (entry >> 32);
}

// Compact scatter entries, the third `ev_packed` format (4 bytes),
// written by k_radix_scatter_compact and read by k_radix_agg_compact
// only.  With S = log2(segments) and D = S - 1 window-delta bits, the
// event is the word x = key32 | delta << 32 of n = 32 + D bits and
// y = mixn(x, n) a bijection of it:
//   segment  the top S bits of y (y >> 31)
//   entry    the low 31 bits of y; bit 31 stays 0, so all-ones is the pad
//   LDS slot the top `seg_bits` bits of the entry
// The segment index and the entry together are y, and mixn_inv gives
// the key and the window back; that runs once per distinct cell at the
// aggregation's flush, and where the scatter sends a granule to the
// overflow spill.  mixn is three rounds of x ^= x >> ceil(n/2) and an
// odd multiply mod 2^n, and a last xor-shift.  A shift of at least n/2
// is its own inverse; the multiplies are undone by the constants'
// inverses mod 2^64, which are their inverses mod 2^n as well.
#define ENTRY_PAD32 0xFFFFFFFFu
#define ENTRY_FMT_CLASSIC 0
#define ENTRY_FMT_HASHED 1
#define ENTRY_FMT_COMPACT 2
#define MIXN_C1 0xff51afd7ed558ccdULL
#define MIXN_C2 0xc4ceb9fe1a85ec53ULL
#define MIXN_C3 0x9e3779b97f4a7c15ULL

constexpr uint64_t mixn_inverse_of(uint64_t c) {
  uint64_t x = c;  // Newton: correct bits double each step, 3 at start
  for (int i = 0; i < 6; ++i) x *= 2 - c * x;
  return x;
}

__host__ __device__ __forceinline__ uint64_t mixn(uint64_t x, int n) {
  const uint64_t m = ((uint64_t)1 << n) - 1;
  const int s = (n + 1) >> 1;
  x ^= x >> s;
  x = (x * MIXN_C1) & m;
  x ^= x >> s;
  x = (x * MIXN_C2) & m;
  x ^= x >> s;
  x = (x * MIXN_C3) & m;
  x ^= x >> s;
  return x;
}

__host__ __device__ __forceinline__ uint64_t mixn_inv(uint64_t y, int n) {
  const uint64_t m = ((uint64_t)1 << n) - 1;
  const int s = (n + 1) >> 1;
  constexpr uint64_t i1 = mixn_inverse_of(MIXN_C1);
  constexpr uint64_t i2 = mixn_inverse_of(MIXN_C2);
  constexpr uint64_t i3 = mixn_inverse_of(MIXN_C3);
  static_assert(i1 * MIXN_C1 == 1 && i2 * MIXN_C2 == 1 && i3 * MIXN_C3 == 1,
                "inverse constants");
  y ^= y >> s;
  y = (y * i3) & m;
  y ^= y >> s;
  y = (y * i2) & m;
  y ^= y >> s;
  y = (y * i1) & m;
  y ^= y >> s;
  return y;
}

// mixn on the 32-bit halves of x = hi << 32 | lo, in place: the same
// value as mixn(x, n) for 33 <= n <= 56 (MIXN_PAIR_MIN_N, _MAX_N) and
// hi < 2^(n-32).  With s = ceil(n/2) in 17..28:
//   - x >> s is below 2^32 (n - s <= 32), so an xor-shift changes only
//     `lo`, by the low word of the pair shifted right (one alignbit);
//   - of the high word of x * C only the low n - 32 <= 24 bits survive
//     the mask, and the low 24 bits of a product depend only on the low
//     24 bits of its factors, so the two cross terms are 24-bit
//     multiplies and one 32x32 -> 64 multiply per round is left.
#define MIXN_PAIR_MIN_N 33
#define MIXN_PAIR_MAX_N 56

__device__ __forceinline__ void mixn_pair(uint32_t& lo, uint32_t& hi, int n) {
  const uint32_t hm = (1u << (n - 32)) - 1u;
  const uint32_t s = (uint32_t)(n + 1) >> 1;
  auto round = [&](uint64_t c) {
    lo ^= __builtin_amdgcn_alignbit(hi, lo, s);
    const uint64_t p = (uint64_t)lo * (uint32_t)c;
    hi = ((uint32_t)(p >> 32) + __umul24(lo, (uint32_t)(c >> 32)) +
          __umul24(hi, (uint32_t)c)) & hm;
    lo = (uint32_t)p;
  };
  round(MIXN_C1);
  round(MIXN_C2);
  round(MIXN_C3);
  lo ^= __builtin_amdgcn_alignbit(hi, lo, s);
}

// Classic `packed` of the compact entry `e` of segment `seg`, against
// the entry base whose low 32 bits are `wbase`.
__device__ __forceinline__ uint64_t compact_classic(
    uint32_t seg, uint32_t e, int n, uint32_t wbase) {
  uint64_t x = mixn_inv(((uint64_t)seg << 31) | e, n);
  return ((uint64_t)(wbase + (uint32_t)(x >> 32)) << 32) | (uint32_t)x;
}

// TS is int64_t (absolute ms) or int32_t (deltas from `ts_base`, the
// wire format of the RCCL exchange — inserting the received segments
// directly skips the int64 timestamp rebuild entirely).
template <int MODE, typename TS = int64_t, bool LATE = false>
__global__ void k_radix_scatter_fixed(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,
    int64_t n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t off_ms,  // sliding stride; == len_ms for tumbling
    int64_t ts_base,
    uint64_t mask,
    int region_bits,
    int64_t cap,
    int* __restrict__ gcursors,       // [n_regions], pre-zeroed
    uint64_t* __restrict__ ev_packed,  // [n_regions * cap]
    int64_t* __restrict__ ev_vals,
    int* __restrict__ ov_cursor,       // [1], pre-zeroed
    uint64_t* __restrict__ ov_packed,  // overflow spill
    int64_t* __restrict__ ov_vals,
    int64_t ov_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    uint64_t win_m2,
    uint64_t win_maxfast,
    int64_t late_cutoff,  // LATE only (see late_append)
    int32_t* __restrict__ late_keys,
    int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals,  // unused for COUNT
    int* __restrict__ late_n,
    int64_t late_cap) {
  static_assert(!(LATE && MODE == AGG_TS), "no late tracking for AGG_TS");
  extern __shared__ int lmem[];
  // LATE: [0] the block's late rows (pass 1), then their placement
  // cursor (pass 2); [1] the block's base in the late buffer.
  __shared__ int s_late[LATE ? 2 : 1];
  int nb = (int)(((mask + 1) >> region_bits));
  int* lhist = lmem;
  int* lbase = lmem + nb;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) lhist[b] = 0;
  if constexpr (LATE) {
    if (threadIdx.x == 0) s_late[0] = 0;
  }
  __syncthreads();
  int64_t start = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  for (int64_t i = start; i < n; i += stride) {
    int64_t t = (int64_t)ts[i] + ts_base;
    if constexpr (LATE) {
      // Counted here, stored by the placement pass; skipped by both.
      bool is_late = t < late_cutoff;
      wave_reserve(is_late, &s_late[0]);
      if (is_late) continue;
    }
    if (t > local_max) local_max = t;
    uint64_t packed;
    int nwin = 1;
    if (MODE == AGG_TS) {
      packed = (uint64_t)(uint32_t)keys[i];
    } else {
      int64_t win = win_of(t, align_ms, off_ms, win_m2, win_maxfast);
      packed = ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
      if (off_ms < len_ms) {
        nwin = (int)(win - win_lo_of(t, align_ms, len_ms, off_ms)) + 1;
      }
    }
    for (int w = 0; w < nwin; ++w) {
      atomicAdd(&lhist[(int)region_of(mix64(packed), mask, region_bits)], 1);
      packed -= (uint64_t)1 << 32;
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    // Unbounded reservation (one atomic per block x bucket; a bounded
    // CAS loop here storms under 2048-way contention).  Items whose
    // in-bucket position lands past `cap` spill to overflow; a block
    // still fills [base, cap) contiguously so the buffer has no holes
    // and readers clamp the cursor to `cap`.
    lbase[b] = lhist[b] > 0 ? atomicAdd(&gcursors[b], lhist[b]) : 0;
    lhist[b] = 0;
  }
  if constexpr (LATE) {
    if (threadIdx.x == 0) {
      s_late[1] = s_late[0] > 0 ? atomicAdd(late_n, s_late[0]) : 0;
      s_late[0] = 0;
    }
  }
  __syncthreads();
  for (int64_t i = start; i < n; i += stride) {
    int64_t t = (int64_t)ts[i] + ts_base;
    if constexpr (LATE) {
      bool is_late = t < late_cutoff;
      int lpos = wave_reserve(is_late, &s_late[0]);
      if (is_late) {
        late_store<MODE == AGG_SUM>(
            (int64_t)s_late[1] + lpos, keys[i], t,
            MODE == AGG_SUM ? vals[i] : 0, late_keys, late_ts, late_vals,
            late_cap, error_flag);
        continue;
      }
    }
    uint64_t packed;
    int nwin = 1;
    if (MODE == AGG_TS) {
      packed = (uint64_t)(uint32_t)keys[i];
    } else {
      int64_t win = win_of(t, align_ms, off_ms, win_m2, win_maxfast);
      packed = ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
      if (off_ms < len_ms) {
        nwin = (int)(win - win_lo_of(t, align_ms, len_ms, off_ms)) + 1;
      }
    }
    int64_t v = (MODE == AGG_SUM) ? vals[i] : (MODE == AGG_TS ? t : 0);
    for (int w = 0; w < nwin; ++w) {
      int b = (int)region_of(mix64(packed), mask, region_bits);
      int64_t in_bucket = lbase[b] + atomicAdd(&lhist[b], 1);
      if (in_bucket < cap) {
        int64_t pos = (int64_t)b * cap + in_bucket;
        ev_packed[pos] = packed;
        if (MODE != AGG_COUNT) ev_vals[pos] = v;
      } else {
        int opos = atomicAdd(ov_cursor, 1);
        if (opos < ov_cap) {
          ov_packed[opos] = packed;
          if (MODE != AGG_COUNT) ov_vals[opos] = v;
        } else {
          atomicOr(error_flag, 1);
        }
      }
      packed -= (uint64_t)1 << 32;
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// Direct one-pass scatter variant: one global atomicAdd on the
// region cursor per event, single read of the input (the block-hist
// version reads the input twice and does two LDS atomics per event).
// The region cursors are ~n_regions hot words in L2; with ≥2^11
// regions the per-address serialization is far below the memory
// time.  Selected via BYTEWAX_SCATTER_DIRECT (measured A/B; see
// profiles/).
template <int MODE, typename TS = int64_t>
__global__ void k_radix_scatter_direct(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,
    int64_t n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t off_ms,  // accepted for launch-shape parity; the launcher
                     // routes sliding (off < len) to the fixed variant
    int64_t ts_base,
    uint64_t mask,
    int region_bits,
    int64_t cap,
    int* __restrict__ gcursors,
    uint64_t* __restrict__ ev_packed,
    int64_t* __restrict__ ev_vals,
    int* __restrict__ ov_cursor,
    uint64_t* __restrict__ ov_packed,
    int64_t* __restrict__ ov_vals,
    int64_t ov_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    uint64_t win_m2,
    uint64_t win_maxfast) {
  int64_t start = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  for (int64_t i = start; i < n; i += stride) {
    int64_t t = (int64_t)ts[i] + ts_base;
    if (t > local_max) local_max = t;
    int64_t win = win_of(t, align_ms, len_ms, win_m2, win_maxfast);
    uint64_t packed =
        ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
    int b = (int)region_of(mix64(packed), mask, region_bits);
    int64_t in_bucket = atomicAdd(&gcursors[b], 1);
    int64_t v = (MODE == AGG_SUM) ? vals[i] : 0;
    if (in_bucket < cap) {
      int64_t pos = (int64_t)b * cap + in_bucket;
      ev_packed[pos] = packed;
      if (MODE == AGG_SUM) ev_vals[pos] = v;
    } else {
      int opos = atomicAdd(ov_cursor, 1);
      if (opos < ov_cap) {
        ov_packed[opos] = packed;
        if (MODE == AGG_SUM) ov_vals[opos] = v;
      } else {
        atomicOr(error_flag, 1);
      }
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// Line-staged scatter: kills the partial-line write amplification of
// the scattered 8 B segment writes (round-1 PMC: 7.7x — ~2 GB of
// actual HBM writes for a 256 MB payload).  Two invariants make every
// `ev_packed` line a single full-line HBM write:
//   1. the shared segment cursors advance only in SC_GRAN-event
//      (64 B) units, so each line is exclusively owned by the one
//      block that reserved it (no cross-XCD line sharing);
//   2. a block writes all 8 entries of its granule within one tile
//      phase, so the line completes in the local XCD's L2 (and is
//      evicted once, whole) instead of staying open across the whole
//      input sweep.
// Events stage per segment in LDS; residual (< SC_GRAN) events per
// segment ride along across tiles and flush as sentinel-padded
// granules at the end (the aggregation kernels skip EMPTY_SLOT).
// Segments may be COARSER than table regions (seg_bits >
// region_bits): fewer, longer runs; the agg kernel then covers
// 2^(seg_bits-region_bits) regions per block.
#define SC_GRAN 8  // events per cursor reservation = one 64 B line

template <int MODE, typename TS = int64_t, int U = 16, int BLK = 256,
          bool LATE = false>
__global__ __launch_bounds__(BLK) void k_radix_scatter_staged(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,  // nullptr for COUNT
    int64_t n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t off_ms,  // sliding stride; == len_ms for tumbling
    int64_t ts_base,
    uint64_t mask,
    int seg_bits,
    int64_t cap,  // per-segment capacity; multiple of SC_GRAN
    int* __restrict__ gcursors,        // [nseg], zeroed before 1st call
    uint64_t* __restrict__ ev_packed,  // [nseg * cap]
    int64_t* __restrict__ ev_vals,     // [nseg * cap] (SUM)
    int* __restrict__ ov_cursor,
    uint64_t* __restrict__ ov_packed,
    int64_t* __restrict__ ov_vals,
    int64_t ov_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    uint64_t win_m2,
    uint64_t win_maxfast,
    int64_t late_cutoff,  // LATE only (see late_append)
    int32_t* __restrict__ late_keys,
    int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals,  // unused for COUNT
    int* __restrict__ late_n,
    int64_t late_cap) {
  static_assert(!(LATE && MODE == AGG_TS), "no late tracking for AGG_TS");
  extern __shared__ char smem[];
  // LATE: [0] late rows of the current tile, [1] their base in the
  // late buffer (reserved in P2, consumed in P3b).
  __shared__ int s_late[LATE ? 2 : 1];
  const int nseg = (int)(((mask + 1) >> seg_bits));
  uint64_t* res = (uint64_t*)smem;  // [nseg][SC_GRAN] residual staging
  int64_t* res_v =
      (int64_t*)(smem + (size_t)nseg * SC_GRAN * 8);  // SUM/TS only
  int* res_cnt =
      (int*)(smem + (size_t)nseg * SC_GRAN * 8 *
                        (MODE != AGG_COUNT ? 2 : 1));  // [nseg]
  int* lhist = res_cnt + nseg;  // [nseg] tile hist, then grant
  int* lbase = lhist + nseg;    // [nseg] granted global base
  int* lofs = lbase + nseg;     // [nseg] virtual-position cursor
  for (int b = threadIdx.x; b < nseg; b += blockDim.x) {
    res_cnt[b] = 0;
    lhist[b] = 0;
  }
  if constexpr (LATE) {
    if (threadIdx.x == 0) s_late[0] = 0;
  }
  __syncthreads();

  // One granule write, with capacity split to the overflow spill.
  auto emit = [&](int b, int64_t gpos, uint64_t packed, int64_t v) {
    if (gpos < cap) {
      int64_t pos = (int64_t)b * cap + gpos;
      ev_packed[pos] = packed;
      if (MODE != AGG_COUNT) ev_vals[pos] = v;
    } else if (packed != EMPTY_SLOT) {
      int opos = atomicAdd(ov_cursor, 1);
      if (opos < ov_cap) {
        ov_packed[opos] = packed;
        if (MODE != AGG_COUNT) ov_vals[opos] = v;
      } else {
        atomicOr(error_flag, 1);
      }
    }
  };

  const int64_t tile = (int64_t)blockDim.x * U;
  int64_t local_max = 0;
  for (int64_t t0 = (int64_t)blockIdx.x * tile; t0 < n;
       t0 += (int64_t)gridDim.x * tile) {
    uint64_t pk[U];
    int64_t pv[U];
    int sg[U];
    int nw[U];
    // P1: load, classify, histogram.
    for (int u = 0; u < U; ++u) {
      int64_t i = t0 + (int64_t)u * blockDim.x + threadIdx.x;
      sg[u] = -1;
      if constexpr (LATE) {
        // Every lane of the wave votes (tail lanes as "not late").  A
        // late event never reaches the tile histogram; it keeps a
        // negative sg[u] (-2, which P3b turns into the late row) and
        // its rank within the tile in nw[u].
        bool in = i < n;
        int64_t tl = in ? ((int64_t)ts[i] + ts_base) : 0;
        bool is_late = in && tl < late_cutoff;
        int lpos = wave_reserve(is_late, &s_late[0]);
        if (is_late) {
          sg[u] = -2;
          nw[u] = lpos;
          continue;
        }
      }
      if (i >= n) continue;
      int64_t t = (int64_t)ts[i] + ts_base;
      if (t > local_max) local_max = t;
      uint64_t packed;
      int nwin = 1;
      if (MODE == AGG_TS) {
        packed = (uint64_t)(uint32_t)keys[i];
      } else {
        // `win_m2` is the magic divisor of the STRIDE (off_ms); for a
        // sliding windower the event expands into every window id in
        // [win_lo, win].
        int64_t win = win_of(t, align_ms, off_ms, win_m2, win_maxfast);
        packed =
            ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
        if (off_ms < len_ms) {
          nwin =
              (int)(win - win_lo_of(t, align_ms, len_ms, off_ms)) + 1;
        }
      }
      pk[u] = packed;
      nw[u] = nwin;
      if (MODE == AGG_SUM) pv[u] = vals[i];
      else if (MODE == AGG_TS) pv[u] = t;
      int b = (int)region_of(mix64(packed), mask, seg_bits);
      sg[u] = b;
      atomicAdd(&lhist[b], 1);
      // Expanded entries get their own histogram slots.
      uint64_t p2 = packed;
      for (int w = 1; w < nwin; ++w) {
        p2 -= (uint64_t)1 << 32;
        atomicAdd(
            &lhist[(int)region_of(mix64(p2), mask, seg_bits)], 1);
      }
    }
    __syncthreads();
    // P2: per-segment granule reservation.
    for (int b = threadIdx.x; b < nseg; b += blockDim.x) {
      int tot = res_cnt[b] + lhist[b];
      int grant = tot & ~(SC_GRAN - 1);
      lbase[b] = grant > 0 ? atomicAdd(&gcursors[b], grant) : 0;
      lofs[b] = res_cnt[b];
      lhist[b] = grant;
    }
    if constexpr (LATE) {
      if (threadIdx.x == 0)
        s_late[1] = s_late[0] > 0 ? atomicAdd(late_n, s_late[0]) : 0;
    }
    __syncthreads();
    // P3a: drain old residual into the granted granule (granule >=
    // SC_GRAN > residual when granted, so all-or-nothing).
    for (int b = threadIdx.x; b < nseg; b += blockDim.x) {
      int grant = lhist[b];
      if (grant > 0) {
        int rc = res_cnt[b];
        int gb = lbase[b];
        for (int j = 0; j < rc; ++j) {
          emit(b, (int64_t)gb + j, res[(size_t)b * SC_GRAN + j],
               MODE != AGG_COUNT ? res_v[(size_t)b * SC_GRAN + j] : 0);
        }
        res_cnt[b] = 0;
      }
    }
    __syncthreads();
    // P3b: place this tile's (possibly window-expanded) entries at
    // their virtual positions.
    for (int u = 0; u < U; ++u) {
      if constexpr (LATE) {
        if (sg[u] == -2) {
          int64_t i = t0 + (int64_t)u * blockDim.x + threadIdx.x;
          late_store<MODE == AGG_SUM>(
              (int64_t)s_late[1] + nw[u], keys[i], (int64_t)ts[i] + ts_base,
              MODE == AGG_SUM ? vals[i] : 0, late_keys, late_ts, late_vals,
              late_cap, error_flag);
        }
      }
      if (sg[u] < 0) continue;
      uint64_t p2 = pk[u];
      for (int w = 0; w < nw[u]; ++w) {
        int b = w == 0 ? sg[u]
                       : (int)region_of(mix64(p2), mask, seg_bits);
        int vpos = atomicAdd(&lofs[b], 1);
        int grant = lhist[b];
        if (vpos < grant) {
          emit(b, (int64_t)lbase[b] + vpos, p2,
               MODE != AGG_COUNT ? pv[u] : 0);
        } else {
          res[(size_t)b * SC_GRAN + (vpos - grant)] = p2;
          if (MODE != AGG_COUNT)
            res_v[(size_t)b * SC_GRAN + (vpos - grant)] = pv[u];
        }
        p2 -= (uint64_t)1 << 32;
      }
    }
    __syncthreads();
    // P3c: carry the leftover count; reset the histogram.
    for (int b = threadIdx.x; b < nseg; b += blockDim.x) {
      res_cnt[b] = lofs[b] - lhist[b];
      lhist[b] = 0;
    }
    if constexpr (LATE) {
      if (threadIdx.x == 0) s_late[0] = 0;
    }
    __syncthreads();
  }
  // Final flush: pad each non-empty residual to a full granule with
  // EMPTY_SLOT sentinels (skipped by the agg kernels).
  for (int b = threadIdx.x; b < nseg; b += blockDim.x) {
    int rc = res_cnt[b];
    if (rc == 0) continue;
    int gb = atomicAdd(&gcursors[b], SC_GRAN);
    for (int j = 0; j < SC_GRAN; ++j) {
      uint64_t p = j < rc ? res[(size_t)b * SC_GRAN + j] : EMPTY_SLOT;
      emit(b, (int64_t)gb + j, p,
           (MODE != AGG_COUNT && j < rc) ? res_v[(size_t)b * SC_GRAN + j]
                                         : 0);
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}


// Write-combined variant of the staged scatter (COUNT, tumbling, no
// late tracking).  Same contract as k_radix_scatter_staged — the
// `ev_packed` layout, SC_GRAN reservation of the shared cursors, the
// sentinel-padded final flush, the capacity split to the overflow
// spill and `max_ts` — so k_radix_agg cannot tell them apart.  What
// changes is how a granted entry reaches memory: instead of one 8-byte
// store per event from whichever lane happens to hold it (a wave store
// touching 64 different lines), the tile's granted entries are staged
// in LDS grouped by segment, and copied out in 16-byte pieces with
// four adjacent lanes covering one 64-byte line.  A wave store then
// writes 16 whole lines: 8x fewer store requests and 2x fewer store
// instructions for the same bytes.
//
// Per tile (BLK * U events, four barriers):
//   P1   classify (the columns were loaded a tile ahead), returning
//        LDS atomic on the segment histogram: the old value is the
//        event's rank in its segment for this tile, so no second
//        cursor atomic is needed.  Then load the next tile's columns.
//   P2a  thread b: tot = residual + hist, grant = tot & ~7, reserve
//        `grant` on the shared cursor; wave scan of the grants.
//   P2b  cross-wave step of the scan -> staging offset of segment b;
//        one destination per granule into gdst[] (or GD_SPILL when the
//        granule lies at or beyond `cap`: cap, bases and grants are
//        multiples of 8, so a granule is wholly inside or outside);
//        old residual drains to the head of the run.
//   P3   events go to stage[off + rc + rank] when inside the grant,
//        else to the residual array.
//   P4   copy-out, lane p takes piece p.
// The default for tumbling COUNT; BYTEWAX_SCATTER=staged2 names it,
// BYTEWAX_SCATTER=staged selects the plain kernel instead.
#define GD_SPILL 0xFFFFFFFFu

// Dynamic LDS of k_radix_scatter_staged2 for a tile of `tile` events.
static inline size_t staged2_lds_bytes(int64_t nseg, int64_t tile) {
  size_t stage_n = (size_t)(tile + 7 * nseg);  // multiple of 8
  return stage_n * 8                           // stage
         + (size_t)nseg * SC_GRAN * 8          // res
         + 3 * (size_t)nseg * sizeof(int)      // res_cnt, lhist, lpack
         + (stage_n / SC_GRAN) * sizeof(uint32_t);  // gdst
}

//
// HASHED (int32 deltas from one host-known base only) writes hashed
// entries (ENTRY_* above) for k_radix_agg_count<.., .., true>; the hash
// that picks an event's segment also gives its entry the LDS slot.  In
// this form P1 takes the window from the 32-bit arithmetic of Win32 and
// issues its U histogram atomics unconditionally, as one batch.  An
// event outside the host-proved delta range, or whose window does not
// fit the 19-bit entry delta, is classified by the generic win_of in
// one rare loop behind P1 and goes to the overflow spill, which holds
// classic `packed` in either format (so does what the capacity split
// sends there).  Measured at the bench shape, the 64-bit window code
// and per-event atomic waits of the classic form cost the hashed kernel
// 29 us of 368 (see profiles/r06_hashed_entries.md).
template <typename TS = int64_t, int U = 16, int BLK = 512,
          bool HASHED = false>
__global__ __launch_bounds__(BLK) void k_radix_scatter_staged2(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,  // unused (COUNT)
    int64_t n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t off_ms,
    int64_t ts_base,
    uint64_t mask,
    int seg_bits,
    int64_t cap,
    int* __restrict__ gcursors,
    uint64_t* __restrict__ ev_packed,
    int64_t* __restrict__ ev_vals,  // unused (COUNT)
    int* __restrict__ ov_cursor,
    uint64_t* __restrict__ ov_packed,
    int64_t* __restrict__ ov_vals,  // unused (COUNT)
    int64_t ov_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    uint64_t win_m2,
    uint64_t win_maxfast,
    Win32 w32) {  // HASHED only
  static_assert(!HASHED || sizeof(TS) == 4, "hashed entries need deltas");
  constexpr int T = BLK * U;
  constexpr int NW = BLK / WAVE;
  // lpack: staging offset (14 bits) | residual count (3) | grant (14+).
  static_assert(T + 7 * BLK < (1 << 14), "staging offset must fit 14 bits");
  static_assert(T <= (1 << 13), "tile rank shares a word with the segment");
  extern __shared__ __attribute__((aligned(16))) char smem_wc[];
  __shared__ int s_wtot[NW];
  const int nseg = (int)(((mask + 1) >> seg_bits));  // host: nseg <= BLK
  const int stage_n = T + 7 * nseg;
  uint64_t* stage = (uint64_t*)smem_wc;        // [stage_n]
  uint64_t* res = stage + stage_n;             // [nseg][SC_GRAN]
  int* res_cnt = (int*)(res + (size_t)nseg * SC_GRAN);  // [nseg]
  int* lhist = res_cnt + nseg;                 // [nseg]
  int* lpack = lhist + nseg;                   // [nseg]
  uint32_t* gdst = (uint32_t*)(lpack + nseg);  // [stage_n / SC_GRAN]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  if (tid < nseg) {
    res_cnt[tid] = 0;
    lhist[tid] = 0;
  }
  __syncthreads();

  auto spill = [&](uint64_t packed) {
    int opos = atomicAdd(ov_cursor, 1);
    if (opos < ov_cap) ov_packed[opos] = packed;
    else atomicOr(error_flag, 1);
  };

  // The spill holds classic `packed` whatever the entry format is.
  auto classic_of = [&](uint64_t entry) {
    return HASHED ? entry_classic(entry, w32.wlo + w32.qoff) : entry;
  };

  // Raw columns of one tile, loaded a tile ahead.  The loads carry no
  // branch (the index is clamped, the lane is masked in P1): a branch
  // around each load makes U dependent round trips out of one batch,
  // and with one workgroup per CU nothing else would hide them.
  int32_t rk[U];
  TS rt[U];
  auto load_tile = [&](int64_t t0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int64_t i = t0 + u * BLK + tid;
      if (i > n - 1) i = n - 1;
      rk[u] = keys[i];
      rt[u] = ts[i];
    }
  };
  const int64_t stride = (int64_t)gridDim.x * T;
  // Classic: maximum of the absolute timestamps.  Hashed: maximum of
  // the int32 deltas (the base is added once at the end), starting from
  // the lane's first event when it has one.
  int64_t local_max = 0;
  int64_t t0 = (int64_t)blockIdx.x * T;
  const bool seen = t0 + tid < n;
  if (t0 < n) {
    load_tile(t0);
    if (HASHED) local_max = (int64_t)rt[0];
  }
  for (; t0 < n; t0 += stride) {
    uint64_t pk[U];
    int sr[U];  // (rank << 13) | segment, or -1 when not placed
    // P1: classify, rank.
    if (!HASHED) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int64_t i = t0 + u * BLK + tid;
        int64_t t = (int64_t)rt[u] + ts_base;
        int64_t win = win_of(t, align_ms, len_ms, win_m2, win_maxfast);
        uint64_t packed =
            ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)rk[u];
        pk[u] = packed;
        int b = (int)region_of(mix64(packed), mask, seg_bits);
        sr[u] = -1;
        if (i < n) {
          if (t > local_max) local_max = t;
          sr[u] = (atomicAdd(&lhist[b], 1) << 13) | b;
        }
      }
    } else {
      // Events of this tile that lane `tid` holds, in steps of BLK.
      int64_t left64 = n - t0 - tid;
      const int left = left64 > T ? T : (left64 < 0 ? 0 : (int)left64);
      int32_t dmax = (int32_t)local_max;
      uint32_t rare = 0;  // events for the generic path
      // The histogram atomic is issued for every slot, with an
      // increment of 0 for the ones that are not placed: inside a
      // branch each of the U returning atomics is waited for on its
      // own, unconditional they are one batch.
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = u * BLK < left;
        const uint32_t d = (uint32_t)rt[u];
        const uint32_t q = win32_div(d + w32.c, w32);
        const uint64_t packed =
            ((uint64_t)(w32.wlo + q) << 32) | (uint32_t)rk[u];
        const uint64_t h64 = mix64(packed);
        const uint32_t delta = q - w32.qoff;
        const bool fits =
            d - w32.dlo < w32.dspan && delta < ENTRY_DELTA_LIMIT;
        pk[u] = ((uint64_t)(uint32_t)rk[u] << 32) |
                (uint64_t)(delta << ENTRY_SLOT_BITS) |
                ((h64 >> 32) & ENTRY_SLOT_MASK);
        if (in && !fits) rare |= 1u << u;
        if (in && (int32_t)d > dmax) dmax = (int32_t)d;
        const bool ok = in && fits;
        int b = (int)region_of(h64, mask, seg_bits);
        int rank = atomicAdd(&lhist[b], ok ? 1 : 0);
        sr[u] = ok ? ((rank << 13) | b) : -1;
      }
      local_max = dmax;
      // Rare: one copy of the generic window code, columns read again.
      while (rare != 0) {
        int u = __ffs(rare) - 1;
        rare &= rare - 1;
        int64_t i = t0 + u * BLK + tid;
        int64_t win = win_of((int64_t)ts[i] + ts_base, align_ms, len_ms,
                             win_m2, win_maxfast);
        spill(((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i]);
      }
    }
    if (t0 + stride < n) load_tile(t0 + stride);
    __syncthreads();
    // P2a: grants, cursor reservation, wave scan of the grants.
    int rc = 0, grant = 0, gb = 0;
    if (tid < nseg) {
      rc = res_cnt[tid];
      int tot = rc + lhist[tid];
      grant = tot & ~(SC_GRAN - 1);
      if (grant > 0) gb = atomicAdd(&gcursors[tid], grant);
      res_cnt[tid] = tot - grant;
      lhist[tid] = 0;
    }
    int incl = grant;
    for (int o = 1; o < WAVE; o <<= 1) {
      int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == WAVE - 1) s_wtot[wave] = incl;
    __syncthreads();
    // P2b: staging offsets, granule destinations, residual drain.
    int total = 0, woff = 0;
    for (int w = 0; w < NW; ++w) {
      int v = s_wtot[w];
      if (w < wave) woff += v;
      total += v;
    }
    if (tid < nseg) {
      int off = woff + incl - grant;
      lpack[tid] = off | (rc << 14) | (grant << 17);
      if (grant > 0) {
        // All seven residual slots, whatever rc is: the run holds at
        // least a granule, and P3 (behind the barrier) fills every
        // slot from rc up to the grant with an event of this tile.
#pragma unroll
        for (int j = 0; j < SC_GRAN - 1; ++j)
          stage[off + j] = res[(size_t)tid * SC_GRAN + j];
        for (int j = 0; j < grant; j += SC_GRAN) {
          int64_t gp = (int64_t)gb + j;
          gdst[(off + j) / SC_GRAN] =
              gp < cap ? (uint32_t)(((int64_t)tid * cap + gp) / SC_GRAN)
                       : GD_SPILL;
        }
      }
    }
    __syncthreads();
    // P3: place this tile's events (staged if granted, else residual).
    for (int u = 0; u < U; ++u) {
      if (sr[u] < 0) continue;
      int b = sr[u] & ((1 << 13) - 1);
      int w = lpack[b];
      int vpos = ((w >> 14) & 7) + (sr[u] >> 13);
      int g = w >> 17;
      if (vpos < g) stage[(w & ((1 << 14) - 1)) + vpos] = pk[u];
      else res[(size_t)b * SC_GRAN + (vpos - g)] = pk[u];
    }
    __syncthreads();
    // P4: copy-out.  Piece p is entries 2p, 2p+1; four adjacent lanes
    // cover one 64 B line of ev_packed.  The next tile's P1 touches
    // only lhist, and its P2b (the next writer of stage/gdst) lies
    // behind two barriers, so no barrier closes the tile.
    for (int p = tid; p < total / 2; p += BLK) {
      ulonglong2 v = *(const ulonglong2*)(stage + 2 * p);
      uint32_t d = gdst[p / 4];
      if (d != GD_SPILL) {
        *(ulonglong2*)(ev_packed + (int64_t)d * SC_GRAN + 2 * (p & 3)) = v;
      } else {
        if (v.x != EMPTY_SLOT) spill(classic_of(v.x));
        if (v.y != EMPTY_SLOT) spill(classic_of(v.y));
      }
    }
  }
  __syncthreads();
  // Final flush: sentinel-padded granules, like the default staged.
  if (tid < nseg) {
    int rc = res_cnt[tid];
    if (rc > 0) {
      int gb = atomicAdd(&gcursors[tid], SC_GRAN);
      for (int j = 0; j < SC_GRAN; ++j) {
        uint64_t p = j < rc ? res[(size_t)tid * SC_GRAN + j] : EMPTY_SLOT;
        int64_t gp = (int64_t)gb + j;
        if (gp < cap) ev_packed[(int64_t)tid * cap + gp] = p;
        else if (p != EMPTY_SLOT) spill(classic_of(p));
      }
    }
  }
  if (HASHED) local_max = seen ? local_max + ts_base : 0;
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// Compact-entry sibling of k_radix_scatter_staged2<int32, .., true>
// (ENTRY_FMT_COMPACT above): the same four phases per tile, with 4-byte
// `stage` and `res`.  A cursor reservation is still one 64-byte line,
// so the granule is 16 entries here: `cap`, grants and the cursor split
// are multiples of 16 and `lpack` carries 4 residual bits.  A P4 piece
// of 16 bytes is four entries, four adjacent lanes to a line as there.
// Segment b's entries live at ((uint32_t*)ev_packed)[b * cap ..], so
// the buffer is used at half its bytes.  An entry no longer carries its
// key: a granule that the capacity split sends to the spill keeps its
// segment index in gdst (GDC_SPILL | segment) so that P4 can rebuild
// classic `packed`, and the final flush knows its segment anyway.
// `dbits` is D; the host guarantees 2^(D+1) segments.
//
// A lane holds four consecutive events at a time: slot u = 4q + j of
// lane `tid` is event (q * BLK + tid) * 4 + j of the tile.  (Entries
// inside a segment are in atomic-arrival order anyway, and the
// aggregation counts.)  A full tile loads each column with U/4 loads of
// 16 bytes when VEC says both column pointers are 16-byte aligned, with
// unclamped dwords otherwise; the last, partial tile loads clamped
// dwords under the same mapping.
#define SCC_GRAN 16
typedef int32_t scc_i32x4 __attribute__((ext_vector_type(4)));
#define GDC_SPILL 0x80000000u

static inline size_t compact_lds_bytes(int64_t nseg, int64_t tile) {
  size_t stage_n = (size_t)(tile + (SCC_GRAN - 1) * nseg);  // multiple of 16
  return stage_n * 4                                // stage
         + (size_t)nseg * SCC_GRAN * 4              // res
         + 3 * (size_t)nseg * sizeof(int)           // res_cnt, lhist, lpack
         + (stage_n / SCC_GRAN) * sizeof(uint32_t);  // gdst
}

template <int U = 16, int BLK = 512, bool VEC = true>
__global__ __launch_bounds__(BLK) void k_radix_scatter_compact(
    const int32_t* __restrict__ keys,
    const int32_t* __restrict__ ts,
    int64_t n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int dbits,
    int64_t cap,
    int* __restrict__ gcursors,
    uint32_t* __restrict__ ev32,
    int* __restrict__ ov_cursor,
    uint64_t* __restrict__ ov_packed,
    int64_t ov_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    uint64_t win_m2,
    uint64_t win_maxfast,
    Win32 w32) {
  constexpr int T = BLK * U;
  constexpr int NW = BLK / WAVE;
  // lpack: staging offset (14 bits) | residual count (4) | grant (14).
  static_assert(T + (SCC_GRAN - 1) * BLK < (1 << 14),
                "staging offset must fit 14 bits");
  static_assert(T <= (1 << 13), "tile rank shares a word with the segment");
  static_assert(U % 4 == 0, "four consecutive events per lane");
  extern __shared__ __attribute__((aligned(16))) char smem_cc[];
  __shared__ int s_wtot[NW];
  const int nseg = 2 << dbits;  // host: nseg <= BLK
  const int nbits = 32 + dbits;
  const uint32_t dlimit = 1u << dbits;
  const uint32_t wbase = w32.wlo + w32.qoff;
  const int stage_n = T + (SCC_GRAN - 1) * nseg;
  uint32_t* stage = (uint32_t*)smem_cc;            // [stage_n]
  uint32_t* res = stage + stage_n;                 // [nseg][SCC_GRAN]
  int* res_cnt = (int*)(res + (size_t)nseg * SCC_GRAN);  // [nseg]
  int* lhist = res_cnt + nseg;                     // [nseg]
  uint32_t* lpack = (uint32_t*)(lhist + nseg);     // [nseg]
  uint32_t* gdst = lpack + nseg;                   // [stage_n / SCC_GRAN]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  if (tid < nseg) {
    res_cnt[tid] = 0;
    lhist[tid] = 0;
  }
  __syncthreads();

  // The spill holds classic `packed` whatever the entry format is.
  auto spill = [&](uint64_t packed) {
    int opos = atomicAdd(ov_cursor, 1);
    if (opos < ov_cap) ov_packed[opos] = packed;
    else atomicOr(error_flag, 1);
  };

  // Raw columns of one tile, loaded a tile ahead and held as the
  // 16-byte vectors they arrive in (slot u is rk[u / 4][u % 4]).
  // Whether the tile is full is uniform across the block.
  scc_i32x4 rk[U / 4];
  scc_i32x4 rt[U / 4];
  auto load_tile = [&](int64_t t0) {
    if (t0 + T <= n) {
      const int32_t* kp = keys + t0 + 4 * tid;
      const int32_t* tp = ts + t0 + 4 * tid;
#pragma unroll
      for (int q = 0; q < U / 4; ++q) {
        if (VEC) {
          rk[q] = *(const scc_i32x4*)(kp + q * BLK * 4);
          rt[q] = *(const scc_i32x4*)(tp + q * BLK * 4);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            rk[q][j] = kp[q * BLK * 4 + j];
            rt[q][j] = tp[q * BLK * 4 + j];
          }
        }
      }
    } else {
      const int last = (int)(n - 1 - t0);  // 0 <= last < T - 1
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int e = ((u >> 2) * BLK + tid) * 4 + (u & 3);
        if (e > last) e = last;
        rk[u >> 2][u & 3] = keys[t0 + e];
        rt[u >> 2][u & 3] = ts[t0 + e];
      }
    }
  };
  const int64_t stride = (int64_t)gridDim.x * T;
  // Maximum of the int32 deltas (the base is added once at the end),
  // starting from the lane's first slot.  A slot past the end of the
  // batch holds a copy of the batch's last event (the clamped load),
  // which cannot raise the batch's maximum, so every slot of a block
  // that has a tile takes part and no `in` test is needed.
  int64_t local_max = 0;
  int64_t t0 = (int64_t)blockIdx.x * T;
  const bool seen = t0 < n;
  if (t0 < n) {
    load_tile(t0);
    local_max = (int64_t)rt[0][0];
  }
  for (; t0 < n; t0 += stride) {
    uint32_t pk[U];
    int sr[U];  // (rank << 13) | segment, or -1 when not placed
    // P1: classify, rank.  Slot u holds an event of this tile when its
    // offset from the lane's first event lies below `left`.
    const int64_t rem = n - t0;
    const int left = (rem > T ? T : (int)rem) - 4 * tid;
    int32_t dmax = (int32_t)local_max;
    uint32_t rare = 0;  // events for the generic path
    // Unconditional histogram atomics, one batch (see staged2).
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = (u >> 2) * BLK * 4 + (u & 3) < left;
      const uint32_t d = (uint32_t)rt[u >> 2][u & 3];
      const uint32_t q = win32_div(d + w32.c, w32);
      const uint32_t delta = q - w32.qoff;
      const bool fits = d - w32.dlo < w32.dspan && delta < dlimit;
      uint32_t lo = (uint32_t)rk[u >> 2][u & 3];
      uint32_t hi = delta & (dlimit - 1);
      mixn_pair(lo, hi, nbits);
      pk[u] = lo & 0x7FFFFFFFu;
      if (in && !fits) rare |= 1u << u;
      if ((int32_t)d > dmax) dmax = (int32_t)d;
      // `ok` is spent before the atomics return: all ones in place of
      // the segment make the whole word -1.  The empty asm keeps the
      // compiler from turning that back into a select on `ok`, which
      // would hold a lane mask per slot across the batch of atomics.
      const bool ok = in && fits;
      int b = (int)((hi << 1) | (lo >> 31));  // < 2^(dbits+1) = nseg
      int bm = ok ? b : -1;
      asm("" : "+v"(bm));
      int rank = atomicAdd(&lhist[b], ok ? 1 : 0);
      sr[u] = (rank << 13) | bm;
    }
    local_max = dmax;
    // Rare: one copy of the generic window code, columns read again.
    while (rare != 0) {
      int u = __ffs(rare) - 1;
      rare &= rare - 1;
      int64_t i = t0 + ((u >> 2) * BLK + tid) * 4 + (u & 3);
      int64_t win = win_of((int64_t)ts[i] + ts_base, align_ms, len_ms,
                           win_m2, win_maxfast);
      spill(((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i]);
    }
    if (t0 + stride < n) load_tile(t0 + stride);
    __syncthreads();
    // P2a: grants, cursor reservation, wave scan of the grants.
    int rc = 0, grant = 0, gb = 0;
    if (tid < nseg) {
      rc = res_cnt[tid];
      int tot = rc + lhist[tid];
      grant = tot & ~(SCC_GRAN - 1);
      if (grant > 0) gb = atomicAdd(&gcursors[tid], grant);
      res_cnt[tid] = tot - grant;
      lhist[tid] = 0;
    }
    int incl = grant;
    for (int o = 1; o < WAVE; o <<= 1) {
      int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == WAVE - 1) s_wtot[wave] = incl;
    __syncthreads();
    // P2b: staging offsets, granule destinations, residual drain.
    int total = 0, woff = 0;
    for (int w = 0; w < NW; ++w) {
      int v = s_wtot[w];
      if (w < wave) woff += v;
      total += v;
    }
    const int off = woff + incl - grant;
    // Residual drain, a wave for its own 64 segments, four segments a
    // step: 16 adjacent lanes move one segment's slots, so `res` is read
    // along the banks and `stage` written in runs of 16 dwords.  (One
    // thread per segment walking its 15 slots reads and writes at a
    // stride of 64 bytes, every lane on the same few banks.)  All
    // fifteen slots, whatever rc is (see staged2).  nseg is a multiple
    // of 64, so the condition is wave-uniform.
    if (wave * WAVE < nseg) {
      const int og = grant > 0 ? off : -1;
      for (int k = 0; k < WAVE / 4; ++k) {
        const int src = k * 4 + (lane >> 4);
        const int o = __shfl(og, src);
        const int j = lane & (SCC_GRAN - 1);
        if (o >= 0 && j < SCC_GRAN - 1)
          stage[o + j] = res[(size_t)(wave * WAVE + src) * SCC_GRAN + j];
      }
    }
    if (tid < nseg) {
      lpack[tid] = (uint32_t)off | ((uint32_t)rc << 14) |
                   ((uint32_t)grant << 18);
      if (grant > 0) {
        for (int j = 0; j < grant; j += SCC_GRAN) {
          int64_t gp = (int64_t)gb + j;
          gdst[(off + j) / SCC_GRAN] =
              gp < cap ? (uint32_t)(((int64_t)tid * cap + gp) / SCC_GRAN)
                       : (GDC_SPILL | (uint32_t)tid);
        }
      }
    }
    __syncthreads();
    // P3: place this tile's events (staged if granted, else residual).
    for (int u = 0; u < U; ++u) {
      if (sr[u] < 0) continue;
      int b = sr[u] & ((1 << 13) - 1);
      uint32_t w = lpack[b];
      int vpos = (int)((w >> 14) & 15u) + (sr[u] >> 13);
      int g = (int)(w >> 18);
      if (vpos < g) stage[(w & ((1u << 14) - 1)) + vpos] = pk[u];
      else res[(size_t)b * SCC_GRAN + (vpos - g)] = pk[u];
    }
    __syncthreads();
    // P4: copy-out.  Piece p is entries 4p .. 4p+3; four adjacent lanes
    // cover one 64 B line.  No barrier closes the tile (see staged2).
    for (int p = tid; p < total / 4; p += BLK) {
      uint4 v = *(const uint4*)(stage + 4 * p);
      uint32_t d = gdst[p / 4];
      if ((d & GDC_SPILL) == 0) {
        *(uint4*)(ev32 + (int64_t)d * SCC_GRAN + 4 * (p & 3)) = v;
      } else {
        const uint32_t seg = d & ~GDC_SPILL;
        const uint32_t e[4] = {v.x, v.y, v.z, v.w};
        for (int j = 0; j < 4; ++j)
          if (e[j] != ENTRY_PAD32)
            spill(compact_classic(seg, e[j], nbits, wbase));
      }
    }
  }
  __syncthreads();
  // Final flush: pad-filled granules, like the default staged.
  if (tid < nseg) {
    int rc = res_cnt[tid];
    if (rc > 0) {
      int gb = atomicAdd(&gcursors[tid], SCC_GRAN);
      for (int j = 0; j < SCC_GRAN; ++j) {
        uint32_t e = j < rc ? res[(size_t)tid * SCC_GRAN + j] : ENTRY_PAD32;
        int64_t gp = (int64_t)gb + j;
        if (gp < cap) ev32[(int64_t)tid * cap + gp] = e;
        else if (e != ENTRY_PAD32)
          spill(compact_classic((uint32_t)tid, e, nbits, wbase));
      }
    }
  }
  local_max = seen ? local_max + ts_base : 0;
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// Aggregate the overflow spill straight into the table (tiny for
// uniform keys).  `spill_total` (may be null) is a running total of
// the spilled events, which the state reads at a close to see whether
// a stream lives on this slow path; launches on one table are ordered,
// so one thread adds with a plain add.
template <int MODE>
__global__ void k_overflow_agg(
    const uint64_t* __restrict__ ov_packed,
    const int64_t* __restrict__ ov_vals,
    const int* __restrict__ ov_cursor,
    int64_t ov_cap,
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int region_bits,
    int* __restrict__ error_flag,
    unsigned long long* __restrict__ spill_total) {
  int64_t n = *ov_cursor;
  if (n > ov_cap) n = ov_cap;
  if (spill_total != nullptr && blockIdx.x == 0 && threadIdx.x == 0 && n > 0)
    *spill_total += (unsigned long long)n;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    unsigned long long inc =
        (MODE == AGG_SUM) ? (unsigned long long)ov_vals[i] : 1ULL;
    if (!hash_add(tkeys, tvals, mask, region_bits, ov_packed[i], inc)) {
      atomicOr(error_flag, 1);
    }
  }
}

// 16-byte view of two adjacent packed entries (one vector load).
typedef unsigned long long agg_u64x2 __attribute__((ext_vector_type(2)));

// Segment aggregation: one workgroup folds one scatter segment into an
// LDS open-address table, then flushes each distinct key once.
//
// The segment is streamed with a register double buffer: every thread
// keeps R independent 16-byte loads (two packed entries each) of chunk
// i+1 in flight while it probes chunk i, so a 1024-thread block has
// R * 16 KiB of HBM reads outstanding instead of one 8-byte load per
// lane (the probe loop's data-dependent exits keep the compiler from
// hoisting loads on its own).  A segment that starts only 8-byte
// aligned (fixed layout, odd `cap`) peels one head entry, and an odd
// remainder one tail entry, so no vector load is ever misaligned or
// reaches past `min(count, cap)`.
template <int MODE>
__global__ __launch_bounds__(1024) void k_radix_agg(
    const uint64_t* __restrict__ ev_packed,
    const int64_t* __restrict__ ev_vals,
    const int* __restrict__ counts,
    int64_t cap,  // segment stride: segment b owns [b*cap, (b+1)*cap);
                  // counts past it went to the overflow spill
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int region_bits,
    int lds_bits,  // LDS staging-table slots (>= region_bits when one
                   // scatter segment spans several table regions)
    int* __restrict__ error_flag) {
  extern __shared__ char smem[];
  int region = 1 << lds_bits;
  uint64_t* lkeys = (uint64_t*)smem;
  unsigned long long* lvals =
      (unsigned long long*)(smem + (size_t)region * sizeof(uint64_t));
  for (int s = threadIdx.x; s < region; s += blockDim.x) {
    lkeys[s] = EMPTY_SLOT;
    lvals[s] = 0;
  }
  __syncthreads();
  int b = blockIdx.x;
  int cnt = counts[b];
  if (cnt > (int)cap) cnt = (int)cap;
  const uint64_t* seg = ev_packed + (int64_t)b * cap;
  const int64_t* segv =
      (MODE == AGG_SUM) ? ev_vals + (int64_t)b * cap : nullptr;

  auto add = [&](uint64_t packed, unsigned long long inc) {
    if (packed == EMPTY_SLOT) return;  // staged-scatter pad
    uint64_t h64 = mix64(packed);
    int lh = (int)((h64 >> 32) & (region - 1));
    bool done = false;
    for (int p = 0; p < region; ++p) {
      uint64_t cur = lkeys[lh];
      if (cur == packed) {
        atomicAdd(&lvals[lh], inc);
        done = true;
        break;
      }
      if (cur == EMPTY_SLOT) {
        uint64_t prev = atomicCAS(
            (unsigned long long*)&lkeys[lh], EMPTY_SLOT, packed);
        if (prev == EMPTY_SLOT || prev == packed) {
          atomicAdd(&lvals[lh], inc);
          done = true;
          break;
        }
      }
      lh = (lh + 1) & (region - 1);
    }
    if (!done) {
      // LDS staging full (only possible when the global regions are
      // at least as full): flush straight to the global region.
      if (!hash_add(tkeys, tvals, mask, region_bits, packed, inc)) {
        atomicOr(error_flag, 1);
      }
    }
  };

  // Head/tail entries outside the 16-byte-aligned vector body.
  const int head = (cnt > 0 && ((uintptr_t)seg & 15) != 0) ? 1 : 0;
  const int nvec = (cnt - head) >> 1;
  const int tail = head + 2 * nvec;  // == cnt or cnt - 1
  if (threadIdx.x == 0 && head) {
    add(seg[0], MODE == AGG_SUM ? (unsigned long long)segv[0] : 1ULL);
  }
  if (threadIdx.x == blockDim.x - 1 && tail < cnt) {
    add(seg[tail],
        MODE == AGG_SUM ? (unsigned long long)segv[tail] : 1ULL);
  }

  // SUM carries the two values next to each pair, so it keeps half the
  // depth to stay inside the 128-VGPR budget of a 1024-thread block.
  constexpr int R = (MODE == AGG_SUM) ? 2 : 4;
  const agg_u64x2* vseg = (const agg_u64x2*)(seg + head);
  const int64_t* vval = (MODE == AGG_SUM) ? segv + head : nullptr;
  const int T = (int)blockDim.x;
  const int chunk = R * T;
  agg_u64x2 cur_p[R], nxt_p[R];
  unsigned long long cur_v[R][2], nxt_v[R][2];
  auto fetch = [&](agg_u64x2 (&bp)[R], unsigned long long (&bv)[R][2],
                   int base) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int v = base + r * T + (int)threadIdx.x;
      if (v < nvec) {
        bp[r] = vseg[v];
        if (MODE == AGG_SUM) {
          bv[r][0] = (unsigned long long)vval[2 * v];
          bv[r][1] = (unsigned long long)vval[2 * v + 1];
        }
      } else {
        bp[r] = agg_u64x2{EMPTY_SLOT, EMPTY_SLOT};
        if (MODE == AGG_SUM) bv[r][0] = bv[r][1] = 0;
      }
    }
  };
  if (nvec > 0) fetch(cur_p, cur_v, 0);
  for (int base = 0; base < nvec; base += chunk) {
    // Issue the next chunk's loads before touching the LDS table.
    if (base + chunk < nvec) fetch(nxt_p, nxt_v, base + chunk);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      add(cur_p[r].x, MODE == AGG_SUM ? cur_v[r][0] : 1ULL);
      add(cur_p[r].y, MODE == AGG_SUM ? cur_v[r][1] : 1ULL);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cur_p[r] = nxt_p[r];
      if (MODE == AGG_SUM) {
        cur_v[r][0] = nxt_v[r][0];
        cur_v[r][1] = nxt_v[r][1];
      }
    }
  }
  __syncthreads();
  // Flush distinct keys once into each key's own table region (the
  // segment's regions are contiguous in HBM, so flushes stay local).
  for (int s = threadIdx.x; s < region; s += blockDim.x) {
    if (lkeys[s] != EMPTY_SLOT) {
      if (!hash_add(tkeys, tvals, mask, region_bits, lkeys[s], lvals[s])) {
        atomicOr(error_flag, 1);
      }
    }
  }
}

// Window deltas a compact cell can hold (the delta nibble 15 is left
// to the empty marker), and where the segment's first window sits in
// that range.
#define AGG_DELTA_MAX 14u
#define AGG_DELTA_MID 7u

// COUNT segment aggregation with 8-byte LDS cells.
//
// Same contract as k_radix_agg<AGG_COUNT> (`ev_packed` / `counts` /
// `cap`, head and tail peeling, EMPTY_SLOT pads, register double
// buffer of 16-byte loads), half the LDS: a cell is
//   key32 (high dword) | window delta (4 bits) | count (28 bits)
// so the table of a 2^13-slot segment is 64 KiB and two workgroups
// share a CU: one clears or flushes while the other streams.  The
// delta is taken against a block-uniform base (the window of the
// segment's first entry minus AGG_DELTA_MID) and restricted to
// 0..AGG_DELTA_MAX, so no valid cell, whatever its key, equals the
// all-ones empty marker; an entry outside that range goes straight to
// the global table, which is exact.  A cell is claimed by a 64-bit CAS
// of empty -> (key, delta, count 0) and counted with a 32-bit add on
// the low dword; the host takes this kernel only when `cap` < 2^28, so
// a count never carries into the delta.
//
// The first probe of a chunk's 2R entries is batched: all slot indices
// are computed and all cells read before the first wait, and entries
// whose cell already carries their tag add at once.  What is left (a
// cell to claim, a collision, a window out of range) goes through ONE
// probe / CAS loop per chunk, in which every lane works through its own
// leftovers one probe step at a time.  A wave then waits for the LDS
// about once per chunk plus once per probe step of its busiest lane,
// where a probe loop per entry waits for the longest chain among 64
// lanes 2R times over.
//
// HASHED: the segment holds hashed entries (ENTRY_* above) against the
// entry base whose low 32 bits are `wlo`.  The LDS slot is the entry's
// low bits, the window delta its 19-bit field, and mix64 runs only in
// hash_add, on the classic `packed` rebuilt for an escape or a flush.
template <int BLK, int R, bool HASHED = false>
__global__ __launch_bounds__(BLK, BLK == 1024 ? 8 : 4) void k_radix_agg_count(
    const uint64_t* __restrict__ ev_packed,
    const int* __restrict__ counts,
    int64_t cap,
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int region_bits,
    int lds_bits,
    int* __restrict__ error_flag,
    uint32_t wlo) {
  extern __shared__ char smem[];
  unsigned long long* cells = (unsigned long long*)smem;
  const int region = 1 << lds_bits;
  const uint32_t lmask = (uint32_t)region - 1;
  const int b = blockIdx.x;
  int cnt = counts[b];
  if (cnt > (int)cap) cnt = (int)cap;
  if (cnt <= 0) return;  // block-uniform
  for (int s = threadIdx.x; s < region / 2; s += BLK) {
    ((agg_u64x2*)cells)[s] = agg_u64x2{EMPTY_SLOT, EMPTY_SLOT};
  }
  const uint64_t* seg = ev_packed + (int64_t)b * cap;
  // Any base is correct; this one puts the first entry's window in the
  // middle of the range.
  // An entry's window (classic) or window delta (hashed), and its key.
  auto win_part = [&](uint64_t packed) {
    return HASHED ? entry_delta(packed) : (uint32_t)(packed >> 32);
  };
  auto key_part = [&](uint64_t packed) {
    return HASHED ? (uint32_t)(packed >> 32) : (uint32_t)packed;
  };
  const uint32_t wbase = win_part(seg[0]) - AGG_DELTA_MID;
  __syncthreads();

  auto escape = [&](uint64_t packed) {
    if (HASHED) packed = entry_classic(packed, wlo);
    if (!hash_add(tkeys, tvals, mask, region_bits, packed, 1ULL)) {
      atomicOr(error_flag, 1);
    }
  };
  auto slot_of = [&](uint64_t packed) {
    if (HASHED) return (uint32_t)packed & lmask;
    return (uint32_t)(mix64(packed) >> 32) & lmask;
  };
  // key | delta, as it stands in the upper 36 bits of a cell.
  auto tag_of = [&](uint64_t packed) {
    return ((unsigned long long)key_part(packed) << 4) |
           (unsigned long long)(win_part(packed) - wbase);
  };
  // Probe / claim loop over a lane's leftovers: the source of truth.
  // `pend` has one bit per entry; `entry(e)` and `start(e)` give the
  // packed value and the first slot to look at, `skipped(e)` says
  // whether the entry's home slot has been ruled out already.
  auto drain = [&](uint32_t pend, auto entry, auto start, auto skipped) {
    uint64_t packed = 0;
    unsigned long long tag = 0;
    uint32_t lh = 0;
    int left = 0;  // probe steps before the table counts as full
    while (left != 0 || pend != 0) {
      if (left == 0) {
        int e = __ffs(pend) - 1;
        pend &= pend - 1;
        packed = entry(e);
        if (win_part(packed) - wbase > AGG_DELTA_MAX) {
          escape(packed);
          continue;
        }
        tag = tag_of(packed);
        lh = start(e);
        left = region - (skipped(e) ? 1 : 0);
      }
      unsigned long long cur = cells[lh];
      if (cur == EMPTY_SLOT) {
        cur = atomicCAS(&cells[lh], EMPTY_SLOT, tag << 28);
        if (cur == EMPTY_SLOT) cur = tag << 28;
      }
      if ((cur >> 28) == tag) {
        atomicAdd((unsigned int*)&cells[lh], 1u);
        left = 0;
      } else {
        lh = (lh + 1) & lmask;
        if (--left == 0) escape(packed);  // LDS table full
      }
    }
  };
  auto add_one = [&](uint64_t packed) {
    if (packed == EMPTY_SLOT) return;  // staged-scatter pad
    drain(
        1u, [&](int) { return packed; },
        [&](int) { return slot_of(packed); }, [&](int) { return false; });
  };

  // Head/tail entries outside the 16-byte-aligned vector body.
  const int head = ((uintptr_t)seg & 15) != 0 ? 1 : 0;
  const int nvec = (cnt - head) >> 1;
  const int tail = head + 2 * nvec;  // == cnt or cnt - 1
  if (threadIdx.x == 0 && head) add_one(seg[0]);
  if (threadIdx.x == BLK - 1 && tail < cnt) add_one(seg[tail]);

  const agg_u64x2* vseg = (const agg_u64x2*)(seg + head);
  constexpr int chunk = R * BLK;
  constexpr int E = 2 * R;
  agg_u64x2 cur_p[R], nxt_p[R];
  auto fetch = [&](agg_u64x2 (&bp)[R], int base) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int v = base + r * BLK + (int)threadIdx.x;
      if (v < nvec) bp[r] = vseg[v];
      else bp[r] = agg_u64x2{EMPTY_SLOT, EMPTY_SLOT};
    }
  };
  fetch(cur_p, 0);
  for (int base = 0; base < nvec; base += chunk) {
    // Issue the next chunk's loads before touching the LDS table.
    if (base + chunk < nvec) fetch(nxt_p, base + chunk);
    uint32_t slot[E];
    unsigned long long first[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      uint64_t packed = (e & 1) ? cur_p[e >> 1].y : cur_p[e >> 1].x;
      slot[e] = slot_of(packed);
      first[e] = cells[slot[e]];
    }
    uint32_t pend = 0, moved = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      uint64_t packed = (e & 1) ? cur_p[e >> 1].y : cur_p[e >> 1].x;
      if (packed == EMPTY_SLOT) continue;  // staged-scatter pad
      bool in_range = win_part(packed) - wbase <= AGG_DELTA_MAX;
      if (in_range && (first[e] >> 28) == tag_of(packed)) {
        atomicAdd((unsigned int*)&cells[slot[e]], 1u);
      } else {
        pend |= 1u << e;
        if (first[e] != EMPTY_SLOT) {
          // Another cell's: start one further on.
          slot[e] = (slot[e] + 1) & lmask;
          moved |= 1u << e;
        }
      }
    }
    if (pend != 0) {
      drain(
          pend,
          [&](int e) {
            uint64_t v = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
              if (j == e) v = (j & 1) ? cur_p[j >> 1].y : cur_p[j >> 1].x;
            }
            return v;
          },
          [&](int e) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
              if (j == e) v = slot[j];
            }
            return v;
          },
          [&](int e) { return ((moved >> e) & 1u) != 0; });
    }
#pragma unroll
    for (int r = 0; r < R; ++r) cur_p[r] = nxt_p[r];
  }
  __syncthreads();

  // Flush each cell once into its key's own table region (the
  // segment's regions are contiguous in HBM, so flushes stay local).
  for (int s = threadIdx.x; s < region; s += BLK) {
    unsigned long long c = cells[s];
    if (c != EMPTY_SLOT) {
      uint32_t win = wbase + ((uint32_t)c >> 28) + (HASHED ? wlo : 0u);
      uint64_t packed = ((uint64_t)win << 32) | (c >> 32);
      if (!hash_add(tkeys, tvals, mask, region_bits, packed,
                    c & 0x0FFFFFFFULL)) {
        atomicOr(error_flag, 1);
      }
    }
  }
}

// COUNT segment aggregation for compact entries (ENTRY_FMT_COMPACT).
//
// The structure of k_radix_agg_count with 4-byte entries: a register
// double buffer of R 16-byte loads (four entries each), head and tail
// peeling of up to three entries, the first probe of a chunk's 4R
// entries batched, one probe / CAS loop per chunk for what is left.
// A cell is entry << 32 | count32 and all-ones is empty: bit 31 of an
// entry is 0, so no cell equals it.  The entry is the whole tag (the
// block's segment index supplies the rest of the hash), the slot its
// top `lds_bits` bits; there is no window range, and an entry goes
// straight to the table only when the LDS table is full.  The flush
// inverts the mixer once per cell to rebuild classic `packed` for
// hash_add.  Segments are slices of the mixn hash, not of the table:
// the flush of a block lands anywhere in the table, which hash_add's
// atomics make correct.
template <int BLK, int R>
__global__ __launch_bounds__(BLK, BLK == 1024 ? 8 : 4) void k_radix_agg_compact(
    const uint32_t* __restrict__ ev32,
    const int* __restrict__ counts,
    int64_t cap,
    uint64_t* __restrict__ tkeys,
    unsigned long long* __restrict__ tvals,
    uint64_t mask,
    int region_bits,
    int lds_bits,
    int* __restrict__ error_flag,
    uint32_t wbase,
    int dbits) {
  extern __shared__ char smem[];
  unsigned long long* cells = (unsigned long long*)smem;
  const int region = 1 << lds_bits;
  const uint32_t lmask = (uint32_t)region - 1;
  const int sshift = 31 - lds_bits;
  const int nbits = 32 + dbits;
  const int b = blockIdx.x;
  int cnt = counts[b];
  if (cnt > (int)cap) cnt = (int)cap;
  if (cnt <= 0) return;  // block-uniform
  for (int s = threadIdx.x; s < region / 2; s += BLK) {
    ((agg_u64x2*)cells)[s] = agg_u64x2{EMPTY_SLOT, EMPTY_SLOT};
  }
  const uint32_t* seg = ev32 + (int64_t)b * cap;
  __syncthreads();

  auto escape = [&](uint32_t e) {
    if (!hash_add(tkeys, tvals, mask, region_bits,
                  compact_classic((uint32_t)b, e, nbits, wbase), 1ULL)) {
      atomicOr(error_flag, 1);
    }
  };
  // Probe / claim loop over a lane's leftovers (see k_radix_agg_count).
  auto drain = [&](uint32_t pend, auto entry, auto start, auto skipped) {
    uint32_t tag = 0;
    uint32_t lh = 0;
    int left = 0;  // probe steps before the table counts as full
    while (left != 0 || pend != 0) {
      if (left == 0) {
        int e = __ffs(pend) - 1;
        pend &= pend - 1;
        tag = entry(e);
        lh = start(e);
        left = region - (skipped(e) ? 1 : 0);
      }
      unsigned long long cur = cells[lh];
      if (cur == EMPTY_SLOT) {
        cur = atomicCAS(&cells[lh], EMPTY_SLOT,
                        (unsigned long long)tag << 32);
        if (cur == EMPTY_SLOT) cur = (unsigned long long)tag << 32;
      }
      if ((uint32_t)(cur >> 32) == tag) {
        atomicAdd((unsigned int*)&cells[lh], 1u);
        left = 0;
      } else {
        lh = (lh + 1) & lmask;
        if (--left == 0) escape(tag);  // LDS table full
      }
    }
  };
  auto add_one = [&](uint32_t e) {
    if (e == ENTRY_PAD32) return;  // scatter pad
    drain(
        1u, [&](int) { return e; }, [&](int) { return e >> sshift; },
        [&](int) { return false; });
  };

  // Head/tail entries outside the 16-byte-aligned vector body.
  int head = (int)(((16 - ((uintptr_t)seg & 15)) & 15) >> 2);
  if (head > cnt) head = cnt;
  const int nvec = (cnt - head) >> 2;
  const int tail = head + 4 * nvec;  // cnt - 3 .. cnt
  if (threadIdx.x == 0)
    for (int j = 0; j < head; ++j) add_one(seg[j]);
  if (threadIdx.x == BLK - 1)
    for (int j = tail; j < cnt; ++j) add_one(seg[j]);

  const uint4* vseg = (const uint4*)(seg + head);
  constexpr int chunk = R * BLK;
  constexpr int E = 4 * R;
  uint4 cur_p[R], nxt_p[R];
  auto fetch = [&](uint4 (&bp)[R], int base) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int v = base + r * BLK + (int)threadIdx.x;
      if (v < nvec) bp[r] = vseg[v];
      else bp[r] = uint4{ENTRY_PAD32, ENTRY_PAD32, ENTRY_PAD32, ENTRY_PAD32};
    }
  };
  auto pick = [&](int e) {
    const uint4& q = cur_p[e >> 2];
    return (e & 3) == 0 ? q.x : (e & 3) == 1 ? q.y : (e & 3) == 2 ? q.z : q.w;
  };
  fetch(cur_p, 0);
  for (int base = 0; base < nvec; base += chunk) {
    // Issue the next chunk's loads before touching the LDS table.
    if (base + chunk < nvec) fetch(nxt_p, base + chunk);
    uint32_t slot[E];
    unsigned long long first[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      // A pad's slot is in range as well (bit 31 is shifted in).
      slot[e] = (pick(e) >> sshift) & lmask;
      first[e] = cells[slot[e]];
    }
    uint32_t pend = 0, moved = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      uint32_t en = pick(e);
      if (en == ENTRY_PAD32) continue;  // scatter pad
      if ((uint32_t)(first[e] >> 32) == en) {
        atomicAdd((unsigned int*)&cells[slot[e]], 1u);
      } else {
        pend |= 1u << e;
        if (first[e] != EMPTY_SLOT) {
          // Another cell's: start one further on.
          slot[e] = (slot[e] + 1) & lmask;
          moved |= 1u << e;
        }
      }
    }
    if (pend != 0) {
      drain(
          pend,
          [&](int e) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
              if (j == e) v = pick(j);
            }
            return v;
          },
          [&](int e) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
              if (j == e) v = slot[j];
            }
            return v;
          },
          [&](int e) { return ((moved >> e) & 1u) != 0; });
    }
#pragma unroll
    for (int r = 0; r < R; ++r) cur_p[r] = nxt_p[r];
  }
  __syncthreads();

  // Flush each cell once: invert the mixer, rebuild `packed`.
  for (int s = threadIdx.x; s < region; s += BLK) {
    unsigned long long c = cells[s];
    if (c != EMPTY_SLOT) {
      if (!hash_add(tkeys, tvals, mask, region_bits,
                    compact_classic((uint32_t)b, (uint32_t)(c >> 32), nbits,
                                    wbase),
                    c & 0xFFFFFFFFULL)) {
        atomicOr(error_flag, 1);
      }
    }
  }
}

// Overflow spill for the stats table (direct contended path).
__global__ void k_overflow_agg_stats(
    const uint64_t* __restrict__ ov_packed,
    const int64_t* __restrict__ ov_vals,
    const int* __restrict__ ov_cursor,
    int64_t ov_cap,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tcnt,
    long long* __restrict__ tsum,
    long long* __restrict__ tmin,
    long long* __restrict__ tmax,
    uint64_t mask,
    int* __restrict__ error_flag) {
  int64_t n = *ov_cursor;
  if (n > ov_cap) n = ov_cap;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    uint64_t slot = find_slot(tkeys, mask, ov_packed[i]);
    if (slot == ~0ULL) {
      atomicOr(error_flag, 1);
      continue;
    }
    long long v = ov_vals[i];
    atomicAdd((unsigned long long*)&tcnt[slot], 1ULL);
    atomicAdd((unsigned long long*)&tsum[slot], (unsigned long long)v);
    atomicMin(&tmin[slot], v);
    atomicMax(&tmax[slot], v);
  }
}

// Radix aggregation for the 4-accumulator stats table (count / sum /
// min / max): one workgroup per region, LDS-resident accumulators,
// one flush per distinct cell.  Events must already be partitioned
// (k_radix_scatter with values).
__global__ __launch_bounds__(1024) void k_radix_agg_stats(
    const uint64_t* __restrict__ ev_packed,
    const int64_t* __restrict__ ev_vals,
    const int* __restrict__ offsets,
    const int* __restrict__ counts,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tcnt,
    long long* __restrict__ tsum,
    long long* __restrict__ tmin,
    long long* __restrict__ tmax,
    int64_t clamp_cap,
    uint64_t mask,
    int region_bits,
    int lds_bits,  // LDS staging slots (>= region_bits for coarse segments)
    int* __restrict__ error_flag) {
  extern __shared__ char smem[];
  int region = 1 << lds_bits;
  uint64_t* lkeys = (uint64_t*)smem;
  long long* lcnt = (long long*)(smem + (size_t)region * 8);
  long long* lsum = (long long*)(smem + (size_t)region * 16);
  long long* lmin = (long long*)(smem + (size_t)region * 24);
  long long* lmax = (long long*)(smem + (size_t)region * 32);
  const long long LLMAX = 0x7FFFFFFFFFFFFFFFLL;
  for (int s = threadIdx.x; s < region; s += blockDim.x) {
    lkeys[s] = EMPTY_SLOT;
    lcnt[s] = 0;
    lsum[s] = 0;
    lmin[s] = LLMAX;
    lmax[s] = -LLMAX - 1;
  }
  __syncthreads();
  int b = blockIdx.x;
  int cnt = counts[b];
  if (clamp_cap > 0 && cnt > (int)clamp_cap) cnt = (int)clamp_cap;
  int start = offsets[b];
  for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
    uint64_t packed = ev_packed[start + j];
    if (packed == EMPTY_SLOT) continue;  // staged-scatter pad
    long long v = ev_vals[start + j];
    uint64_t h64 = mix64(packed);
    int lh = (int)((h64 >> 32) & (region - 1));
    int slot = -1;
    for (int p = 0; p < region; ++p) {
      uint64_t cur = lkeys[lh];
      if (cur == packed) {
        slot = lh;
        break;
      }
      if (cur == EMPTY_SLOT) {
        uint64_t prev = atomicCAS(
            (unsigned long long*)&lkeys[lh], EMPTY_SLOT, packed);
        if (prev == EMPTY_SLOT || prev == packed) {
          slot = lh;
          break;
        }
      }
      lh = (lh + 1) & (region - 1);
    }
    if (slot >= 0) {
      atomicAdd((unsigned long long*)&lcnt[slot], 1ULL);
      atomicAdd((unsigned long long*)&lsum[slot], (unsigned long long)v);
      atomicMin(&lmin[slot], v);
      atomicMax(&lmax[slot], v);
    } else {
      // LDS region full: fall through to the global region directly.
      uint64_t gslot = find_slot(tkeys, mask, packed);
      if (gslot == ~0ULL) {
        atomicOr(error_flag, 1);
      } else {
        atomicAdd((unsigned long long*)&tcnt[gslot], 1ULL);
        atomicAdd((unsigned long long*)&tsum[gslot], (unsigned long long)v);
        atomicMin(&tmin[gslot], v);
        atomicMax(&tmax[gslot], v);
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < region; s += blockDim.x) {
    if (lkeys[s] != EMPTY_SLOT) {
      uint64_t gslot = find_slot(tkeys, mask, lkeys[s]);
      if (gslot == ~0ULL) {
        atomicOr(error_flag, 1);
        continue;
      }
      atomicAdd((unsigned long long*)&tcnt[gslot],
                (unsigned long long)lcnt[s]);
      atomicAdd((unsigned long long*)&tsum[gslot],
                (unsigned long long)lsum[s]);
      atomicMin(&tmin[gslot], lmin[s]);
      atomicMax(&tmax[gslot], lmax[s]);
    }
  }
}

// Extract all slots whose window id is in [win_lo, win_hi) WITHOUT
// mutating the table.  Deleting slots in place is forbidden: it breaks
// open-addressing probe chains for keys displaced past the cleared
// slot (a later re-insert of such a key would claim its home slot and
// duplicate the cell).  Reclamation happens via k_close_migrate.
// Output compaction: wave ballot + one atomic per wave, lanes write at
// their popcount rank.
__global__ void k_close_extract(
    const uint64_t* __restrict__ tkeys,
    const unsigned long long* __restrict__ tvals,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t cap) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < nslots; i += stride) {
    uint64_t k = tkeys[i];
    bool take = false;
    int32_t win = 0;
    if (k != EMPTY_SLOT) {
      win = (int32_t)(uint32_t)(k >> 32);
      take = (int64_t)win >= win_lo && (int64_t)win < win_hi;
    }
    unsigned long long ball = __ballot(take);
    int lane = threadIdx.x & (WAVE - 1);
    if (ball != 0) {
      int wave_total = __popcll(ball);
      int rank = __popcll(ball & ((1ULL << lane) - 1ULL));
      int base = 0;
      int lead = __ffsll((unsigned long long)ball) - 1;
      if (lane == lead) base = atomicAdd(out_n, wave_total);
      base = __shfl(base, lead);
      if (take) {
        int64_t idx = base + rank;
        if (idx < cap) {
          out_keys[idx] = (int32_t)(uint32_t)(k & 0xFFFFFFFFULL);
          out_wins[idx] = win;
          out_vals[idx] = (int64_t)tvals[i];
        }
      }
    }
  }
}

// Window close with reclamation: emit cells below `win_hi` and
// migrate the still-open cells into a fresh (pre-reset) table.  The
// caller swaps tables afterwards and resets the old one
// asynchronously.  Migrated cells are unique by construction so the
// rebuild cannot create duplicate chains.
//
// Output rows are reserved once per CM_CHUNK-slot chunk: a block loads
// the chunk's keys 16 bytes per lane into registers, ranks its takes
// with a wave scan plus a cross-wave LDS step, and thread 0 does the
// one `atomicAdd(out_n, chunk_total)`.  A 2^22-slot table makes 2048
// same-address atomics per close where the per-wave reservation made
// one per wave with a due cell.  Rows past `cap` are counted, not
// written.
//
// Migration stores the value plainly after `find_slot_r` has claimed
// the slot.  That is exact because (1) the target table is fresh
// (keys EMPTY, values zero) and each migrated cell is unique, so
// exactly one thread of this kernel claims a given slot and nobody
// else touches its value; and (2) nothing else writes the target
// while the kernel runs: every writer of either table (the insert and
// aggregation kernels, the overflow drain, the resets of the retired
// table) is enqueued on the same stream as the close, before or after
// it.  The side stream of the two-stream insert runs only the
// scatter, which writes the event buffers and never a table.
#define CM_BLK 256
#define CM_PER 8  // slots per thread per chunk (four 16-byte loads)
#define CM_CHUNK (CM_BLK * CM_PER)
#define CM_MAX_GRID 1024  // four blocks per CU

__global__ __launch_bounds__(CM_BLK) void k_close_migrate(
    const uint64_t* __restrict__ tkeys,
    const unsigned long long* __restrict__ tvals,
    int64_t nslots,
    int64_t win_hi,
    uint64_t* __restrict__ nkeys,
    unsigned long long* __restrict__ nvals,
    uint64_t mask,
    int region_bits,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t cap,
    int* __restrict__ error_flag) {
  constexpr int NW = CM_BLK / WAVE;
  // Double-buffered by chunk parity: two barriers per chunk suffice.
  __shared__ int s_wave[2][NW];
  __shared__ int s_base[2];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const bool vec = ((((uintptr_t)tkeys) | ((uintptr_t)tvals)) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  int par = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x, par ^= 1) {
    const int64_t c0 = c * CM_CHUNK;
    uint64_t k[CM_PER];
    unsigned long long v[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = c0 + (int64_t)j * (CM_BLK * 2) + threadIdx.x * 2;
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
        v[2 * j] = 0;
        v[2 * j + 1] = 0;
        if (kk.x != EMPTY_SLOT || kk.y != EMPTY_SLOT) {
          ulonglong2 vv = *(const ulonglong2*)(tvals + s);
          v[2 * j] = vv.x;
          v[2 * j + 1] = vv.y;
        }
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
          v[2 * j + q] = k[2 * j + q] != EMPTY_SLOT ? tvals[s + q] : 0;
        }
      }
    }
    unsigned takem = 0;
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int32_t win = (int32_t)(uint32_t)(k[q] >> 32);
      if ((int64_t)win < win_hi) {
        takem |= 1u << q;
      } else {
        uint64_t slot = find_slot_r(nkeys, mask, region_bits, k[q]);
        if (slot == ~0ULL) atomicOr(error_flag, 1);
        else nvals[slot] = v[q];
      }
    }
    const int cnt = __popc(takem);
    int incl = cnt;
    for (int off = 1; off < WAVE; off <<= 1) {
      int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == WAVE - 1) s_wave[par][wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < NW; ++w) total += s_wave[par][w];
      s_base[par] = total > 0 ? atomicAdd(out_n, total) : 0;
    }
    __syncthreads();
    if (takem != 0) {
      int64_t idx = (int64_t)s_base[par] + (incl - cnt);
      for (int w = 0; w < wave; ++w) idx += s_wave[par][w];
      for (int q = 0; q < CM_PER; ++q) {
        if (!((takem >> q) & 1u)) continue;
        if (idx < cap) {
          out_keys[idx] = (int32_t)(uint32_t)(k[q] & 0xFFFFFFFFULL);
          out_wins[idx] = (int32_t)(uint32_t)(k[q] >> 32);
          out_vals[idx] = (int64_t)v[q];
        }
        ++idx;
      }
    }
  }
}

// Find (or claim) the slot for `packed` in an open-address table
// (whole-table or region layout, see hash_add).  Returns the slot
// index or ~0 on full table/region.
__device__ __forceinline__ uint64_t find_slot_r(
    uint64_t* __restrict__ tkeys, uint64_t mask, int region_bits,
    uint64_t packed) {
  uint64_t h64 = mix64(packed);
  uint64_t h, probe_mask, base;
  if (region_bits == 0) {
    base = 0;
    probe_mask = mask;
    h = h64 & mask;
  } else {
    base = region_of(h64, mask, region_bits) << region_bits;
    probe_mask = (1ULL << region_bits) - 1;
    h = (h64 >> 32) & probe_mask;
  }
  for (uint64_t probes = 0; probes <= probe_mask; ++probes) {
    uint64_t slot = base | h;
    uint64_t cur = tkeys[slot];
    if (cur == packed) return slot;
    if (cur == EMPTY_SLOT) {
      uint64_t prev = atomicCAS(
          (unsigned long long*)&tkeys[slot], EMPTY_SLOT, packed);
      if (prev == EMPTY_SLOT || prev == packed) return slot;
    }
    h = (h + 1) & probe_mask;
  }
  return ~0ULL;
}

__device__ __forceinline__ uint64_t find_slot(
    uint64_t* __restrict__ tkeys, uint64_t mask, uint64_t packed) {
  return find_slot_r(tkeys, mask, 0, packed);
}

// 1BRC-style keyed running stats: count / sum / min / max per
// (key, window).  One pass over the batch, four atomics per event.
template <bool LATE = false>
__global__ void k_stats_insert(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ ts,
    const int64_t* __restrict__ vals,
    int64_t n,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tcnt,
    long long* __restrict__ tsum,
    long long* __restrict__ tmin,
    long long* __restrict__ tmax,
    uint64_t mask,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    int64_t late_cutoff,  // LATE only (see late_append)
    int32_t* __restrict__ late_keys,
    int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals,
    int* __restrict__ late_n,
    int64_t late_cap) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  for (; i < n; i += stride) {
    int64_t t = ts[i] + ts_base;
    if constexpr (LATE) {
      bool is_late = t < late_cutoff;
      late_append<true>(
          is_late, is_late ? keys[i] : 0, t, is_late ? vals[i] : 0,
          late_keys, late_ts, late_vals, late_n, late_cap, error_flag);
      if (is_late) continue;
    }
    if (t > local_max) local_max = t;
    int64_t win = (t - align_ms) / len_ms;
    uint64_t packed =
        ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
    uint64_t slot = find_slot(tkeys, mask, packed);
    if (slot == ~0ULL) {
      atomicOr(error_flag, 1);
      continue;
    }
    long long v = vals[i];
    atomicAdd((unsigned long long*)&tcnt[slot], 1ULL);
    atomicAdd((unsigned long long*)&tsum[slot], (unsigned long long)v);
    atomicMin(&tmin[slot], v);
    atomicMax(&tmax[slot], v);
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// Recovery fixup: add deltas to count/sum of existing slots.
__global__ void k_stats_fixup(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ ts,
    const int64_t* __restrict__ cnt_delta,
    const int64_t* __restrict__ sum_delta,
    int64_t n,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tcnt,
    long long* __restrict__ tsum,
    uint64_t mask,
    int64_t align_ms,
    int64_t len_ms) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int64_t win = (ts[i] - align_ms) / len_ms;
    uint64_t packed =
        ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
    uint64_t slot = find_slot(tkeys, mask, packed);
    if (slot == ~0ULL) continue;
    atomicAdd((unsigned long long*)&tcnt[slot],
              (unsigned long long)cnt_delta[i]);
    atomicAdd((unsigned long long*)&tsum[slot],
              (unsigned long long)sum_delta[i]);
  }
}

__global__ void k_stats_extract(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tcnt,
    const long long* __restrict__ tsum,
    const long long* __restrict__ tmin,
    const long long* __restrict__ tmax,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_cnt,
    int64_t* __restrict__ out_sum,
    int64_t* __restrict__ out_min,
    int64_t* __restrict__ out_max,
    int* __restrict__ out_n,
    int64_t cap) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < nslots; i += stride) {
    uint64_t k = tkeys[i];
    bool take = false;
    int32_t win = 0;
    if (k != EMPTY_SLOT) {
      win = (int32_t)(uint32_t)(k >> 32);
      take = (int64_t)win >= win_lo && (int64_t)win < win_hi;
    }
    unsigned long long ball = __ballot(take);
    int lane = threadIdx.x & (WAVE - 1);
    if (ball != 0) {
      int wave_total = __popcll(ball);
      int rank = __popcll(ball & ((1ULL << lane) - 1ULL));
      int base = 0;
      int lead = __ffsll((unsigned long long)ball) - 1;
      if (lane == lead) base = atomicAdd(out_n, wave_total);
      base = __shfl(base, lead);
      if (take) {
        int64_t idx = base + rank;
        if (idx < cap) {
          out_keys[idx] = (int32_t)(uint32_t)(k & 0xFFFFFFFFULL);
          out_wins[idx] = win;
          out_cnt[idx] = tcnt[i];
          out_sum[idx] = tsum[i];
          out_min[idx] = tmin[i];
          out_max[idx] = tmax[i];
        }
      }
    }
  }
}

// Stats window close with reclamation: the count/sum/min/max twin of
// k_close_migrate.  One pass over the table in CM_CHUNK-slot chunks
// sorts every cell by its window id `w`:
//   win_lo <= w < win_hi  emit the six columns;
//   w >= win_hi           migrate into the fresh table;
//   w < win_lo            drop.  Such a cell was made by an event
//                         behind the watermark on a path that does not
//                         track lateness, after its window had been
//                         emitted; no extract ever reads it, so
//                         dropping it changes no output.
// The caller swaps the five arrays afterwards and resets the retired
// ones (keys EMPTY, cnt/sum 0, min I64_MAX, max I64_MIN).
//
// Keys are loaded 16 bytes per lane and stay in registers; the four
// value arrays (32 bytes per slot) are read only for a slot that is
// emitted or migrated, at the point where it is, so a thread never
// holds CM_PER x 4 values.  Output rows are reserved as in
// k_close_migrate: wave scan, cross-wave LDS step, one
// `atomicAdd(out_n, chunk_total)` by thread 0; rows past `cap` are
// counted, not written.
//
// Migration stores the four values plainly after `find_slot` has
// claimed the slot (every stats writer uses the whole-table layout).
// The exactness argument of k_close_migrate holds unchanged: (1) the
// target is fresh and each migrated cell is unique, so exactly one
// thread of this kernel claims a given slot and nobody else touches
// its values; (2) nothing else writes the target while the kernel
// runs: every writer of either table (the stats insert, radix insert
// and fixup kernels, the resets of the retired arrays) is enqueued on
// the same stream as the close.  The stats insert has no side stream
// at all.
__global__ __launch_bounds__(CM_BLK) void k_stats_close_migrate(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tcnt,
    const long long* __restrict__ tsum,
    const long long* __restrict__ tmin,
    const long long* __restrict__ tmax,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    uint64_t* __restrict__ nkeys,
    long long* __restrict__ ncnt,
    long long* __restrict__ nsum,
    long long* __restrict__ nmin,
    long long* __restrict__ nmax,
    uint64_t mask,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_cnt,
    int64_t* __restrict__ out_sum,
    int64_t* __restrict__ out_min,
    int64_t* __restrict__ out_max,
    int* __restrict__ out_n,
    int64_t cap,
    int* __restrict__ error_flag) {
  constexpr int NW = CM_BLK / WAVE;
  // Double-buffered by chunk parity: two barriers per chunk suffice.
  __shared__ int s_wave[2][NW];
  __shared__ int s_base[2];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const bool vec = (((uintptr_t)tkeys) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  int par = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x, par ^= 1) {
    // Slot of k[q]: s0 + (q / 2) * (CM_BLK * 2) + (q & 1).
    const int64_t s0 = c * CM_CHUNK + threadIdx.x * 2;
    uint64_t k[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = s0 + (int64_t)j * (CM_BLK * 2);
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
        }
      }
    }
    unsigned takem = 0;
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int64_t win = (int64_t)(int32_t)(uint32_t)(k[q] >> 32);
      if (win < win_lo) continue;
      if (win < win_hi) {
        takem |= 1u << q;
      } else {
        int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
        long long vc = tcnt[s], vs = tsum[s], vmn = tmin[s], vmx = tmax[s];
        uint64_t slot = find_slot(nkeys, mask, k[q]);
        if (slot == ~0ULL) {
          atomicOr(error_flag, 1);
        } else {
          ncnt[slot] = vc;
          nsum[slot] = vs;
          nmin[slot] = vmn;
          nmax[slot] = vmx;
        }
      }
    }
    const int cnt = __popc(takem);
    int incl = cnt;
    for (int off = 1; off < WAVE; off <<= 1) {
      int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == WAVE - 1) s_wave[par][wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < NW; ++w) total += s_wave[par][w];
      s_base[par] = total > 0 ? atomicAdd(out_n, total) : 0;
    }
    __syncthreads();
    if (takem != 0) {
      int64_t idx = (int64_t)s_base[par] + (incl - cnt);
      for (int w = 0; w < wave; ++w) idx += s_wave[par][w];
      for (int q = 0; q < CM_PER; ++q) {
        if (!((takem >> q) & 1u)) continue;
        if (idx < cap) {
          int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
          out_keys[idx] = (int32_t)(uint32_t)(k[q] & 0xFFFFFFFFULL);
          out_wins[idx] = (int32_t)(uint32_t)(k[q] >> 32);
          out_cnt[idx] = tcnt[s];
          out_sum[idx] = tsum[s];
          out_min[idx] = tmin[s];
          out_max[idx] = tmax[s];
        }
        ++idx;
      }
    }
  }
}

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
  int64_t q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// Sliding stats close: fold panes into windows and reclaim dead panes
// in one pass over the pane table.  The table holds one cell per
// (key, pane), a pane being gcd(length, offset) wide; window `w` is
// the `L` panes [w * o, w * o + L), so pane `p` lies in the windows
// floor((p - L) / o) + 1 .. floor(p / o).  Every occupied cell
//   - is folded into each of its windows in [win_lo, win_hi): the
//     cell (key, w) is claimed in the separate fold table and the
//     pane's count/sum/min/max are merged into it with atomicAdd,
//     atomicAdd, atomicMin, atomicMax (count and sum add, min and max
//     observe, so the merge of the panes equals the aggregate of the
//     window's events in any order);
//   - is copied into the fresh table when p >= pane_keep (some window
//     that contains it is still open), exactly as
//     k_stats_close_migrate migrates, and dropped otherwise.
// A pane next to the horizon is both folded and migrated.  The kernel
// emits no rows: the caller runs k_stats_extract over the fold table,
// subtracts L from the window column and refills the fold table's
// five arrays.
//
// The chunked shape is k_stats_close_migrate's: 16-byte key loads,
// CM_CHUNK slots per block step, values read only for a cell that is
// folded or migrated.  No row reservation, so no LDS and no barrier.
//
// Window ids below zero are normal here (the first L - 1 panes after
// `align` lie in windows that open before it), and (w = -1, key = -1)
// would pack to EMPTY_SLOT, so the fold table stores w + L in the
// high half.  With t >= align every pane id is >= 0, every window id
// >= 1 - L and the stored value >= 1; a window below 1 - L (an event
// before `align`, which the stats kernels do not support) is skipped.
//
// Exactness.  Migration: as k_stats_close_migrate, (1) the target is
// fresh and each migrated cell unique, (2) every other writer of
// either table runs on the same stream.  Fold table: (1) it is all
// EMPTY / 0 / 0 / I64_MAX / I64_MIN when the kernel starts, because
// the fills that follow the previous extract are on the same stream;
// (2) `find_slot` hands every thread that folds into (key, w) the
// same slot, and the four merges into it are atomics that commute, so
// the up to L threads that meet there need no order; the fills are
// the identities of the four merges, so a slot needs no first-writer
// initialisation; (3) nothing reads the fold table before the kernel
// has finished: the extract is the next launch on the stream, and
// nothing else ever writes it.
__global__ __launch_bounds__(CM_BLK) void k_stats_pane_close(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tcnt,
    const long long* __restrict__ tsum,
    const long long* __restrict__ tmin,
    const long long* __restrict__ tmax,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    int64_t pane_keep,
    int64_t L,
    int64_t o,
    uint64_t* __restrict__ nkeys,
    long long* __restrict__ ncnt,
    long long* __restrict__ nsum,
    long long* __restrict__ nmin,
    long long* __restrict__ nmax,
    uint64_t mask,
    uint64_t* __restrict__ fkeys,
    long long* __restrict__ fcnt,
    long long* __restrict__ fsum,
    long long* __restrict__ fmin,
    long long* __restrict__ fmax,
    uint64_t fmask,
    int* __restrict__ error_flag) {
  const bool vec = (((uintptr_t)tkeys) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // Slot of k[q]: s0 + (q / 2) * (CM_BLK * 2) + (q & 1).
    const int64_t s0 = c * CM_CHUNK + threadIdx.x * 2;
    uint64_t k[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = s0 + (int64_t)j * (CM_BLK * 2);
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
        }
      }
    }
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int64_t p = (int64_t)(int32_t)(uint32_t)(k[q] >> 32);
      int64_t lo = floor_div(p - L, o) + 1;
      int64_t hi = floor_div(p, o);
      if (lo < win_lo) lo = win_lo;
      if (lo < 1 - L) lo = 1 - L;
      if (hi > win_hi - 1) hi = win_hi - 1;
      const bool keep = p >= pane_keep;
      if (lo > hi && !keep) continue;
      int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
      long long vc = tcnt[s], vs = tsum[s], vmn = tmin[s], vmx = tmax[s];
      const uint64_t key = k[q] & 0xFFFFFFFFULL;
      for (int64_t w = lo; w <= hi; ++w) {
        uint64_t packed = ((uint64_t)(uint32_t)(int32_t)(w + L) << 32) | key;
        uint64_t slot = find_slot(fkeys, fmask, packed);
        if (slot == ~0ULL) {
          atomicOr(error_flag, 1);
          break;
        }
        atomicAdd((unsigned long long*)&fcnt[slot], (unsigned long long)vc);
        atomicAdd((unsigned long long*)&fsum[slot], (unsigned long long)vs);
        atomicMin(&fmin[slot], vmn);
        atomicMax(&fmax[slot], vmx);
      }
      if (keep) {
        uint64_t slot = find_slot(nkeys, mask, k[q]);
        if (slot == ~0ULL) {
          atomicOr(error_flag, 1);
        } else {
          ncnt[slot] = vc;
          nsum[slot] = vs;
          nmin[slot] = vmn;
          nmax[slot] = vmx;
        }
      }
    }
  }
}

// Per-key global join-cell update, "last" insert / "complete" emit
// semantics (reference operators/__init__.py _JoinLogic): store this
// side's value; the update that makes all sides present emits the
// joined row and resets the presence flags, so the next emission
// again requires a fresh value from every side.  Shared by the
// direct insert, the region kernels, and the overflow spill.
__device__ __forceinline__ void join_apply(
    uint64_t packed,
    long long v,
    int side,
    int full,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tval0,
    long long* __restrict__ tval1,
    int* __restrict__ tflags,
    uint64_t mask,
    int region_bits,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag,
    int rearm = 0) {  // the key had >= 2 events this batch: per-item
                      // semantics leave the side flag RE-SET after an
                      // emission (a duplicate lands after the
                      // completing event clears the flags), so a
                      // deduped caller must restore it
  uint64_t slot = find_slot_r(tkeys, mask, region_bits, packed);
  if (slot == ~0ULL) {
    atomicOr(error_flag, 1);
    return;
  }
  if (side == 0) {
    atomicExch((unsigned long long*)&tval0[slot], (unsigned long long)v);
  } else {
    atomicExch((unsigned long long*)&tval1[slot], (unsigned long long)v);
  }
  int old = atomicOr(&tflags[slot], 1 << side);
  if ((old | (1 << side)) == full && old != full) {
    int idx = atomicAdd(out_n, 1);
    if (idx < out_cap) {
      out_keys[idx] = (int32_t)(uint32_t)(packed & 0xFFFFFFFFULL);
      out_v0[idx] = tval0[slot];
      out_v1[idx] = tval1[slot];
    }
    atomicAnd(&tflags[slot], 0);
    if (rearm) atomicOr(&tflags[slot], 1 << side);
  }
}

// Direct (unpartitioned) join insert: one global-table update per
// event.
__global__ void k_join_insert(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ vals,
    int64_t n,
    int side,
    int n_sides,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tval0,
    long long* __restrict__ tval1,
    int* __restrict__ tflags,
    uint64_t mask,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int* __restrict__ out_n,
    int64_t cap,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int full = (1 << n_sides) - 1;
  for (; i < n; i += stride) {
    join_apply((uint64_t)(uint32_t)keys[i], vals[i], side, full, tkeys,
               tval0, tval1, tflags, mask, 0, out_keys, out_v0, out_v1,
               out_n, cap, error_flag);
  }
}

// Region-partitioned join insert: events arrive pre-bucketed into
// per-region segments (k_radix_scatter_fixed with len=2^40 so the
// window id is 0 and `packed` is the bare key); one workgroup per
// region keeps its table slice L2-warm while processing its segment.
__global__ void k_join_region(
    const uint64_t* __restrict__ ev_packed,
    const int64_t* __restrict__ ev_vals,
    const int* __restrict__ counts,
    int64_t cap,
    int side,
    int n_sides,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tval0,
    long long* __restrict__ tval1,
    int* __restrict__ tflags,
    uint64_t mask,
    int region_bits,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  int b = blockIdx.x;
  int cnt = counts[b];
  if (cnt > (int)cap) cnt = (int)cap;
  int64_t start = (int64_t)b * cap;
  int full = (1 << n_sides) - 1;
  for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
    uint64_t packed = ev_packed[start + j];
    if (packed == EMPTY_SLOT) continue;  // staged-scatter pad
    join_apply(packed, ev_vals[start + j], side, full, tkeys, tval0,
               tval1, tflags, mask, region_bits, out_keys, out_v0,
               out_v1, out_n, out_cap, error_flag);
  }
}

// LDS-deduped region join: one workgroup per region; the region's
// batch segment is first collapsed in LDS to (key -> last value)
// for this side, then merged — ONE global-table update per distinct
// key instead of per event (same staging shape as k_radix_agg).
// Since each launch carries a single side, a per-batch dedup cannot
// change emission counts: at most one not-full -> full transition
// per key per single-side batch either way.
template <int BLK = 256>
__global__ __launch_bounds__(BLK) void k_join_region_lds(
    const uint64_t* __restrict__ ev_packed,
    const int64_t* __restrict__ ev_vals,
    const int* __restrict__ counts,
    int64_t cap,
    int side,
    int n_sides,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tval0,
    long long* __restrict__ tval1,
    int* __restrict__ tflags,
    uint64_t mask,
    int region_bits,
    int lds_bits,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  extern __shared__ char smem[];
  int R = 1 << lds_bits;
  uint64_t* lkeys = (uint64_t*)smem;
  unsigned long long* lvals =
      (unsigned long long*)(smem + (size_t)R * sizeof(uint64_t));
  int* lcnt = (int*)(smem + (size_t)R * 2 * sizeof(uint64_t));
  for (int s = threadIdx.x; s < R; s += blockDim.x) {
    lkeys[s] = EMPTY_SLOT;
    lcnt[s] = 0;
  }
  __syncthreads();
  int b = blockIdx.x;
  int cnt = counts[b];
  if (cnt > (int)cap) cnt = (int)cap;
  int64_t start = (int64_t)b * cap;
  int full = (1 << n_sides) - 1;
  for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
    uint64_t packed = ev_packed[start + j];
    if (packed == EMPTY_SLOT) continue;  // staged-scatter pad
    unsigned long long v = (unsigned long long)ev_vals[start + j];
    uint64_t h64 = mix64(packed);
    int lh = (int)((h64 >> 32) & (R - 1));
    bool done = false;
    for (int p = 0; p < R; ++p) {
      uint64_t cur = lkeys[lh];
      if (cur == packed) {
        atomicExch(&lvals[lh], v);
        atomicAdd(&lcnt[lh], 1);
        done = true;
        break;
      }
      if (cur == EMPTY_SLOT) {
        uint64_t prev = atomicCAS(
            (unsigned long long*)&lkeys[lh], EMPTY_SLOT, packed);
        if (prev == EMPTY_SLOT || prev == packed) {
          atomicExch(&lvals[lh], v);
          atomicAdd(&lcnt[lh], 1);
          done = true;
          break;
        }
      }
      lh = (lh + 1) & (R - 1);
    }
    if (!done) {
      // LDS staging full: apply straight to the global region.
      join_apply(packed, (long long)v, side, full, tkeys, tval0, tval1,
                 tflags, mask, region_bits, out_keys, out_v0, out_v1,
                 out_n, out_cap, error_flag);
    }
  }
  __syncthreads();
  // Merge distinct keys once into the global table (the segment's
  // region is contiguous in HBM, so the probes stay local); keys
  // with >= 2 events keep per-item re-arm semantics via join_apply.
  for (int s = threadIdx.x; s < R; s += blockDim.x) {
    if (lkeys[s] != EMPTY_SLOT) {
      join_apply(lkeys[s], (long long)lvals[s], side, full, tkeys,
                 tval0, tval1, tflags, mask, region_bits, out_keys,
                 out_v0, out_v1, out_n, out_cap, error_flag,
                 lcnt[s] >= 2);
    }
  }
}

// Overflow spill for the region join (direct path).
__global__ void k_join_overflow(
    const uint64_t* __restrict__ ov_packed,
    const int64_t* __restrict__ ov_vals,
    const int* __restrict__ ov_cursor,
    int64_t ov_cap,
    int side,
    int n_sides,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tval0,
    long long* __restrict__ tval1,
    int* __restrict__ tflags,
    uint64_t mask,
    int region_bits,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  int64_t n = *ov_cursor;
  if (n > ov_cap) n = ov_cap;
  int full = (1 << n_sides) - 1;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    join_apply(ov_packed[i], ov_vals[i], side, full, tkeys, tval0,
               tval1, tflags, mask, region_bits, out_keys, out_v0,
               out_v1, out_n, out_cap, error_flag);
  }
}

// Extract live join-side state (for recovery snapshots).
__global__ void k_join_extract(
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tval0,
    long long* __restrict__ tval1,
    int* __restrict__ tflags,
    int64_t nslots,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int32_t* __restrict__ out_flags,
    int* __restrict__ out_n,
    int64_t cap) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < nslots; i += stride) {
    uint64_t k = tkeys[i];
    bool take = (k != EMPTY_SLOT) && (tflags[i] != 0);
    unsigned long long ball = __ballot(take);
    int lane = threadIdx.x & (WAVE - 1);
    if (ball != 0) {
      int wave_total = __popcll(ball);
      int rank = __popcll(ball & ((1ULL << lane) - 1ULL));
      int base = 0;
      int lead = __ffsll((unsigned long long)ball) - 1;
      if (lane == lead) base = atomicAdd(out_n, wave_total);
      base = __shfl(base, lead);
      if (take) {
        int64_t idx = base + rank;
        if (idx < cap) {
          out_keys[idx] = (int32_t)(uint32_t)(k & 0xFFFFFFFFULL);
          out_v0[idx] = tval0[i];
          out_v1[idx] = tval1[i];
          out_flags[idx] = tflags[i];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Windowed two-sided join ("first"/"last" insert, "final" emit).  The
// table is the whole-table layout of the stats writers: `tkeys` holds
// `window << 32 | key` (EMPTY_SLOT = empty), and per side there are a
// timestamp array `tts` (the stamp: the timestamp of the event that
// holds the side) and a value array `tval`.  A side is present iff its
// stamp differs from WJ_TS_NONE<FIRST> (I64_MIN under "last", I64_MAX
// under "first"); event timestamps lie strictly between the two, so a
// value is never a sentinel.  `telect` is one int32 election word per
// slot, shared by both sides because one insert call handles one side.
//
// Winner rule of one (key, window, side): "last" keeps the event with
// the greatest (ts, arrival), "first" the one with the smallest, where
// arrival orders batches by call and rows by index.
//
// Insert is three launches on one stream over one side's batch:
//   stamp   find_slot, then atomicMax ("last") / atomicMin ("first")
//           of ts on the side's stamp.  The slot goes to `ev_slot[i]`
//           (-1: table full) so that the later passes do not probe.
//           Under "first" an event that strictly lowers the stamp
//           opens the cell's election word (WJ_IDLE -> WJ_OPEN).
//           The LATE form first diverts events below the late cutoff
//           to the late buffer (see late_append) with ev_slot -1.
//   elect   every event whose ts equals the now final stamp bids its
//           row index: atomicMax ("last") / atomicMin ("first") on the
//           election word.  Under "first" only opened cells take bids.
//   commit  the event whose row index equals the elected one stores
//           its value and puts the election word back to idle.
//
// Exactness.  (1) Who may write a value: only the commit pass, and
// there only the event whose row equals the cell's election word.  Row
// indices are unique within a batch, so at most one event per cell and
// batch stores; the word is idle between inserts, and idle (-1 under
// "last", WJ_IDLE under "first") equals no row index, the launcher
// bounds n below WJ_OPEN.  (2) That event is the winner.  After the
// stamp pass a stamp is max ("last") / min ("first") of its old value
// and the batch's timestamps for the cell, atomics being total per
// address.  "last": a batch event wins iff its ts is >= every earlier
// one's, i.e. equals the new stamp (an equal earlier batch loses to
// the later arrival), and among those the greatest row wins: exactly
// the bidders and the atomicMax of the elect pass.  If none equals the
// stamp the earlier holder stays and nobody bids.  "first": a batch
// event wins iff its ts is strictly below the old stamp (an equal
// earlier batch keeps the side) and equals the new stamp, smallest row
// first.  The stamp went strictly down iff some event's atomicMin
// returned a value above its ts, and that event opened the word; so
// "opened and ts == stamp" is exactly the winning set, and an event
// that merely equals an earlier batch's stamp finds the word idle.
// Every opened cell has a bidder (the event that set the final
// stamp), so every opened word is put back by the commit.  (3) Launch
// order is enough: each pass reads only what the pass before wrote
// (stamps and ev_slot, then election words), and launches on one
// stream run in order with their writes visible to the next.  Every
// other writer of the table (close, resets, restore) is enqueued on
// that stream too.  (4) Late rows (the `LATE` stamp pass).  An event
// with t < late_cutoff stores ev_slot[i] = -1 and nothing else of the
// table: it does not probe, lowers no stamp and opens no election
// word.  ev_slot is a scratch that keeps the slots of earlier batches,
// so that store is what takes the row out: elect and commit skip a
// negative slot, hence a late row is in no pass's bidder set and (1)
// and (2) hold over the accepted rows alone.  The late cursor is only
// ever advanced by wave leaders, one atomicAdd of the wave's late
// count each, and every late lane stores to its own rank above the
// returned base, so rows neither collide nor leave holes.
#define WJ_IDLE 0x7FFFFFFF  // "first": no election open
#define WJ_OPEN 0x7FFFFFFE  // "first": stamp lowered, bids welcome

template <bool FIRST>
__device__ __forceinline__ constexpr long long wj_ts_none() {
  return FIRST ? INT64_MAX : INT64_MIN;
}

template <bool FIRST, typename TS = int64_t, bool LATE = false>
__global__ void k_wjoin_stamp(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,  // LATE only (the late row's value)
    int64_t n,
    uint64_t* __restrict__ tkeys,
    long long* __restrict__ tts,  // this side's stamps
    int* __restrict__ telect,
    uint64_t mask,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int32_t* __restrict__ ev_slot,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag,
    int64_t late_cutoff,  // LATE only (see late_append)
    int32_t* __restrict__ late_keys,
    int64_t* __restrict__ late_ts,
    int64_t* __restrict__ late_vals,
    int* __restrict__ late_n,
    int64_t late_cap) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  for (; i < n; i += stride) {
    int64_t t = (int64_t)ts[i] + ts_base;
    if constexpr (LATE) {
      // Every lane still in the loop votes; lanes past n have left it.
      bool is_late = t < late_cutoff;
      late_append<true>(
          is_late, is_late ? keys[i] : 0, t, is_late ? vals[i] : 0,
          late_keys, late_ts, late_vals, late_n, late_cap, error_flag);
      if (is_late) {
        // The scratch keeps earlier batches' slots: without this store
        // the row would bid and commit into another cell.
        ev_slot[i] = -1;
        continue;
      }
    }
    if (t > local_max) local_max = t;
    int64_t win = floor_div(t - align_ms, len_ms);
    uint64_t packed =
        ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
    uint64_t slot = find_slot(tkeys, mask, packed);
    if (slot == ~0ULL) {
      atomicOr(error_flag, 1);
      ev_slot[i] = -1;
      continue;
    }
    ev_slot[i] = (int32_t)slot;
    if constexpr (FIRST) {
      long long old = atomicMin(&tts[slot], (long long)t);
      if ((long long)t < old) atomicMin(&telect[slot], WJ_OPEN);
    } else {
      atomicMax(&tts[slot], (long long)t);
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

template <bool FIRST, typename TS = int64_t>
__global__ void k_wjoin_elect(
    const TS* __restrict__ ts,
    int64_t n,
    int64_t ts_base,
    const long long* __restrict__ tts,
    int* __restrict__ telect,
    const int32_t* __restrict__ ev_slot) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int32_t slot = ev_slot[i];
    if (slot < 0) continue;
    if ((long long)((int64_t)ts[i] + ts_base) != tts[slot]) continue;
    if constexpr (FIRST) {
      // Bids only lower an opened word, so it never reads idle again
      // within this pass.
      if (telect[slot] != WJ_IDLE) atomicMin(&telect[slot], (int)i);
    } else {
      atomicMax(&telect[slot], (int)i);
    }
  }
}

template <bool FIRST>
__global__ void k_wjoin_commit(
    const int64_t* __restrict__ vals,
    int64_t n,
    long long* __restrict__ tval,  // this side's values
    int* __restrict__ telect,
    const int32_t* __restrict__ ev_slot) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int32_t slot = ev_slot[i];
    if (slot < 0) continue;
    // The elected row is the only one that can compare equal: the
    // other events of the cell see either it or the idle value.
    if (telect[slot] != (int)i) continue;
    tval[slot] = vals[i];
    telect[slot] = FIRST ? WJ_IDLE : -1;
  }
}

// Presence mask of a cell from its two stamps (bit s = side s).
__device__ __forceinline__ int wj_mask(
    long long t0, long long t1, long long ts_none) {
  return (t0 != ts_none ? 1 : 0) | (t1 != ts_none ? 2 : 0);
}

// Windowed-join close with reclamation: the join's twin of
// k_stats_close_migrate.  One pass over the table in CM_CHUNK-slot
// chunks sorts every cell by its window id `w`:
//   win_lo <= w < win_hi  emit keys, wins, v0, v1, mask;
//   w >= win_hi           migrate into the fresh table, both stamps
//                         and both values;
//   w < win_lo            drop.  Such a cell was made by an event
//                         behind the closed horizon; its window has
//                         been emitted and no extract reads it.  Only
//                         inserts without late tracking make one: the
//                         LATE stamp pass accepts t >= wm - wait only,
//                         whose window is at or above the horizon.
// The caller swaps the tables afterwards and resets the retired one
// (keys EMPTY, stamps `ts_none`, values 0, election words idle).
// Election words are idle between inserts, so they are not migrated:
// the fresh table's are idle already.
//
// Keys are loaded 16 bytes per lane and stay in registers; stamps and
// values are read only for a slot that is emitted or migrated, at the
// point where it is.  Output rows are reserved per chunk as in
// k_close_migrate: wave scan, cross-wave LDS step, one
// `atomicAdd(out_n, chunk_total)` by thread 0; rows past `cap` are
// counted, not written.  A missing side's value column reads 0; the
// mask, never the value, says whether a side is there.
//
// Exactness is k_stats_close_migrate's: (1) the target is fresh and
// every migrated cell is unique, so exactly one thread claims a given
// slot and stores its four words plainly; (2) nothing else writes
// either table meanwhile: the insert passes, the resets and this
// kernel are all enqueued on one stream.
__global__ __launch_bounds__(CM_BLK) void k_wjoin_close_migrate(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tts0,
    const long long* __restrict__ tts1,
    const long long* __restrict__ tv0,
    const long long* __restrict__ tv1,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    long long ts_none,
    uint64_t* __restrict__ nkeys,
    long long* __restrict__ nts0,
    long long* __restrict__ nts1,
    long long* __restrict__ nv0,
    long long* __restrict__ nv1,
    uint64_t mask,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int32_t* __restrict__ out_mask,
    int* __restrict__ out_n,
    int64_t cap,
    int* __restrict__ error_flag) {
  constexpr int NW = CM_BLK / WAVE;
  // Double-buffered by chunk parity: two barriers per chunk suffice.
  __shared__ int s_wave[2][NW];
  __shared__ int s_base[2];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const bool vec = (((uintptr_t)tkeys) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  int par = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x, par ^= 1) {
    // Slot of k[q]: s0 + (q / 2) * (CM_BLK * 2) + (q & 1).
    const int64_t s0 = c * CM_CHUNK + threadIdx.x * 2;
    uint64_t k[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = s0 + (int64_t)j * (CM_BLK * 2);
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
        }
      }
    }
    unsigned takem = 0;
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int64_t win = (int64_t)(int32_t)(uint32_t)(k[q] >> 32);
      if (win < win_lo) continue;
      int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
      if (win < win_hi) {
        // A cell with no side (only a timestamp equal to `ts_none`,
        // outside the documented range, leaves one) is not a row.
        if (wj_mask(tts0[s], tts1[s], ts_none) != 0) takem |= 1u << q;
      } else {
        long long a0 = tts0[s], a1 = tts1[s], b0 = tv0[s], b1 = tv1[s];
        uint64_t slot = find_slot(nkeys, mask, k[q]);
        if (slot == ~0ULL) {
          atomicOr(error_flag, 1);
        } else {
          nts0[slot] = a0;
          nts1[slot] = a1;
          nv0[slot] = b0;
          nv1[slot] = b1;
        }
      }
    }
    const int cnt = __popc(takem);
    int incl = cnt;
    for (int off = 1; off < WAVE; off <<= 1) {
      int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == WAVE - 1) s_wave[par][wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < NW; ++w) total += s_wave[par][w];
      s_base[par] = total > 0 ? atomicAdd(out_n, total) : 0;
    }
    __syncthreads();
    if (takem != 0) {
      int64_t idx = (int64_t)s_base[par] + (incl - cnt);
      for (int w = 0; w < wave; ++w) idx += s_wave[par][w];
      for (int q = 0; q < CM_PER; ++q) {
        if (!((takem >> q) & 1u)) continue;
        if (idx < cap) {
          int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
          int m = wj_mask(tts0[s], tts1[s], ts_none);
          out_keys[idx] = (int32_t)(uint32_t)(k[q] & 0xFFFFFFFFULL);
          out_wins[idx] = (int32_t)(uint32_t)(k[q] >> 32);
          out_v0[idx] = (m & 1) ? tv0[s] : 0;
          out_v1[idx] = (m & 2) ? tv1[s] : 0;
          out_mask[idx] = m;
        }
        ++idx;
      }
    }
  }
}

// Non-mutating scan of the windowed-join table (snapshots, EOF): every
// live cell of windows in [win_lo, win_hi) with both values, both
// stamps and the presence mask (a missing side's value and stamp read
// 0).  Rows are reserved per wave.
__global__ void k_wjoin_extract(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tts0,
    const long long* __restrict__ tts1,
    const long long* __restrict__ tv0,
    const long long* __restrict__ tv1,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    long long ts_none,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int64_t* __restrict__ out_t0,
    int64_t* __restrict__ out_t1,
    int32_t* __restrict__ out_mask,
    int* __restrict__ out_n,
    int64_t cap) {
  // Whole waves stay in the loop together: the ballot below needs
  // every lane of a wave that has any slot left.
  int64_t base_i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int lane = threadIdx.x & (WAVE - 1);
  for (int64_t i = base_i; i - lane < nslots; i += stride) {
    uint64_t k = i < nslots ? tkeys[i] : EMPTY_SLOT;
    bool take = false;
    int32_t win = 0;
    int m = 0;
    long long a0 = 0, a1 = 0;
    if (k != EMPTY_SLOT) {
      win = (int32_t)(uint32_t)(k >> 32);
      if ((int64_t)win >= win_lo && (int64_t)win < win_hi) {
        a0 = tts0[i];
        a1 = tts1[i];
        m = wj_mask(a0, a1, ts_none);
        take = m != 0;
      }
    }
    unsigned long long ball = __ballot(take);
    if (ball != 0) {
      int wave_total = __popcll(ball);
      int rank = __popcll(ball & ((1ULL << lane) - 1ULL));
      int base = 0;
      int lead = __ffsll((unsigned long long)ball) - 1;
      if (lane == lead) base = atomicAdd(out_n, wave_total);
      base = __shfl(base, lead);
      if (take) {
        int64_t idx = base + rank;
        if (idx < cap) {
          out_keys[idx] = (int32_t)(uint32_t)(k & 0xFFFFFFFFULL);
          out_wins[idx] = win;
          out_v0[idx] = (m & 1) ? tv0[i] : 0;
          out_v1[idx] = (m & 2) ? tv1[i] : 0;
          out_t0[idx] = (m & 1) ? a0 : 0;
          out_t1[idx] = (m & 2) ? a1 : 0;
          out_mask[idx] = m;
        }
      }
    }
  }
}

// Sliding windowed join close: two passes over the pane table.  The
// table holds one cell per (key, pane), a pane being a tumbling window
// of gcd(length, offset); the geometry is k_stats_pane_close's: window
// `w` is the `L` panes [w * o, w * o + L), pane `p` lies in the windows
// floor((p - L) / o) + 1 .. floor(p / o), clipped to [win_lo, win_hi)
// and to >= 1 - L, and the fold table stores w + L in the high key half
// so that (w = -1, key = -1) does not pack to EMPTY_SLOT.  A window
// below 1 - L (an event before `align`, which the sliding join does not
// support) is skipped.
//
// The fold table is five arrays (keys, ts0, ts1, v0, v1; no election
// words), EMPTY / ts_none / ts_none / 0 / 0 when the stamp pass starts.
// A side of a fold cell is a (stamp, value) pair, which no single
// commuting atomic merges; hence
//   stamp   (k_wjoin_pane_stamp) every occupied pane cell with a side
//           claims (key, w + L) for each of its windows in range and
//           does atomicMax ("last") / atomicMin ("first") of each
//           present side's pane stamp on that side's fold stamp.  A
//           cell with p >= pane_keep is also copied into the fresh
//           pane table (both stamps, both values), exactly as
//           k_wjoin_close_migrate migrates; the others are dropped.
//   commit  (k_wjoin_pane_commit) the same walk over the old pane
//           table, which the stamp pass has not written: per window in
//           range and present side the fold cell is looked up again
//           (find only, no claim), and the pane whose stamp equals the
//           fold stamp stores its value plainly.
// The rows are then read with k_wjoin_extract over the fold table; the
// caller subtracts L from the window column and refills the table.
//
// The chunked shape is k_wjoin_close_migrate's: 16-byte key loads,
// CM_CHUNK slots per block step, stamps and values read only for a
// cell that is folded or migrated.  No row reservation, so no LDS and
// no barrier.
//
// Exactness.  (1) Who may write a fold value: only the commit pass, and
// there only a pane cell whose side stamp equals the fold cell's.
// (2) That writer is unique and is the winner.  The panes of a window
// are disjoint in time and a side's stamp is the timestamp of an event
// of that pane, so the stamps of one (key, side) in different panes are
// pairwise different.  After the stamp pass a fold stamp is the max
// ("last") / min ("first") of the stamps of the window's panes that
// hold the side, atomics being total per address and `ts_none` their
// identity; exactly one pane equals it.  The side of window `w` under
// "last" is the event with the greatest (ts, arrival) over the window:
// it lies in the pane with the greatest stamp, and within that pane the
// insert has already applied the arrival tie rule, equal timestamps
// never spanning two panes.  "first" mirrors it.  (3) Launch order is
// enough: the commit reads only fold keys and stamps, which the stamp
// pass finished writing before the commit starts on the same stream,
// and the old pane table, which neither pass writes; the extract is
// the next launch after the commit, and the refills follow it.  Every
// other writer of the three tables (insert, resets, restore) is
// enqueued on that stream too.  Migration: as k_wjoin_close_migrate,
// the target is fresh and each migrated cell unique.
__device__ __forceinline__ bool wj_pane_windows(
    uint64_t cell, int64_t win_lo, int64_t win_hi, int64_t L, int64_t o,
    int64_t* p, int64_t* lo, int64_t* hi) {
  *p = (int64_t)(int32_t)(uint32_t)(cell >> 32);
  int64_t a = floor_div(*p - L, o) + 1;
  int64_t b = floor_div(*p, o);
  if (a < win_lo) a = win_lo;
  if (a < 1 - L) a = 1 - L;
  if (b > win_hi - 1) b = win_hi - 1;
  *lo = a;
  *hi = b;
  return a <= b;
}

// Find-only probe (no claim): the slot of `packed` or ~0 if absent.
__device__ __forceinline__ uint64_t lookup_slot(
    const uint64_t* __restrict__ tkeys, uint64_t mask, uint64_t packed) {
  uint64_t h = mix64(packed) & mask;
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    uint64_t cur = tkeys[h];
    if (cur == packed) return h;
    if (cur == EMPTY_SLOT) return ~0ULL;
    h = (h + 1) & mask;
  }
  return ~0ULL;
}

template <bool FIRST>
__global__ __launch_bounds__(CM_BLK) void k_wjoin_pane_stamp(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tts0,
    const long long* __restrict__ tts1,
    const long long* __restrict__ tv0,
    const long long* __restrict__ tv1,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    int64_t pane_keep,
    int64_t L,
    int64_t o,
    uint64_t* __restrict__ nkeys,
    long long* __restrict__ nts0,
    long long* __restrict__ nts1,
    long long* __restrict__ nv0,
    long long* __restrict__ nv1,
    uint64_t mask,
    uint64_t* __restrict__ fkeys,
    long long* __restrict__ fts0,
    long long* __restrict__ fts1,
    uint64_t fmask,
    int* __restrict__ error_flag) {
  constexpr long long ts_none = wj_ts_none<FIRST>();
  const bool vec = (((uintptr_t)tkeys) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // Slot of k[q]: s0 + (q / 2) * (CM_BLK * 2) + (q & 1).
    const int64_t s0 = c * CM_CHUNK + threadIdx.x * 2;
    uint64_t k[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = s0 + (int64_t)j * (CM_BLK * 2);
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
        }
      }
    }
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int64_t p, lo, hi;
      const bool fold =
          wj_pane_windows(k[q], win_lo, win_hi, L, o, &p, &lo, &hi);
      const bool keep = p >= pane_keep;
      if (!fold && !keep) continue;
      int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
      const long long a0 = tts0[s], a1 = tts1[s];
      // A cell with no side (see k_wjoin_close_migrate) makes no row.
      if (fold && wj_mask(a0, a1, ts_none) != 0) {
        const uint64_t key = k[q] & 0xFFFFFFFFULL;
        for (int64_t w = lo; w <= hi; ++w) {
          uint64_t packed = ((uint64_t)(uint32_t)(int32_t)(w + L) << 32) | key;
          uint64_t slot = find_slot(fkeys, fmask, packed);
          if (slot == ~0ULL) {
            atomicOr(error_flag, 1);
            break;
          }
          if constexpr (FIRST) {
            if (a0 != ts_none) atomicMin(&fts0[slot], a0);
            if (a1 != ts_none) atomicMin(&fts1[slot], a1);
          } else {
            if (a0 != ts_none) atomicMax(&fts0[slot], a0);
            if (a1 != ts_none) atomicMax(&fts1[slot], a1);
          }
        }
      }
      if (keep) {
        long long b0 = tv0[s], b1 = tv1[s];
        uint64_t slot = find_slot(nkeys, mask, k[q]);
        if (slot == ~0ULL) {
          atomicOr(error_flag, 1);
        } else {
          nts0[slot] = a0;
          nts1[slot] = a1;
          nv0[slot] = b0;
          nv1[slot] = b1;
        }
      }
    }
  }
}

// The commit pass of the sliding join close (see k_wjoin_pane_stamp,
// whose walk and window ranges this repeats).  Only finds, no claims:
// the stamp pass claimed every fold cell looked up here, so a missing
// one means that pass ran out of fold slots (it has raised the flag
// already) and is reported the same way.
__global__ __launch_bounds__(CM_BLK) void k_wjoin_pane_commit(
    const uint64_t* __restrict__ tkeys,
    const long long* __restrict__ tts0,
    const long long* __restrict__ tts1,
    const long long* __restrict__ tv0,
    const long long* __restrict__ tv1,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    int64_t L,
    int64_t o,
    long long ts_none,
    const uint64_t* __restrict__ fkeys,
    const long long* __restrict__ fts0,
    const long long* __restrict__ fts1,
    long long* __restrict__ fv0,
    long long* __restrict__ fv1,
    uint64_t fmask,
    int* __restrict__ error_flag) {
  const bool vec = (((uintptr_t)tkeys) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // Slot of k[q]: s0 + (q / 2) * (CM_BLK * 2) + (q & 1).
    const int64_t s0 = c * CM_CHUNK + threadIdx.x * 2;
    uint64_t k[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = s0 + (int64_t)j * (CM_BLK * 2);
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
        }
      }
    }
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int64_t p, lo, hi;
      if (!wj_pane_windows(k[q], win_lo, win_hi, L, o, &p, &lo, &hi)) continue;
      int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
      const long long a0 = tts0[s], a1 = tts1[s];
      if (wj_mask(a0, a1, ts_none) == 0) continue;
      const long long b0 = tv0[s], b1 = tv1[s];
      const uint64_t key = k[q] & 0xFFFFFFFFULL;
      for (int64_t w = lo; w <= hi; ++w) {
        uint64_t packed = ((uint64_t)(uint32_t)(int32_t)(w + L) << 32) | key;
        uint64_t slot = lookup_slot(fkeys, fmask, packed);
        if (slot == ~0ULL) {
          atomicOr(error_flag, 1);
          break;
        }
        // `ts_none` is no event's timestamp, so an absent side never
        // compares equal to a fold stamp some other pane has set.
        if (a0 != ts_none && fts0[slot] == a0) fv0[slot] = b0;
        if (a1 != ts_none && fts1[slot] == a1) fv1[slot] = b1;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Windowed product join: every left value of a (key, window) cell
// paired with every right value of it ("product" insert, "final" emit).
// A cell is two variable-length value lists, so the state is not a row
// per cell but
//   table   `tkeys` holds `window << 32 | key` (EMPTY_SLOT = empty) and
//           `tcnt[2 * slot + s]` the number of values of side `s`;
//   logs    one append log per side of 16-byte entries (packed cell
//           word, int64 value), `log_n` its int32 cursor.
// The table says how many values a cell has, the logs hold them in
// arrival order of the reservations, which is no order at all: the
// product of two lists is the same multiset whatever their order.
//
// Insert (k_wjprod_insert, one launch per side batch) is wjprod_put
// per event: find_slot, atomicAdd on the side's count, one 16-byte
// append at a wave-reserved log position.  An event that finds the
// table full sets the error flag and does neither, so for every
// (cell, side) the count equals the number of log entries at all times
// between launches (*).
//
// A close at [win_lo, win_hi) is three launches around one readback:
//   plan    (k_wjprod_plan) lists every due cell as (packed, n0, n1)
//           and writes its list index into `slot_cell[slot]`.  Nothing
//           else is written, so the host may still refuse the close
//           (too many rows) with the state untouched.  The host takes
//           inclusive int64 prefix sums of n0 + n1 (`val_end`) and of
//           max(n0, 1) * max(n1, 1) (`row_end`) over the list.
//   gather  (k_wjprod_gather, once per side over its log) sorts every
//           entry by its window `w`: w < win_lo is dropped (an event
//           behind the closed horizon); w < win_hi stores its value
//           into the arena; otherwise it is put into the fresh table
//           and the fresh log by wjprod_put.  The caller swaps tables
//           and logs and resets the retired ones.
//   expand  (k_wjprod_expand) one thread per output row.
//
// Exactness.  (1) Every log entry takes exactly one of the three arms
// of the gather, by its window alone.  (2) Arena: cell `c` owns the
// words [val_end[c] - n0 - n1, val_end[c]), disjoint between cells by
// the prefix sum; side 0 the first n0 of them, side 1 the rest.  A due
// entry of (cell, side) takes `atomicSub(count, 1) - 1` as its place.
// By (*) exactly n_s entries of that (cell, side) exist, the count
// starts at n_s (the plan only read it), and atomics on one address
// are totally ordered, so the places handed out are a permutation of
// 0 .. n_s - 1: every arena word is written exactly once.  (3) A
// migrated entry bumps the fresh count and appends to the fresh log
// together, so (*) holds for the fresh state.  The fresh log has the
// retired one's capacity and receives a subset of its entries.  (4) The
// insert, the three close launches, the prefix sums, the resets and
// the log growth copies are all enqueued on one stream.
#define ERR_WJPROD_BOUND 4  // a guard fired: host-side bound is wrong

// One event into a product-join table and log.  Called by every lane
// still in its loop, `take` or not, so that the wave votes together.
__device__ __forceinline__ void wjprod_put(
    bool take, uint64_t packed, int64_t val,
    uint64_t* __restrict__ tkeys, int* __restrict__ tcnt, uint64_t mask,
    int side, ulonglong2* __restrict__ log, int* __restrict__ log_n,
    int64_t log_cap, int* __restrict__ error_flag) {
  uint64_t slot = take ? find_slot(tkeys, mask, packed) : ~0ULL;
  const bool ok = slot != ~0ULL;
  if (take && !ok) atomicOr(error_flag, 1);
  if (ok) atomicAdd(&tcnt[2 * slot + side], 1);
  int pos = wave_reserve(ok, log_n);
  if (ok) {
    if (pos >= 0 && pos < log_cap) {
      log[pos] = make_ulonglong2(packed, (unsigned long long)val);
    } else {
      atomicOr(error_flag, ERR_WJPROD_BOUND);
    }
  }
}

template <typename TS = int64_t>
__global__ void k_wjprod_insert(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,
    int64_t n,
    uint64_t* __restrict__ tkeys,
    int* __restrict__ tcnt,
    uint64_t mask,
    int side,
    ulonglong2* __restrict__ log,
    int* __restrict__ log_n,
    int64_t log_cap,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  for (; i < n; i += stride) {
    int64_t t = (int64_t)ts[i] + ts_base;
    if (t > local_max) local_max = t;
    int64_t win = floor_div(t - align_ms, len_ms);
    uint64_t packed =
        ((uint64_t)(uint32_t)(int32_t)win << 32) | (uint32_t)keys[i];
    wjprod_put(true, packed, vals[i], tkeys, tcnt, mask, side, log, log_n,
               log_cap, error_flag);
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

// The plan pass of the product-join close (see above): the due cells
// of [win_lo, win_hi) as a compact list, in the chunked shape of
// k_wjoin_close_migrate.  List places are reserved once per chunk; a
// slot is listed at most once, so `cells_n` never passes `nslots`, the
// length of the list arrays.  Reads the table, writes the list, its
// cursor and `slot_cell` at the listed slots only.
__global__ __launch_bounds__(CM_BLK) void k_wjprod_plan(
    const uint64_t* __restrict__ tkeys,
    const int* __restrict__ tcnt,
    int64_t nslots,
    int64_t win_lo,
    int64_t win_hi,
    uint64_t* __restrict__ cell_pk,
    int* __restrict__ cell_n,  // (n0, n1) per listed cell
    int* __restrict__ slot_cell,
    int* __restrict__ cells_n) {
  constexpr int NW = CM_BLK / WAVE;
  // Double-buffered by chunk parity: two barriers per chunk suffice.
  __shared__ int s_wave[2][NW];
  __shared__ int s_base[2];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const bool vec = (((uintptr_t)tkeys) & 15) == 0;
  const int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  int par = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x, par ^= 1) {
    // Slot of k[q]: s0 + (q / 2) * (CM_BLK * 2) + (q & 1).
    const int64_t s0 = c * CM_CHUNK + threadIdx.x * 2;
    uint64_t k[CM_PER];
    for (int j = 0; j < CM_PER / 2; ++j) {
      int64_t s = s0 + (int64_t)j * (CM_BLK * 2);
      if (vec && s + 1 < nslots) {
        ulonglong2 kk = *(const ulonglong2*)(tkeys + s);
        k[2 * j] = kk.x;
        k[2 * j + 1] = kk.y;
      } else {
        for (int q = 0; q < 2; ++q) {
          k[2 * j + q] = s + q < nslots ? tkeys[s + q] : EMPTY_SLOT;
        }
      }
    }
    unsigned takem = 0;
    for (int q = 0; q < CM_PER; ++q) {
      if (k[q] == EMPTY_SLOT) continue;
      int64_t win = (int64_t)(int32_t)(uint32_t)(k[q] >> 32);
      if (win >= win_lo && win < win_hi) takem |= 1u << q;
    }
    const int cnt = __popc(takem);
    int incl = cnt;
    for (int off = 1; off < WAVE; off <<= 1) {
      int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == WAVE - 1) s_wave[par][wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < NW; ++w) total += s_wave[par][w];
      s_base[par] = total > 0 ? atomicAdd(cells_n, total) : 0;
    }
    __syncthreads();
    if (takem != 0) {
      int64_t idx = (int64_t)s_base[par] + (incl - cnt);
      for (int w = 0; w < wave; ++w) idx += s_wave[par][w];
      for (int q = 0; q < CM_PER; ++q) {
        if (!((takem >> q) & 1u)) continue;
        if (idx < nslots) {
          int64_t s = s0 + (int64_t)(q >> 1) * (CM_BLK * 2) + (q & 1);
          int2 nn = *(const int2*)(tcnt + 2 * s);
          cell_pk[idx] = k[q];
          *(int2*)(cell_n + 2 * idx) = nn;
          slot_cell[s] = (int)idx;
        }
        ++idx;
      }
    }
  }
}

// The gather pass of the product-join close over one side's log (see
// above).  `tkeys` / `tcnt` are the retired table: found, never
// claimed, and the side's counts of due cells counted down to zero.
// `n*` is the fresh state.  The guards only fire if the host's
// bookkeeping is wrong; they keep every store inside its array.
__global__ void k_wjprod_gather(
    const ulonglong2* __restrict__ log,
    int64_t n,
    int side,
    const uint64_t* __restrict__ tkeys,
    int* __restrict__ tcnt,
    uint64_t mask,
    int64_t win_lo,
    int64_t win_hi,
    const int* __restrict__ slot_cell,
    const int* __restrict__ cell_n,
    const int64_t* __restrict__ val_end,
    int64_t ncells,
    int64_t* __restrict__ arena,
    int64_t arena_n,
    uint64_t* __restrict__ nkeys,
    int* __restrict__ ncnt,
    ulonglong2* __restrict__ nlog,
    int* __restrict__ nlog_n,
    int64_t nlog_cap,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    const ulonglong2 e = log[i];
    const int64_t win = (int64_t)(int32_t)(uint32_t)(e.x >> 32);
    if (win >= win_lo && win < win_hi) {
      uint64_t slot = lookup_slot(tkeys, mask, e.x);
      int64_t c = slot != ~0ULL ? (int64_t)slot_cell[slot] : -1;
      bool stored = false;
      if (c >= 0 && c < ncells) {
        const int n0 = cell_n[2 * c], n1 = cell_n[2 * c + 1];
        const int pos = atomicSub(&tcnt[2 * slot + side], 1) - 1;
        const int64_t at =
            val_end[c] - n0 - n1 + (side ? (int64_t)n0 : 0) + pos;
        if (pos >= 0 && pos < (side ? n1 : n0) && at >= 0 && at < arena_n) {
          arena[at] = (int64_t)e.y;
          stored = true;
        }
      }
      if (!stored) atomicOr(error_flag, ERR_WJPROD_BOUND);
    }
    wjprod_put(win >= win_hi, e.x, (int64_t)e.y, nkeys, ncnt, mask, side,
               nlog, nlog_n, nlog_cap, error_flag);
  }
}

// The expand pass of the product-join close: one thread per output
// row, grid-stride.  Row `r` belongs to the cell `c` with
// row_end[c - 1] <= r < row_end[c] (an upper-bound search; a cell has
// at least one row, so the bounds strictly increase); within it the
// rows run over the left list in the slow index and the right list in
// the fast one, an empty side standing for one absent value.  All row
// arithmetic is 64-bit: one cell can pass 2^31 rows.  Consecutive rows
// are consecutive addresses in every output column.
__global__ void k_wjprod_expand(
    int64_t nrows,
    int64_t ncells,
    const int64_t* __restrict__ row_end,
    const int64_t* __restrict__ val_end,
    const uint64_t* __restrict__ cell_pk,
    const int* __restrict__ cell_n,
    const int64_t* __restrict__ arena,
    int32_t* __restrict__ out_keys,
    int32_t* __restrict__ out_wins,
    int64_t* __restrict__ out_v0,
    int64_t* __restrict__ out_v1,
    int32_t* __restrict__ out_mask) {
  int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; r < nrows; r += stride) {
    int64_t lo = 0, hi = ncells - 1;  // row_end[ncells - 1] == nrows > r
    while (lo < hi) {
      int64_t mid = (lo + hi) >> 1;
      if (row_end[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int64_t c = lo;
    const int64_t n0 = cell_n[2 * c], n1 = cell_n[2 * c + 1];
    const int64_t m1 = n1 > 0 ? n1 : 1;
    const int64_t local = r - (c > 0 ? row_end[c - 1] : 0);
    const int64_t a = val_end[c] - n0 - n1;
    const uint64_t pk = cell_pk[c];
    out_keys[r] = (int32_t)(uint32_t)(pk & 0xFFFFFFFFULL);
    out_wins[r] = (int32_t)(uint32_t)(pk >> 32);
    out_v0[r] = n0 > 0 ? arena[a + local / m1] : 0;
    out_v1[r] = n1 > 0 ? arena[a + n0 + local % m1] : 0;
    out_mask[r] = (n0 > 0 ? 1 : 0) | (n1 > 0 ? 2 : 0);
  }
}

// ---------------------------------------------------------------------------
// Session windows (gap-based).  Per-key state is one table cell:
// (session_start, last_ts, accumulator).  Batches arrive SORTED by
// (key, ts) — the host wrapper sorts — and one thread walks each
// key's contiguous segment in order: a gap > gap_ms closes the
// running session (emit) and starts a new one.  Parallelism is the
// distinct-key count of the batch, which is the right shape for the
// high-cardinality workloads the device path targets (low-cardinality
// session streams belong on the host path).
//
// Reference semantics: bytewax windowing.py _SessionWindowerLogic
// (gap merge); here in-order ingestion makes merges degenerate to
// extension, matching the reference under watermark-ordered input.

// Table layout: skeys int64 (EMPTY_SLOT = empty), svals 3x int64 per
// slot (start, last, acc).
__device__ inline uint64_t session_find_or_claim(
    uint64_t* skeys, uint64_t mask, uint64_t key) {
  uint64_t h = mix64(key);
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    uint64_t slot = (h + probe) & mask;
    uint64_t cur = skeys[slot];
    if (cur == key) return slot;
    if (cur == EMPTY_SLOT) {
      uint64_t prev = atomicCAS(
          (unsigned long long*)&skeys[slot], EMPTY_SLOT, key);
      if (prev == EMPTY_SLOT || prev == key) return slot;
    }
  }
  return ~0ULL;
}

template <int MODE>
__global__ void k_session_insert(
    const int32_t* __restrict__ keys,   // sorted by (key, ts)
    const int64_t* __restrict__ ts,
    const int64_t* __restrict__ vals,
    const int64_t* __restrict__ seg_start,  // [n_segs] segment offsets
    const int64_t* __restrict__ seg_end,
    int64_t n_segs,
    int64_t gap_ms,
    uint64_t* __restrict__ skeys,
    long long* __restrict__ sstart,
    long long* __restrict__ slast,
    long long* __restrict__ sacc,
    uint64_t mask,
    int32_t* __restrict__ out_keys,  // closed sessions
    int64_t* __restrict__ out_start,
    int64_t* __restrict__ out_end,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t out_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag) {
  int64_t seg = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; seg < n_segs; seg += stride) {
    int64_t i = seg_start[seg];
    int64_t end = seg_end[seg];
    if (i >= end) continue;
    uint64_t key = (uint64_t)(uint32_t)keys[i];
    uint64_t slot = session_find_or_claim(skeys, mask, key);
    if (slot == ~0ULL) {
      atomicOr(error_flag, 1);
      continue;
    }
    // This thread owns the key's whole segment; no other thread
    // touches this slot within the launch.
    long long start = sstart[slot];
    long long last = slast[slot];
    long long acc = sacc[slot];
    bool open = last >= 0;
    for (; i < end; ++i) {
      int64_t t = ts[i];
      int64_t v = (MODE == AGG_SUM) ? vals[i] : 1;
      if (open && t - last > gap_ms) {
        int idx = atomicAdd(out_n, 1);
        if (idx < out_cap) {
          out_keys[idx] = (int32_t)(uint32_t)key;
          out_start[idx] = start;
          out_end[idx] = last;
          out_vals[idx] = acc;
        } else {
          atomicOr(error_flag, 1);
        }
        open = false;
      }
      if (!open) {
        start = t;
        acc = 0;
        open = true;
      }
      last = t;
      acc += v;
    }
    sstart[slot] = start;
    slast[slot] = last;
    sacc[slot] = acc;
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      long long other = __shfl_down(last, off);
      if (other > last) last = other;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      atomicMax(max_ts, (unsigned long long)last);
    }
  }
}

// Close sessions whose last event is older than `horizon_ms` (the
// watermark minus the gap): emit and clear the cell.  Clearing is
// safe here, unlike the windowed table, because the NEXT insert
// re-claims slots via CAS (session_find_or_claim tolerates probe
// holes by claiming the first empty slot; a key displaced past a
// cleared hole simply occupies two probes' worth of distance — the
// chain is never read without the CAS claim).  To keep lookups exact
// we still migrate live cells to the alternate table, mirroring the
// windowed close.
__global__ void k_session_close_migrate(
    const uint64_t* __restrict__ skeys,
    const long long* __restrict__ sstart,
    const long long* __restrict__ slast,
    const long long* __restrict__ sacc,
    int64_t nslots,
    int64_t horizon_ms,
    uint64_t* __restrict__ dst_keys,
    long long* __restrict__ dst_start,
    long long* __restrict__ dst_last,
    long long* __restrict__ dst_acc,
    uint64_t mask,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_start,
    int64_t* __restrict__ out_end,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < nslots; i += stride) {
    uint64_t key = skeys[i];
    if (key == EMPTY_SLOT) continue;
    long long last = slast[i];
    if (last < 0) continue;
    if (last < horizon_ms) {
      int idx = atomicAdd(out_n, 1);
      if (idx < out_cap) {
        out_keys[idx] = (int32_t)(uint32_t)key;
        out_start[idx] = sstart[i];
        out_end[idx] = last;
        out_vals[idx] = sacc[i];
      } else {
        atomicOr(error_flag, 1);
      }
    } else {
      uint64_t slot = session_find_or_claim(dst_keys, mask, key);
      if (slot == ~0ULL) {
        atomicOr(error_flag, 1);
        continue;
      }
      dst_start[slot] = sstart[i];
      dst_last[slot] = last;
      dst_acc[slot] = sacc[i];
    }
  }
}

// ---------------------------------------------------------------------------
// Out-of-order session windows: up to `max_open` open sessions per
// key.  Table layout: skeys[nslots], scnt[nslots] (open sessions in
// the cell) and start/last/acc of shape [nslots, max_open], sessions
// sorted by start inside a cell and separated by more than the gap.
//
// An insert is three launches over the (key, ts)-sorted batch:
//   k_session_run_count    per-block count of run heads
//   k_session_run_collapse one (key, start, last, acc) record per run
//   k_session_run_merge    two-pointer merge of a key's runs into its
//                          cell, coalescing across the gap
// The first two are parallel over events, the third over runs; insert
// never closes a session (an event may still bridge two of them), so
// only k_session_multi_close_migrate emits.

#define SESS_RUN_BLK 256
#define SESS_ERR_TABLE 1
#define SESS_ERR_MAX_OPEN 2

// Event i starts a run iff it is the first event, the first of its
// key, or more than the gap after its predecessor.
__device__ inline bool session_run_head(
    const int32_t* __restrict__ keys, const int64_t* __restrict__ ts,
    int64_t i, int64_t gap_ms) {
  if (i == 0) return true;
  if (keys[i] != keys[i - 1]) return true;
  return ts[i] - ts[i - 1] > gap_ms;
}

__global__ __launch_bounds__(SESS_RUN_BLK) void k_session_run_count(
    const int32_t* __restrict__ keys,  // sorted by (key, ts)
    const int64_t* __restrict__ ts,
    int64_t n,
    int64_t gap_ms,
    int* __restrict__ block_heads) {
  __shared__ int wave_cnt[SESS_RUN_BLK / WAVE];
  int64_t i = blockIdx.x * (int64_t)SESS_RUN_BLK + threadIdx.x;
  int lane = threadIdx.x & (WAVE - 1);
  int wave = threadIdx.x / WAVE;
  bool head = i < n && session_run_head(keys, ts, i, gap_ms);
  unsigned long long ball = __ballot(head);
  if (lane == 0) wave_cnt[wave] = __popcll(ball);
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < SESS_RUN_BLK / WAVE; ++w) total += wave_cnt[w];
    block_heads[blockIdx.x] = total;
  }
}

// Pass B: recompute the head flags, rank them (ballot/popcount inside
// the wave, LDS offsets across waves, `block_off` across blocks) and
// write one record per run in sorted order.  Every event knows its
// run id (heads at or before it, minus one), so no thread loops over
// a run: heads write key/start, tails write last, and the accumulator
// is tail index minus head index (COUNT) or a wave-level segmented
// shuffle reduction with one int64 atomicAdd per (wave, run) (SUM —
// integer adds, so exact and order-independent).  `run_acc` arrives
// zeroed.
template <int MODE>
__global__ __launch_bounds__(SESS_RUN_BLK) void k_session_run_collapse(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ ts,
    const int64_t* __restrict__ vals,
    int64_t n,
    int64_t gap_ms,
    const int64_t* __restrict__ block_off,  // exclusive scan of heads
    int32_t* __restrict__ run_key,
    long long* __restrict__ run_start,
    long long* __restrict__ run_last,
    unsigned long long* __restrict__ run_acc) {
  __shared__ int wave_cnt[SESS_RUN_BLK / WAVE];
  int64_t i = blockIdx.x * (int64_t)SESS_RUN_BLK + threadIdx.x;
  int lane = threadIdx.x & (WAVE - 1);
  int wave = threadIdx.x / WAVE;
  bool in = i < n;
  bool head = in && session_run_head(keys, ts, i, gap_ms);
  unsigned long long ball = __ballot(head);
  if (lane == 0) wave_cnt[wave] = __popcll(ball);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wave_cnt[w];
  unsigned long long le =
      lane == WAVE - 1 ? ~0ULL : ((1ULL << (lane + 1)) - 1ULL);
  // Event 0 is a head, so every in-range event has rid >= 0.
  int64_t rid =
      in ? block_off[blockIdx.x] + before + __popcll(ball & le) - 1 : -1;
  bool tail = false;
  if (in) {
    tail = i == n - 1 || keys[i + 1] != keys[i] ||
           ts[i + 1] - ts[i] > gap_ms;
    if (head) {
      run_key[rid] = keys[i];
      run_start[rid] = ts[i];
    }
    if (tail) run_last[rid] = ts[i];
  }
  if (MODE == AGG_COUNT) {
    long long d = (tail ? i + 1 : 0) - (head ? i : 0);
    if (d != 0) atomicAdd(&run_acc[rid], (unsigned long long)d);
  } else {
    long long v = in ? vals[i] : 0;
    // rid is non-decreasing across the wave: a segmented suffix sum.
    for (int off = 1; off < WAVE; off <<= 1) {
      long long ov = __shfl_down(v, off);
      long long orid = __shfl_down((long long)rid, off);
      if (lane + off < WAVE && orid == rid) v += ov;
    }
    long long prid = __shfl_up((long long)rid, 1);
    if (in && (lane == 0 || prid != rid)) {
      atomicAdd(&run_acc[rid], (unsigned long long)v);
    }
  }
}

// One thread per run; only the first run of a key acts, and takes the
// key's following runs with it, so one thread owns a key (and, after
// the CAS claim, its cell) for the whole launch.  The merged list is
// staged in LDS ([session][thread], conflict-free) rather than in
// private arrays.  More than MAX_OPEN sessions raise the flag and
// leave the cell as it was.
template <int MAX_OPEN>
__global__ __launch_bounds__(WAVE) void k_session_run_merge(
    const int32_t* __restrict__ run_key,
    const long long* __restrict__ run_start,
    const long long* __restrict__ run_last,
    const long long* __restrict__ run_acc,
    const int64_t* __restrict__ n_runs_p,
    int64_t run_cap,
    int64_t gap_ms,
    uint64_t* __restrict__ skeys,
    int* __restrict__ scnt,
    long long* __restrict__ sstart,
    long long* __restrict__ slast,
    long long* __restrict__ sacc,
    uint64_t mask,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag) {
  __shared__ long long l_start[MAX_OPEN][WAVE];
  __shared__ long long l_last[MAX_OPEN][WAVE];
  __shared__ long long l_acc[MAX_OPEN][WAVE];
  int tid = threadIdx.x;
  int64_t n_runs = *n_runs_p;
  if (n_runs > run_cap) n_runs = run_cap;
  int64_t stride = gridDim.x * (int64_t)WAVE;
  long long mx = 0;
  for (int64_t r = blockIdx.x * (int64_t)WAVE + tid; r < n_runs;
       r += stride) {
    long long rl = run_last[r];
    if (rl > mx) mx = rl;
    int32_t k = run_key[r];
    if (r > 0 && run_key[r - 1] == k) continue;
    uint64_t slot =
        session_find_or_claim(skeys, mask, (uint64_t)(uint32_t)k);
    if (slot == ~0ULL) {
      atomicOr(error_flag, SESS_ERR_TABLE);
      continue;
    }
    int c = scnt[slot];
    if (c > MAX_OPEN) c = MAX_OPEN;
    long long* cs = sstart + slot * MAX_OPEN;
    long long* cl = slast + slot * MAX_OPEN;
    long long* ca = sacc + slot * MAX_OPEN;
    int a = 0;
    int64_t b = r;
    int m = 0;
    bool have = false;
    long long cur_s = 0, cur_l = 0, cur_a = 0;
    while (true) {
      bool ha = a < c;
      bool hb = b < n_runs && run_key[b] == k;
      if (!ha && !hb) break;
      long long ns, nl, na;
      if (ha && (!hb || cs[a] <= run_start[b])) {
        ns = cs[a];
        nl = cl[a];
        na = ca[a];
        ++a;
      } else {
        ns = run_start[b];
        nl = run_last[b];
        na = run_acc[b];
        ++b;
      }
      if (have && ns - cur_l <= gap_ms) {
        if (nl > cur_l) cur_l = nl;
        cur_a += na;
      } else {
        if (have) {
          if (m < MAX_OPEN) {
            l_start[m][tid] = cur_s;
            l_last[m][tid] = cur_l;
            l_acc[m][tid] = cur_a;
          }
          ++m;
        }
        cur_s = ns;
        cur_l = nl;
        cur_a = na;
        have = true;
      }
    }
    if (have) {
      if (m < MAX_OPEN) {
        l_start[m][tid] = cur_s;
        l_last[m][tid] = cur_l;
        l_acc[m][tid] = cur_a;
      }
      ++m;
    }
    if (m > MAX_OPEN) {
      atomicOr(error_flag, SESS_ERR_MAX_OPEN);
      continue;
    }
    for (int j = 0; j < m; ++j) {
      cs[j] = l_start[j][tid];
      cl[j] = l_last[j][tid];
      ca[j] = l_acc[j][tid];
    }
    scnt[slot] = m;
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    long long other = __shfl_down(mx, off);
    if (other > mx) mx = other;
  }
  if (tid == 0 && mx > 0) atomicMax(max_ts, (unsigned long long)mx);
}

// Per slot: sessions in a cell are sorted and gap-separated, so the
// closable ones (last < horizon) form a prefix.  Emit the prefix,
// compact the rest to the front of the key's cell in the alternate
// table.
__global__ void k_session_multi_close_migrate(
    const uint64_t* __restrict__ skeys,
    const int* __restrict__ scnt,
    const long long* __restrict__ sstart,
    const long long* __restrict__ slast,
    const long long* __restrict__ sacc,
    int64_t nslots,
    int max_open,
    int64_t horizon_ms,
    uint64_t* __restrict__ dst_keys,
    int* __restrict__ dst_cnt,
    long long* __restrict__ dst_start,
    long long* __restrict__ dst_last,
    long long* __restrict__ dst_acc,
    uint64_t mask,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_start,
    int64_t* __restrict__ out_end,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < nslots; i += stride) {
    uint64_t key = skeys[i];
    if (key == EMPTY_SLOT) continue;
    int c = scnt[i];
    if (c > max_open) c = max_open;
    if (c <= 0) continue;
    int64_t base = i * max_open;
    int p = 0;
    while (p < c && slast[base + p] < horizon_ms) ++p;
    if (p > 0) {
      int idx = atomicAdd(out_n, p);
      for (int j = 0; j < p; ++j) {
        if ((int64_t)idx + j < out_cap) {
          out_keys[idx + j] = (int32_t)(uint32_t)key;
          out_start[idx + j] = sstart[base + j];
          out_end[idx + j] = slast[base + j];
          out_vals[idx + j] = sacc[base + j];
        } else {
          atomicOr(error_flag, SESS_ERR_TABLE);
        }
      }
    }
    if (p < c) {
      uint64_t slot = session_find_or_claim(dst_keys, mask, key);
      if (slot == ~0ULL) {
        atomicOr(error_flag, SESS_ERR_TABLE);
        continue;
      }
      int64_t dbase = (int64_t)slot * max_open;
      for (int j = p; j < c; ++j) {
        dst_start[dbase + j - p] = sstart[base + j];
        dst_last[dbase + j - p] = slast[base + j];
        dst_acc[dbase + j - p] = sacc[base + j];
      }
      dst_cnt[slot] = c - p;
    }
  }
}

// Stream compaction: keep events where mask != 0, preserving relative
// order per wave (wave-ballot ranks + one atomic per wave).
__global__ void k_filter_compact(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ ts,
    const int64_t* __restrict__ vals,  // may be nullptr
    const uint8_t* __restrict__ mask,
    int64_t n,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_ts,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n) {
  int lane = threadIdx.x & (WAVE - 1);
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = first; i - lane < n; i += stride) {
    bool keep = (i < n) && mask[i] != 0;
    unsigned long long ball = __ballot(keep);
    if (ball == 0) continue;
    int wave_total = __popcll(ball);
    int rank = __popcll(ball & ((1ULL << lane) - 1ULL));
    int base = 0;
    int lead = __ffsll(ball) - 1;
    if (lane == lead) base = atomicAdd(out_n, wave_total);
    base = __shfl(base, lead);
    if (keep) {
      int64_t o = base + rank;
      out_keys[o] = keys[i];
      out_ts[o] = ts[i];
      if (vals != nullptr) out_vals[o] = vals[i];
    }
  }
}

// Histogram of destination workers for the keyed exchange.
__global__ void k_bucket_hist(
    const int32_t* __restrict__ keys,
    int64_t n,
    int world,
    int* __restrict__ counts) {
  extern __shared__ int lcounts[];
  for (int w = threadIdx.x; w < world; w += blockDim.x) lcounts[w] = 0;
  __syncthreads();
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int dst = (int)(mix64((uint32_t)keys[i]) % (uint64_t)world);
    atomicAdd(&lcounts[dst], 1);
  }
  __syncthreads();
  for (int w = threadIdx.x; w < world; w += blockDim.x) {
    if (lcounts[w] > 0) atomicAdd(&counts[w], lcounts[w]);
  }
}

// Scatter events into per-destination contiguous segments.
// `cursors` must be pre-loaded with the exclusive prefix sums of the
// destination counts.  Order within a destination is not preserved
// (items within an epoch are unordered).
template <typename TS = int64_t>
__global__ void k_bucket_scatter(
    const int32_t* __restrict__ keys,
    const TS* __restrict__ ts,
    const int64_t* __restrict__ vals,  // may be nullptr
    int64_t n,
    int world,
    int* __restrict__ cursors,
    int32_t* __restrict__ out_keys,
    TS* __restrict__ out_ts,
    int64_t* __restrict__ out_vals) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int32_t k = keys[i];
    int dst = (int)(mix64((uint32_t)k) % (uint64_t)world);
    int idx = atomicAdd(&cursors[dst], 1);
    out_keys[idx] = k;
    out_ts[idx] = ts[i];
    if (vals != nullptr) out_vals[idx] = vals[i];
  }
}

// ---------------------------------------------------------------------------
// String dictionary encode (str keys -> dense int32 ids, on device).
//
// The reference's key contract is `str` (reference src/operators.rs:
// 363-439 extract_key); the columnar fast path keys RecordBatches by
// int32 id.  These kernels bridge the two: string bytes (+offsets)
// land on device once, each string is 128-bit hashed and mapped to a
// dense id through an open-address device dictionary.
//
// Exactness: the device table stores the full 128-bit hash (lo is
// the CAS claim word, hi the published check word).  Newly created
// ids are read back as (id, batch_index) pairs so the host keeps the
// authoritative id->string list.  Key identity on the device path IS
// 128-bit hash equality: nothing compares string bytes, so two
// strings with equal (lo, hi) would share an id silently
// (probability ~1e-26 at 1e6 keys).  Two strings with equal lo only
// are told apart by hi: the second one never finds a slot of its own
// and surfaces as DICT_ERR_MISS.
//
// Errors are a bit set in `error_flag`, every bit set with atomicOr so
// that none overwrites another (bytewax_amd/gpu/strings.py reports
// them by priority: a full table also makes the lookup miss).
//
// Race-free without spins: insert and lookup are SEPARATE kernel
// launches.  k_dict_insert only guarantees every distinct string has
// a claimed slot with published (hi, id) by kernel end (threads that
// lose the CAS to the same hash exit; the winner's hi/id stores are
// globally visible at the kernel boundary).  k_dict_lookup then
// resolves every event's id with plain loads.
// ---------------------------------------------------------------------------

// `error_flag` bits of the dictionary kernels (DICT_ERR_* in
// bytewax_amd/gpu/strings.py).
#define DICT_ERR_FULL 1    // no free slot left for a new string
#define DICT_ERR_MISS 2    // lookup found no published (lo, hi) cell
#define DICT_ERR_NEWCAP 4  // more new ids than the readback buffer holds

__device__ __forceinline__ void str_hash128(
    const uint8_t* __restrict__ s, int len, uint64_t* h_lo,
    uint64_t* h_hi) {
  // FNV-1a over the bytes, finalized twice with independent seeds.
  uint64_t h = 0xcbf29ce484222325ULL;
  for (int i = 0; i < len; ++i) {
    h ^= (uint64_t)s[i];
    h *= 0x100000001b3ULL;
  }
  uint64_t lo = mix64(h ^ 0x9e3779b97f4a7c15ULL);
  if (lo == EMPTY_SLOT) lo = 0;  // reserve the empty sentinel
  *h_lo = lo;
  *h_hi = mix64(h + 0x2545f4914f6cdd1dULL);
}

__global__ void k_dict_insert(
    const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ offs,  // [n+1]
    int64_t n,
    uint64_t* __restrict__ dlo,   // [nslots] CAS claim words
    uint64_t* __restrict__ dhi,   // [nslots] published check words
    int32_t* __restrict__ dids,   // [nslots] published ids
    uint64_t mask,
    int* __restrict__ counter,        // next id
    int32_t* __restrict__ new_ids,    // [new_cap] readback: id
    int32_t* __restrict__ new_idx,    // [new_cap] readback: batch index
    int* __restrict__ new_n,
    int64_t new_cap,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int len = (int)(offs[i + 1] - offs[i]);
    uint64_t lo, hi;
    str_hash128(bytes + offs[i], len, &lo, &hi);
    uint64_t h = lo & mask;
    for (uint64_t probes = 0; probes <= mask; ++probes) {
      uint64_t cur = dlo[h];
      if (cur == lo) break;  // claimed (here or elsewhere): winner publishes
      if (cur == EMPTY_SLOT) {
        uint64_t prev = atomicCAS((unsigned long long*)&dlo[h],
                                  EMPTY_SLOT, lo);
        if (prev == EMPTY_SLOT) {
          int id = atomicAdd(counter, 1);
          dhi[h] = hi;
          dids[h] = id;
          int r = atomicAdd(new_n, 1);
          if (r < new_cap) {
            new_ids[r] = id;
            new_idx[r] = (int32_t)i;
          } else {
            atomicOr(error_flag, DICT_ERR_NEWCAP);
          }
          break;
        }
        if (prev == lo) break;
      }
      h = (h + 1) & mask;
      if (probes == mask) atomicOr(error_flag, DICT_ERR_FULL);
    }
  }
}

__global__ void k_dict_lookup(
    const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ offs,
    int64_t n,
    const uint64_t* __restrict__ dlo,
    const uint64_t* __restrict__ dhi,
    const int32_t* __restrict__ dids,
    uint64_t mask,
    int32_t* __restrict__ out_ids,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int len = (int)(offs[i + 1] - offs[i]);
    uint64_t lo, hi;
    str_hash128(bytes + offs[i], len, &lo, &hi);
    uint64_t h = lo & mask;
    int32_t id = -1;
    for (uint64_t probes = 0; probes <= mask; ++probes) {
      uint64_t cur = dlo[h];
      if (cur == lo && dhi[h] == hi) {
        id = dids[h];
        break;
      }
      if (cur == EMPTY_SLOT) break;
      h = (h + 1) & mask;
    }
    out_ids[i] = id;
    if (id < 0) atomicOr(error_flag, DICT_ERR_MISS);
  }
}

// Restore path: re-claim slots with PINNED ids (snapshot order must
// be reproduced exactly across restarts).
__global__ void k_dict_insert_pinned(
    const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ offs,
    const int32_t* __restrict__ ids,
    int64_t n,
    uint64_t* __restrict__ dlo,
    uint64_t* __restrict__ dhi,
    int32_t* __restrict__ dids,
    uint64_t mask,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int len = (int)(offs[i + 1] - offs[i]);
    uint64_t lo, hi;
    str_hash128(bytes + offs[i], len, &lo, &hi);
    uint64_t h = lo & mask;
    for (uint64_t probes = 0; probes <= mask; ++probes) {
      uint64_t prev = atomicCAS((unsigned long long*)&dlo[h],
                                EMPTY_SLOT, lo);
      if (prev == EMPTY_SLOT) {
        dhi[h] = hi;
        dids[h] = ids[i];
        break;
      }
      h = (h + 1) & mask;
      if (probes == mask) atomicOr(error_flag, DICT_ERR_FULL);
    }
  }
}

// ---------------------------------------------------------------------------
// String exchange: route raw string bytes to their owning rank by
// CONTENT hash, so multi-GPU str-keyed streams encode at the owner
// and dictionary ids never cross ranks (bytewax_amd/gpu/strings.py).
// Wire order is bucket-major: lengths/ts/vals in per-destination
// contiguous segments, bytes packed in the same relative order
// (receivers rebuild offsets with a cumsum over lengths).
// ---------------------------------------------------------------------------

__device__ __forceinline__ int str_owner(
    const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offs,
    int64_t i, int world) {
  uint64_t lo, hi;
  str_hash128(bytes + offs[i], (int)(offs[i + 1] - offs[i]), &lo, &hi);
  return (int)(hi % (uint64_t)world);
}

__global__ void k_str_bucket_hist(
    const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ offs,
    int64_t n,
    int world,
    int* __restrict__ counts,            // [world] strings
    long long* __restrict__ byte_counts  // [world] bytes
) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int dst = str_owner(bytes, offs, i, world);
    atomicAdd(&counts[dst], 1);
    atomicAdd((unsigned long long*)&byte_counts[dst],
              (unsigned long long)(offs[i + 1] - offs[i]));
  }
}

__global__ void k_str_meta_scatter(
    const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ offs,
    const int64_t* __restrict__ ts,
    const int64_t* __restrict__ vals,  // may be nullptr
    int64_t n,
    int world,
    int* __restrict__ cursors,  // [world] exclusive prefix of counts
    int32_t* __restrict__ send_lens,
    int64_t* __restrict__ send_ts,
    int64_t* __restrict__ send_vals,
    int32_t* __restrict__ src_idx) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    int dst = str_owner(bytes, offs, i, world);
    int pos = atomicAdd(&cursors[dst], 1);
    send_lens[pos] = (int32_t)(offs[i + 1] - offs[i]);
    send_ts[pos] = ts[i];
    if (vals != nullptr) send_vals[pos] = vals[i];
    src_idx[pos] = (int32_t)i;
  }
}

__global__ void k_str_byte_gather(
    const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ offs,
    const int32_t* __restrict__ src_idx,
    const int64_t* __restrict__ send_offs,  // [n] exclusive cumsum of lens
    int64_t n,
    uint8_t* __restrict__ send_bytes) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < n; j += stride) {
    int64_t i = src_idx[j];
    int64_t src = offs[i];
    int len = (int)(offs[i + 1] - src);
    int64_t dst = send_offs[j];
    for (int b = 0; b < len; ++b) send_bytes[dst + b] = bytes[src + b];
  }
}

// ---------------------------------------------------------------------------
// Host-side wrappers (torch extension API)
// ---------------------------------------------------------------------------

static void check_dev(const torch::Tensor& t, torch::ScalarType st,
                      const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == st, name, " has wrong dtype");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// Host view of the late-event side output (see late_append).  The
// insert launchers take a pointer: nullptr selects the default
// instantiations, exactly the launches the plain entry points always
// made.
struct LateSink {
  int64_t cutoff;
  int32_t* keys;
  int64_t* ts;
  int64_t* vals;  // nullptr for COUNT
  int* n;
  int64_t cap;
};

static LateSink make_late_sink(
    int64_t late_cutoff,
    torch::Tensor& late_keys,
    torch::Tensor& late_ts,
    c10::optional<torch::Tensor>& late_vals,
    torch::Tensor& late_n,
    bool need_vals) {
  check_dev(late_keys, torch::kInt32, "late_keys");
  check_dev(late_ts, torch::kInt64, "late_ts");
  check_dev(late_n, torch::kInt32, "late_n");
  int64_t cap = late_keys.numel();
  TORCH_CHECK(late_ts.numel() >= cap, "late_ts smaller than late_keys");
  TORCH_CHECK(late_n.numel() >= 1, "late_n must hold the cursor");
  int64_t* vp = nullptr;
  if (need_vals) {
    TORCH_CHECK(late_vals.has_value(), "late tracking needs late_vals");
    check_dev(*late_vals, torch::kInt64, "late_vals");
    TORCH_CHECK(late_vals->numel() >= cap,
                "late_vals smaller than late_keys");
    vp = late_vals->data_ptr<int64_t>();
  }
  return LateSink{late_cutoff, late_keys.data_ptr<int32_t>(),
                  late_ts.data_ptr<int64_t>(), vp,
                  late_n.data_ptr<int32_t>(), cap};
}

static void window_agg_insert_impl(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    bool dedup,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms,
    const LateSink* late) {
  TORCH_CHECK(late == nullptr || !dedup,
              "late tracking is incompatible with the dedup path");
  if (off_ms <= 0) off_ms = len_ms;
  TORCH_CHECK(off_ms <= len_ms, "window offset must be <= length");
  TORCH_CHECK(off_ms == len_ms || !dedup,
              "sliding windows are incompatible with the dedup path");
  check_dev(keys, torch::kInt32, "keys");
  bool ts32 = ts.scalar_type() == torch::kInt32;
  if (!ts32) check_dev(ts, torch::kInt64, "ts");
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(tvals, torch::kInt64, "tvals");
  check_dev(max_ts, torch::kInt64, "max_ts");
  check_dev(error_flag, torch::kInt32, "error_flag");
  int64_t n = keys.numel();
  TORCH_CHECK(ts.numel() == n, "ts/keys length mismatch");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(len_ms > 0, "window length must be positive");
  const int64_t* vptr = nullptr;
  if (mode == AGG_SUM) {
    TORCH_CHECK(vals.has_value(), "sum mode requires vals");
    check_dev(*vals, torch::kInt64, "vals");
    TORCH_CHECK(vals->numel() == n, "vals/keys length mismatch");
    vptr = vals->data_ptr<int64_t>();
  }
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  auto launch = [&](auto kern, auto tsptr) {
    hipLaunchKernelGGL(
        kern, grid, block, 0, stream,
        keys.data_ptr<int32_t>(), tsptr, vptr, n,
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(),
        (uint64_t)(nslots - 1), align_ms, len_ms, off_ms, ts_base,
        (int)region_bits,
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), (const int64_t*)nullptr,
        late ? late->cutoff : (int64_t)0, late ? late->keys : nullptr,
        late ? late->ts : nullptr, late ? late->vals : nullptr,
        late ? late->n : nullptr, late ? late->cap : (int64_t)0);
  };
  auto dispatch = [&](auto tsptr) {
    using TSV = std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
    if (late != nullptr && mode == AGG_COUNT)
      launch((k_window_agg_insert<AGG_COUNT, false, TSV, true>), tsptr);
    else if (late != nullptr)
      launch((k_window_agg_insert<AGG_SUM, false, TSV, true>), tsptr);
    else if (mode == AGG_COUNT && !dedup)
      launch(k_window_agg_insert<AGG_COUNT, false, TSV>, tsptr);
    else if (mode == AGG_COUNT && dedup)
      launch(k_window_agg_insert<AGG_COUNT, true, TSV>, tsptr);
    else if (mode == AGG_SUM && !dedup)
      launch(k_window_agg_insert<AGG_SUM, false, TSV>, tsptr);
    else
      launch(k_window_agg_insert<AGG_SUM, true, TSV>, tsptr);
  };
  if (ts32) dispatch(ts.data_ptr<int32_t>());
  else dispatch(ts.data_ptr<int64_t>());
}

void window_agg_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    bool dedup,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms) {
  window_agg_insert_impl(keys, ts, vals, tkeys, tvals, max_ts, error_flag,
                         align_ms, len_ms, mode, dedup, ts_base, region_bits,
                         off_ms, nullptr);
}

// Late-tracking form of window_agg_insert: events with absolute
// ts < late_cutoff are appended to (late_keys, late_ts[, late_vals])
// at the running cursor late_n instead of being folded (see
// late_append).  late_keys.numel() is the buffer capacity.
void window_agg_insert_late(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms,
    int64_t late_cutoff,
    torch::Tensor late_keys,
    torch::Tensor late_ts,
    c10::optional<torch::Tensor> late_vals,
    torch::Tensor late_n) {
  LateSink sink = make_late_sink(late_cutoff, late_keys, late_ts, late_vals,
                                 late_n, mode == AGG_SUM);
  window_agg_insert_impl(keys, ts, vals, tkeys, tvals, max_ts, error_flag,
                         align_ms, len_ms, mode, false, ts_base, region_bits,
                         off_ms, &sink);
}

static unsigned device_cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount,
                              dev) == hipSuccess &&
        v > 0)
      cus = v;
    else
      cus = 256;
  }
  return (unsigned)cus;
}

// BYTEWAX_AGG=wide selects the 16-byte-cell kernel for COUNT (A/B).
static bool agg_wide_env() {
  const char* s = std::getenv("BYTEWAX_AGG");
  return s != nullptr && s[0] == 'w';
}

// BYTEWAX_ENTRIES=classic keeps classic scatter entries, =hashed stops
// at the 8-byte hashed ones (A/B, tests).
static bool entries_classic_env() {
  const char* s = std::getenv("BYTEWAX_ENTRIES");
  return s != nullptr && s[0] == 'c';
}
static bool entries_hashed_env() {
  const char* s = std::getenv("BYTEWAX_ENTRIES");
  return s != nullptr && s[0] == 'h';
}

// Launch shape of k_radix_scatter_staged2 for `nseg` segments; false
// when the kernel cannot take them.
static bool staged2_shape(int64_t nseg, int* threads, int* u, size_t* lds) {
  int env_u = 0, env_threads = 0;
  if (const char* e = std::getenv("BYTEWAX_SCATTER_U")) env_u = atoi(e);
  if (const char* e = std::getenv("BYTEWAX_SCATTER_THREADS"))
    env_threads = atoi(e);
  *threads = env_threads == 1024 ? 1024 : 512;
  *u = *threads == 512 && env_u != 8 ? 16 : 8;
  *lds = staged2_lds_bytes(nseg, (int64_t)*threads * *u);
  return nseg <= *threads && *lds <= 160 * 1024;
}

// Whether launch_count_staged takes staged2 (tumbling windows, the
// kernel selected, its LDS fits, `ev_packed` 16-byte aligned).
static bool count_staged2_ok(int64_t xf, const void* evp, int64_t nseg) {
  int threads, u;
  size_t lds;
  return xf == 1 && scatter_staged2_env() && (((uintptr_t)evp) & 15) == 0 &&
         staged2_shape(nseg, &threads, &u, &lds);
}

// Whether launch_count_agg takes the compact-cell kernel.
static bool count_agg_compact(int64_t cap, int seg_bits) {
  return !agg_wide_env() && cap < ((int64_t)1 << 28) && seg_bits >= 8 &&
         seg_bits <= 13;
}

// What a COUNT scatter / aggregation pair agrees on for one scatter
// call: the entry format and, for hashed entries, the bases and the
// divider.  Every caller of launch_count_staged and launch_count_agg
// plans here and hands the plan to both, so the two launches cannot
// disagree.
struct CountEntries {
  bool hashed = false;  // hashed or compact: an entry base exists
  int dbits = 0;        // compact entries: their window-delta bits D
  int64_t W = 0;      // window id that y = 0 of the first segment is in
  uint32_t qoff = 0;  // entry base = W + qoff
  uint32_t dm = 0;    // divider for len_ms
  int sh1 = 0, sh2 = 0;
  bool compact() const { return dbits > 0; }
  int fmt() const {
    return compact() ? ENTRY_FMT_COMPACT
                     : hashed ? ENTRY_FMT_HASHED : ENTRY_FMT_CLASSIC;
  }
  // What launch_count_agg is told: the entry base, or "classic".
  int64_t agg_w() const {
    return hashed ? W + (int64_t)qoff : ENTRY_W_CLASSIC;
  }
};

// Window-delta bits of compact entries over `nseg` segments (nseg a
// power of two, at least 128).
static int compact_dbits(int64_t nseg) {
  int s = 0;
  while (((int64_t)1 << s) < nseg) ++s;
  return s - 1;
}

// Hashed entries need: the staged2 scatter in its default tile shape,
// the compact-cell aggregation, timestamps that are int32 deltas from a
// host-known base, a window length Win32 can divide by (below 2^31 ms),
// and no BYTEWAX_ENTRIES=classic.
//
// `staged_count`: the caller is about to call launch_count_staged
// (staged kind, COUNT, no late tracking).  `first_base`: ts_base of the
// call's first non-empty segment.  W lies 2^31 ms before it, rounded
// down to a window, so that c of that segment is in [2^31, 2^31 +
// len_ms) and nearly the whole int32 delta domain gives 0 <= y < 2^32.
// The entry base lies 2^18 windows before the window of `first_base`
// (but not before W), so the 19-bit entry delta reaches about as far
// back as forward.
//
// Compact entries need all of that and at least 128 segments (D >= 6);
// their base lies 2^(D-1) windows before the window of `first_base`.
// `allow_compact` is false for a caller whose aggregation side cannot
// be told the format, and for a state that has demoted itself.
static CountEntries plan_count_entries(
    bool staged_count, int64_t xf, const void* evp, int64_t nseg,
    int64_t cap, int seg_bits, bool ts_i32, int64_t align_ms,
    int64_t len_ms, int64_t first_base, bool allow_compact = true) {
  CountEntries ce;
  if (!staged_count || !ts_i32 || entries_classic_env() ||
      !count_staged2_ok(xf, evp, nseg) || !count_agg_compact(cap, seg_bits))
    return ce;
  if (len_ms < 1 || len_ms >= ((int64_t)1 << 31)) return ce;
  // Built for the default tile shape only.
  int threads, u;
  size_t lds;
  staged2_shape(nseg, &threads, &u, &lds);
  if (threads != 512 || u != 16) return ce;
  __int128 num = (__int128)first_base - align_ms - ((__int128)1 << 31);
  __int128 w = num / len_ms;
  if (num % len_ms < 0) w -= 1;  // floor
  if (w < -((__int128)1 << 62) || w > ((__int128)1 << 62)) return ce;
  ce.hashed = true;
  ce.W = (int64_t)w;
  int l = 0;
  while (((int64_t)1 << l) < len_ms) ++l;
  ce.dm = (uint32_t)((((unsigned __int128)1 << 32) *
                      (uint64_t)(((int64_t)1 << l) - len_ms)) /
                     (uint64_t)len_ms) + 1u;
  ce.sh1 = l < 1 ? l : 1;
  ce.sh2 = l > 1 ? l - 1 : 0;
  int64_t q0 = (int64_t)((num - w * len_ms + ((__int128)1 << 31)) / len_ms);
  int64_t back = (int64_t)1 << 18;
  if (allow_compact && !entries_hashed_env() && nseg >= 128 &&
      (nseg & (nseg - 1)) == 0 && (cap & ~(int64_t)(SCC_GRAN - 1)) > 0) {
    ce.dbits = compact_dbits(nseg);
    back = (int64_t)1 << (ce.dbits - 1);
  }
  ce.qoff = q0 > back ? (uint32_t)(q0 - back) : 0u;
  return ce;
}

// Win32 of one launch with base `ts_base` under the call's entry base.
static Win32 make_win32(
    const CountEntries& ce, int64_t ts_base, int64_t align_ms,
    int64_t len_ms) {
  Win32 w{};
  __int128 c = (__int128)ts_base - align_ms - (__int128)ce.W * len_ms;
  __int128 lo = -((__int128)1 << 31), hi = ((__int128)1 << 31) - 1;
  if (-c > lo) lo = -c;                                    // y >= 0
  if ((__int128)align_ms - ts_base > lo) lo = (__int128)align_ms - ts_base;
  __int128 top = ((__int128)1 << 32) - 1 - c;              // y < 2^32
  if (top < hi) hi = top;
  if (hi >= lo) {
    __int128 span = hi - lo + 1;
    if (span > 0xFFFFFFFFll) span = 0xFFFFFFFFll;
    w.dlo = (uint32_t)(int32_t)(int64_t)lo;
    w.dspan = (uint32_t)(uint64_t)span;
  }
  w.c = (uint32_t)(uint64_t)(c & 0xFFFFFFFFll);
  w.wlo = (uint32_t)(uint64_t)ce.W;
  w.qoff = ce.qoff;
  w.dm = ce.dm;
  w.sh1 = ce.sh1;
  w.sh2 = ce.sh2;
  return w;
}

// The one place that picks and launches the staged COUNT scatter
// without late tracking (tumbling or sliding; `xf` is the sliding
// expansion factor).  radix_window_insert, radix_scatter_only and the
// native step loop all come through here, so a variant is reachable,
// and the default, everywhere or nowhere.
//
// Tumbling windows take the write-combined kernel (staged2) when it is
// selected, its LDS fits a CU and `ev_packed` is 16-byte aligned;
// everything else takes k_radix_scatter_staged.  Knobs (A/B only):
// BYTEWAX_SCATTER_THREADS, BYTEWAX_SCATTER_U, BYTEWAX_SCATTER_BLOCKS.
template <typename TSV>
static void launch_count_staged(
    hipStream_t stream, const int32_t* keys, const TSV* ts, int64_t n,
    int64_t xf, int64_t align_ms, int64_t len_ms, int64_t off_ms,
    int64_t ts_base, uint64_t mask, int seg_bits, int64_t nseg, int64_t cap,
    int* gcur, uint64_t* evp, int* ovc, uint64_t* ovp, int64_t ov_cap,
    unsigned long long* max_ts, int* err, uint64_t win_m2,
    uint64_t win_maxfast, bool overlapped, const CountEntries& ce) {
  int env_u = 0, env_threads = 0, env_blocks = 0;
  if (const char* e = std::getenv("BYTEWAX_SCATTER_U")) env_u = atoi(e);
  if (const char* e = std::getenv("BYTEWAX_SCATTER_THREADS"))
    env_threads = atoi(e);
  if (const char* e = std::getenv("BYTEWAX_SCATTER_BLOCKS")) {
    int v = atoi(e);
    if (v > 0) env_blocks = v;
  }
  auto go = [&](auto kern, int threads, int u, unsigned cap_gs, size_t lds,
                auto... extra) {
    int64_t tile = (int64_t)threads * u;
    int64_t gs = (n * xf + tile - 1) / tile;
    if (env_blocks > 0) cap_gs = (unsigned)env_blocks;
    if (gs > (int64_t)cap_gs) gs = cap_gs;
    if (gs < 1) gs = 1;
    hipLaunchKernelGGL(
        kern, dim3((unsigned)gs), dim3((unsigned)threads), lds, stream, keys,
        ts, (const int64_t*)nullptr, n, align_ms, len_ms, off_ms, ts_base,
        mask, seg_bits, cap, gcur, evp, (int64_t*)nullptr, ovc, ovp,
        (int64_t*)nullptr, ov_cap, max_ts, err, win_m2, win_maxfast,
        extra...);
    // A refused launch (LDS budget, bad configuration) must not pass
    // for an empty batch.
    HIP_CHECK(hipGetLastError());
  };
  // `ce` comes from plan_count_entries, which asked the same question.
  TORCH_CHECK(!ce.hashed || count_staged2_ok(xf, evp, nseg),
              "hashed entries planned for a scatter that is not staged2");
  if (count_staged2_ok(xf, evp, nseg)) {
    // 512 x 16: one workgroup per CU (LDS-bound), 8192-event tiles.
    // 1024 x 8 keeps 16 waves per CU and measured 4 % faster alone
    // for staged2 before the next tile's columns were held in
    // registers (325 against 338 us); with them its 128-VGPR budget
    // spills 12 bytes per lane (36 with int64 timestamps), and the
    // compact kernel at 1024 x 8 spills 172 (it needs 234 VGPRs at
    // 512 x 16, where the budget is 256 and nothing spills).  The
    // hashed and the compact kernels are built at 512 x 16 only.
    // One block per CU, each walking its share of the tiles: measured
    // fastest when the scatter has the chip to itself (1024 x 8: 325
    // us at 256 blocks, 351 at 512, 407 at 1024 for the 64M-event
    // batch), and the padded final flush shrinks with it.
    // `overlapped`: the caller runs the aggregation of the previous
    // batch on another stream meanwhile.  Its 128 KB workgroups cannot
    // share a CU with this kernel's, so some blocks start late; two
    // blocks per CU halve the share a late block drags behind it.
    const unsigned cus = device_cu_count() * (overlapped ? 2u : 1u);
    int threads, u;
    size_t lds;
    staged2_shape(nseg, &threads, &u, &lds);
    Win32 w32{};
    if constexpr (sizeof(TSV) == 4) {
      if (ce.hashed) {
        // Planned for the default shape only.
        w32 = make_win32(ce, ts_base, align_ms, len_ms);
        if (ce.compact()) {
          TORCH_CHECK(nseg == ((int64_t)2 << ce.dbits) && nseg <= 512,
                      "compact entries planned for another segment count");
          TORCH_CHECK(32 + ce.dbits >= MIXN_PAIR_MIN_N &&
                          32 + ce.dbits <= MIXN_PAIR_MAX_N,
                      "compact entries: hash width outside mixn_pair's range");
          int64_t gs = (n + 8191) / 8192;
          unsigned cap_gs = env_blocks > 0 ? (unsigned)env_blocks : cus;
          if (gs > (int64_t)cap_gs) gs = cap_gs;
          if (gs < 1) gs = 1;
          // 16-byte column loads need both columns 16-byte aligned; a
          // per-source-rank segment of a receive buffer need not be.
          const bool vec = (((uintptr_t)keys | (uintptr_t)ts) & 15) == 0;
          auto launch = [&](auto kern) {
            // Granules of 16 entries: both launches round `cap` down.
            hipLaunchKernelGGL(
                kern, dim3((unsigned)gs), dim3(512),
                compact_lds_bytes(nseg, 8192), stream, keys, ts, n, align_ms,
                len_ms, ts_base, ce.dbits, cap & ~(int64_t)(SCC_GRAN - 1),
                gcur, (uint32_t*)evp, ovc, ovp, ov_cap, max_ts, err, win_m2,
                win_maxfast, w32);
          };
          if (vec) launch(k_radix_scatter_compact<16, 512, true>);
          else launch(k_radix_scatter_compact<16, 512, false>);
          HIP_CHECK(hipGetLastError());
          return;
        }
        go((k_radix_scatter_staged2<TSV, 16, 512, true>), 512, 16, cus, lds,
           w32);
        return;
      }
    }
    TORCH_CHECK(!ce.hashed, "hashed entries need int32 timestamp deltas");
    if (threads == 1024)
      go((k_radix_scatter_staged2<TSV, 8, 1024>), 1024, 8, cus, lds, w32);
    else if (u == 16)
      go((k_radix_scatter_staged2<TSV, 16, 512>), 512, 16, cus, lds, w32);
    else
      go((k_radix_scatter_staged2<TSV, 8, 512>), 512, 8, cus, lds, w32);
    return;
  }
  // One tile = blockDim * U events; enough blocks to fill the chip at
  // the REGISTER-bounded occupancy (98 VGPRs: two 512-thread
  // workgroups per CU, where the 40 KB staging LDS alone would allow
  // four), few enough to keep the end-of-kernel residual padding
  // small.  512-thread workgroups measured fastest (60.1 vs 56.6e9 at
  // 256, 57.2 at 1024 — see profiles/).
  size_t lds = (size_t)nseg * SC_GRAN * 8 + 4 * (size_t)nseg * sizeof(int);
  int threads = 512;
  if (env_threads == 256 || env_threads == 1024) threads = env_threads;
  if (threads == 512)
    go((k_radix_scatter_staged<AGG_COUNT, TSV, 16, 512>), 512, 16, 1024u,
       lds, NO_LATE_ARGS);
  else if (threads == 1024)
    go((k_radix_scatter_staged<AGG_COUNT, TSV, 16, 1024>), 1024, 16, 1024u,
       lds, NO_LATE_ARGS);
  else if (env_u == 8)
    go((k_radix_scatter_staged<AGG_COUNT, TSV, 8>), 256, 8, 1024u, lds,
       NO_LATE_ARGS);
  else if (env_u == 32)
    go((k_radix_scatter_staged<AGG_COUNT, TSV, 32>), 256, 32, 1024u, lds,
       NO_LATE_ARGS);
  else
    go((k_radix_scatter_staged<AGG_COUNT, TSV, 16>), 256, 16, 1024u, lds,
       NO_LATE_ARGS);
}

// The one place that picks and launches the COUNT segment aggregation
// (radix_window_insert, radix_agg_only and the native step loop).
// One workgroup per scatter segment; `seg_bits` is also the size of
// its LDS table.  The compact-cell kernel holds a count in 28 bits, so
// it is taken only when no segment can hold 2^28 entries.
static void launch_count_agg(
    hipStream_t stream, const uint64_t* evp, const int* gcur, int64_t cap,
    uint64_t* tkeys, unsigned long long* tvals, uint64_t mask,
    int region_bits, int seg_bits, int64_t nseg, int* err,
    int64_t entry_w, int entry_fmt) {
  // `entry_w`: CountEntries::agg_w() of the scatter call that filled
  // `evp`: its entry base when the entries are hashed or compact, else
  // ENTRY_W_CLASSIC.  `entry_fmt`: its CountEntries::fmt().
  const bool hashed = entry_w != ENTRY_W_CLASSIC;
  const uint32_t wlo = hashed ? (uint32_t)(uint64_t)entry_w : 0u;
  TORCH_CHECK(hashed == (entry_fmt != ENTRY_FMT_CLASSIC),
              "entry format and entry base disagree");
  if (entry_fmt == ENTRY_FMT_COMPACT) {
    TORCH_CHECK(count_agg_compact(cap, seg_bits) && nseg >= 128 &&
                    (nseg & (nseg - 1)) == 0,
                "compact entries need the compact-cell aggregation and a "
                "power-of-two segment count of at least 128");
    auto go = [&](auto kern, int threads) {
      hipLaunchKernelGGL(
          kern, dim3((unsigned)nseg), dim3((unsigned)threads),
          (size_t)8 << seg_bits, stream, (const uint32_t*)evp, gcur,
          cap & ~(int64_t)(SCC_GRAN - 1), tkeys, tvals, mask, region_bits,
          seg_bits, err, wlo, compact_dbits(nseg));
      HIP_CHECK(hipGetLastError());
    };
    int r = 2;
    if (const char* e = std::getenv("BYTEWAX_AGG_R")) r = atoi(e);
    if (seg_bits >= 12) {
      if (r == 1) go((k_radix_agg_compact<1024, 1>), 1024);
      else go((k_radix_agg_compact<1024, 2>), 1024);
    } else {
      go((k_radix_agg_compact<256, 2>), 256);
    }
    return;
  }
  if (count_agg_compact(cap, seg_bits)) {
    auto go = [&](auto kern, int threads) {
      hipLaunchKernelGGL(
          kern, dim3((unsigned)nseg), dim3((unsigned)threads),
          (size_t)8 << seg_bits, stream, evp, gcur, cap, tkeys, tvals, mask,
          region_bits, seg_bits, err, wlo);
      // A refused launch (LDS budget, bad configuration) must not pass
      // for an empty batch.
      HIP_CHECK(hipGetLastError());
    };
    // 1024 x 2: two workgroups per CU inside the 64-VGPR budget that
    // leaves; R = 4 needs scratch there (see profiles/).
    if (seg_bits >= 12) {
      if (hashed) go((k_radix_agg_count<1024, 2, true>), 1024);
      else go((k_radix_agg_count<1024, 2>), 1024);
    } else {
      if (hashed) go((k_radix_agg_count<256, 2, true>), 256);
      else go((k_radix_agg_count<256, 2>), 256);
    }
    return;
  }
  // Only the compact kernel reads hashed entries.
  TORCH_CHECK(!hashed, "hashed scatter entries need the compact aggregation");
  hipLaunchKernelGGL(
      k_radix_agg<AGG_COUNT>, dim3((unsigned)nseg),
      dim3(seg_bits >= 12 ? 1024u : 256u), (size_t)16 << seg_bits, stream,
      evp, (const int64_t*)nullptr, gcur, cap, tkeys, tvals, mask,
      region_bits, seg_bits, err);
  HIP_CHECK(hipGetLastError());
}

// k_overflow_agg is grid-stride: a block per CU drains a large spill
// (a batch whose windows do not fit the entry delta) with the whole
// chip and costs nothing when the spill is empty.
static dim3 overflow_agg_grid() { return dim3(device_cu_count()); }

// The optional running total of spilled events (int64 [1]).
static unsigned long long* spill_total_ptr(
    const c10::optional<torch::Tensor>& t) {
  if (!t.has_value()) return nullptr;
  check_dev(*t, torch::kInt64, "spill_total");
  TORCH_CHECK(t->numel() >= 1, "spill_total must hold one int64");
  return (unsigned long long*)t->data_ptr<int64_t>();
}

static void radix_window_insert_impl(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,   // int32 [n_regions]
    torch::Tensor ev_packed,  // int64 [n_regions * cap]
    torch::Tensor ev_vals,    // int64 [n_regions * cap] (sum mode)
    torch::Tensor ov_cursor,  // int32 [1]
    torch::Tensor ov_packed,  // int64 overflow spill
    torch::Tensor ov_vals,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms,  // sliding stride; 0 or == len_ms for tumbling
    std::vector<int64_t> seg_counts,
    std::vector<int64_t> seg_bases,
    const LateSink* late,
    c10::optional<torch::Tensor> spill_total = c10::nullopt,
    bool allow_compact = true) {
  if (off_ms <= 0) off_ms = len_ms;
  TORCH_CHECK(off_ms <= len_ms, "window offset must be <= length");
  check_dev(keys, torch::kInt32, "keys");
  // Segmented form: `ts` holds int32 deltas laid out as contiguous
  // per-source-rank segments (the RCCL all-to-allv wire format);
  // seg_counts[i] events use seg_bases[i] as their absolute base.
  // This inserts exchange output without ever materializing int64
  // timestamps (saves ~3 HBM passes over the biggest column).
  bool seg32 = !seg_counts.empty();
  bool ts32 = ts.scalar_type() == torch::kInt32;
  if (seg32) {
    TORCH_CHECK(seg_counts.size() == seg_bases.size(),
                "seg_counts/seg_bases length mismatch");
    check_dev(ts, torch::kInt32, "ts32");
  } else if (!ts32) {
    check_dev(ts, torch::kInt64, "ts");
  }
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(region_bits > 0, "radix path requires region_bits > 0");
  TORCH_CHECK(region_bits <= 12, "region_bits > 12 exceeds the LDS "
              "budget of the aggregation kernel (16 B/slot)");
  int64_t nb = nslots >> region_bits;
  TORCH_CHECK(nb >= 1 && nb <= 8192, "region count out of range");
  TORCH_CHECK(gcursors.numel() >= nb, "gcursors too small");
  const int64_t* vptr = nullptr;
  if (mode == AGG_SUM) {
    TORCH_CHECK(vals.has_value(), "sum mode requires vals");
    vptr = vals->data_ptr<int64_t>();
  }
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));

  ScatterKind kind = scatter_kind_env();
  // An event expands into ceil(len/off) windows when sliding; the
  // direct variant has no expansion loop.
  int64_t xf = off_ms < len_ms ? (len_ms + off_ms - 1) / off_ms : 1;
  TORCH_CHECK(xf <= 64, "sliding expansion > 64x; use a larger offset");
  if (kind == SCAT_DIRECT && xf > 1) kind = SCAT_FIXED;
  // Late tracking lives in the fixed and staged kernels only: the
  // direct variant routes to fixed, staged2 to staged.
  if (late != nullptr && kind == SCAT_DIRECT) kind = SCAT_FIXED;
  int coarse = scatter_coarse_bits(kind);
  int seg_bits = (int)region_bits + coarse;
  int64_t nseg = nslots >> seg_bits;
  // LDS budgets: staged scatter stages SC_GRAN packed (+vals) per
  // segment; the agg kernel stages 16 B per LDS slot.
  size_t staged_lds = (size_t)nseg * SC_GRAN * 8 *
                          (mode == AGG_SUM ? 2 : 1) +
                      4 * (size_t)nseg * sizeof(int);
  // The LATE staged scatter holds two more ints of (static) LDS; at
  // nseg == 2048 the COUNT staging alone fills the 160 KiB of a CU, so
  // late tracking takes the fixed layout there.
  const size_t late_lds = late != nullptr ? 2 * sizeof(int) : 0;
  while (kind == SCAT_STAGED &&
         (nseg < 1 || staged_lds + late_lds > 160 * 1024 ||
          seg_bits > 13)) {
    if (coarse > 0 && seg_bits > 13) {
      coarse -= 1;
    } else {
      kind = SCAT_FIXED;
      coarse = 0;
    }
    seg_bits = (int)region_bits + coarse;
    nseg = nslots >> seg_bits;
    staged_lds = (size_t)nseg * SC_GRAN * 8 * (mode == AGG_SUM ? 2 : 1) +
                 4 * (size_t)nseg * sizeof(int);
  }
  if (seg_bits > 13) {
    coarse = 0;
    seg_bits = (int)region_bits;
    nseg = nb;
  }
  int64_t cap = ev_packed.numel() / nseg;
  if (kind == SCAT_STAGED) {
    cap &= ~(int64_t)(SC_GRAN - 1);
    if (cap < SC_GRAN) {
      // Tiny buffers (small batches): granule rounding would zero the
      // per-segment capacity; the fixed variant has no granularity.
      kind = SCAT_FIXED;
      coarse = 0;
      seg_bits = (int)region_bits;
      nseg = nb;
      cap = ev_packed.numel() / nseg;
    }
  }
  TORCH_CHECK(cap * nseg >= 2 * n * xf || cap >= n * xf,
              "scatter buffers too small (need ~2x batch x expansion)");
  if (mode == AGG_SUM) {
    TORCH_CHECK(ev_vals.numel() >= nseg * cap, "ev_vals too small");
  }
  gcursors.narrow(0, 0, nseg).zero_();
  ov_cursor.zero_();
  size_t hist_lds = (size_t)nseg * sizeof(int);

  // Scatter grid: fewer blocks keep fewer segment cursors (and thus
  // partially-written cache lines) open at once — per-XCD L2 can then
  // accumulate full lines before eviction.  Tunable while we converge
  // on the best default (BYTEWAX_SCATTER_BLOCKS).
  int env_blocks = 0;
  if (const char* sb = std::getenv("BYTEWAX_SCATTER_BLOCKS")) {
    int v = atoi(sb);
    if (v > 0) env_blocks = v;
  }

  struct Seg {
    int64_t off, n, base;
  };
  std::vector<Seg> segs;
  if (seg32) {
    int64_t off = 0;
    for (size_t i = 0; i < seg_counts.size(); ++i) {
      if (seg_counts[i] > 0) segs.push_back({off, seg_counts[i], seg_bases[i]});
      off += seg_counts[i];
    }
    TORCH_CHECK(off == n, "segment counts must sum to batch length");
  } else {
    segs.push_back({0, n, ts_base});
  }

  uint64_t win_m2, win_maxfast;
  magic_div_u64(off_ms, &win_m2, &win_maxfast);
  const CountEntries ce = plan_count_entries(
      kind == SCAT_STAGED && mode == AGG_COUNT && late == nullptr, xf,
      ev_packed.data_ptr<int64_t>(), nseg, cap, seg_bits, seg32 || ts32,
      align_ms, len_ms, segs[0].base, allow_compact);
  unsigned scat_threads = 256;
  // `extra`: the trailing late-tracking arguments of the staged and
  // fixed kernels.
  auto scat = [&](auto kern, auto tsptr, const Seg& sg, unsigned gx,
                  size_t lds, auto... extra) {
    hipLaunchKernelGGL(
        kern, dim3(gx), dim3(scat_threads), lds, stream,
        keys.data_ptr<int32_t>() + sg.off, tsptr + sg.off,
        vptr != nullptr ? vptr + sg.off : nullptr, sg.n, align_ms, len_ms,
        off_ms, sg.base, mask, seg_bits, cap, gcursors.data_ptr<int32_t>(),
        (uint64_t*)ev_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ev_vals.data_ptr<int64_t>() : nullptr,
        ov_cursor.data_ptr<int32_t>(),
        (uint64_t*)ov_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ov_vals.data_ptr<int64_t>() : nullptr,
        ov_packed.numel(),
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), win_m2, win_maxfast, extra...);
    // A refused launch (LDS budget, bad configuration) must not pass
    // for an empty batch.
    HIP_CHECK(hipGetLastError());
  };
  // Late-tracking launches: one configuration per mode (the defaults
  // of the plain path: 512x16 tiles for COUNT, 256x16 for SUM), no
  // env-tuned U/BLK matrix.
  auto scat_late = [&](auto tsptr, const Seg& sg) {
    using TSV = std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
    if (kind == SCAT_STAGED) {
      int sthreads = mode == AGG_COUNT ? 512 : 256;
      scat_threads = (unsigned)sthreads;
      unsigned gs =
          (unsigned)((sg.n * xf + sthreads * 16 - 1) / (sthreads * 16));
      if (gs > 1024u) gs = 1024u;
      if (gs < 1) gs = 1;
      if (mode == AGG_COUNT)
        scat((k_radix_scatter_staged<AGG_COUNT, TSV, 16, 512, true>), tsptr,
             sg, gs, staged_lds, late->cutoff, late->keys, late->ts,
             late->vals, late->n, late->cap);
      else
        scat((k_radix_scatter_staged<AGG_SUM, TSV, 16, 256, true>), tsptr,
             sg, gs, staged_lds, late->cutoff, late->keys, late->ts,
             late->vals, late->n, late->cap);
    } else {
      scat_threads = 256;
      unsigned gx = (unsigned)n_blocks(sg.n, 256);
      if (mode == AGG_COUNT)
        scat((k_radix_scatter_fixed<AGG_COUNT, TSV, true>), tsptr, sg, gx,
             2 * hist_lds, late->cutoff, late->keys, late->ts, late->vals,
             late->n, late->cap);
      else
        scat((k_radix_scatter_fixed<AGG_SUM, TSV, true>), tsptr, sg, gx,
             2 * hist_lds, late->cutoff, late->keys, late->ts, late->vals,
             late->n, late->cap);
    }
  };
  auto scat_any = [&](auto tsptr, const Seg& sg) {
    using TSV = std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
    if (late != nullptr) {
      scat_late(tsptr, sg);
      return;
    }
    unsigned gx = (unsigned)n_blocks(sg.n, 256);
    if (env_blocks > 0 && (unsigned)env_blocks < gx) gx = (unsigned)env_blocks;
    if (kind == SCAT_STAGED) {
      if (mode == AGG_COUNT) {
        launch_count_staged<TSV>(
            stream, keys.data_ptr<int32_t>() + sg.off, tsptr + sg.off, sg.n,
            xf, align_ms, len_ms, off_ms, sg.base, mask, seg_bits, nseg, cap,
            gcursors.data_ptr<int32_t>(),
            (uint64_t*)ev_packed.data_ptr<int64_t>(),
            ov_cursor.data_ptr<int32_t>(),
            (uint64_t*)ov_packed.data_ptr<int64_t>(), ov_packed.numel(),
            (unsigned long long*)max_ts.data_ptr<int64_t>(),
            error_flag.data_ptr<int32_t>(), win_m2, win_maxfast,
            /*overlapped=*/false, ce);
      } else {
        unsigned cap_gs = env_blocks > 0 ? (unsigned)env_blocks : 1024u;
        unsigned gs = (unsigned)((sg.n * xf + 256 * 16 - 1) / (256 * 16));
        if (gs > cap_gs) gs = cap_gs;
        if (gs < 1) gs = 1;
        scat_threads = 256;
        scat(k_radix_scatter_staged<AGG_SUM, TSV>, tsptr, sg, gs,
             staged_lds, NO_LATE_ARGS);
      }
    } else if (kind == SCAT_DIRECT) {
      scat_threads = 256;
      if (mode == AGG_COUNT)
        scat(k_radix_scatter_direct<AGG_COUNT, TSV>, tsptr, sg, gx, 0);
      else
        scat(k_radix_scatter_direct<AGG_SUM, TSV>, tsptr, sg, gx, 0);
    } else {
      scat_threads = 256;
      if (mode == AGG_COUNT)
        scat(k_radix_scatter_fixed<AGG_COUNT, TSV>, tsptr, sg, gx,
             2 * hist_lds, NO_LATE_ARGS);
      else
        scat(k_radix_scatter_fixed<AGG_SUM, TSV>, tsptr, sg, gx,
             2 * hist_lds, NO_LATE_ARGS);
    }
  };
  for (const Seg& sg : segs) {
    if (seg32 || ts32) scat_any(ts.data_ptr<int32_t>(), sg);
    else scat_any(ts.data_ptr<int64_t>(), sg);
  }

  // Segment b's events live at [b*cap, b*cap + count).
  size_t agg_lds = (size_t)16 << seg_bits;
  dim3 agg_block(seg_bits >= 12 ? 1024 : 256);
  auto agg = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, dim3((unsigned)nseg), agg_block, agg_lds, stream,
        (const uint64_t*)ev_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ev_vals.data_ptr<int64_t>() : nullptr,
        gcursors.data_ptr<int32_t>(), cap,
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
        (int)region_bits, seg_bits, error_flag.data_ptr<int32_t>());
  };
  if (mode == AGG_COUNT) {
    launch_count_agg(
        stream, (const uint64_t*)ev_packed.data_ptr<int64_t>(),
        gcursors.data_ptr<int32_t>(), cap,
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
        (int)region_bits, seg_bits, nseg, error_flag.data_ptr<int32_t>(),
        ce.agg_w(), ce.fmt());
  } else {
    agg(k_radix_agg<AGG_SUM>);
  }

  auto ov = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, overflow_agg_grid(), dim3(256), 0, stream,
        (const uint64_t*)ov_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ov_vals.data_ptr<int64_t>() : nullptr,
        ov_cursor.data_ptr<int32_t>(), ov_packed.numel(),
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
        (int)region_bits, error_flag.data_ptr<int32_t>(),
        spill_total_ptr(spill_total));
  };
  if (mode == AGG_COUNT) ov(k_overflow_agg<AGG_COUNT>);
  else ov(k_overflow_agg<AGG_SUM>);
}

void radix_window_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms = 0,  // sliding stride; 0 or == len_ms for tumbling
    std::vector<int64_t> seg_counts = {},
    std::vector<int64_t> seg_bases = {},
    // Running total of spilled events (int64 [1]), and whether compact
    // entries may be planned (a demoted state says no).
    c10::optional<torch::Tensor> spill_total = c10::nullopt,
    bool compact = true) {
  radix_window_insert_impl(
      keys, ts, vals, tkeys, tvals, max_ts, error_flag, gcursors, ev_packed,
      ev_vals, ov_cursor, ov_packed, ov_vals, align_ms, len_ms, mode, ts_base,
      region_bits, off_ms, std::move(seg_counts), std::move(seg_bases),
      nullptr, std::move(spill_total), compact);
}

// Late-tracking form of radix_window_insert (unsegmented batches
// only; see window_agg_insert_late for the late arguments).
void radix_window_insert_late(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms,
    int64_t late_cutoff,
    torch::Tensor late_keys,
    torch::Tensor late_ts,
    c10::optional<torch::Tensor> late_vals,
    torch::Tensor late_n) {
  LateSink sink = make_late_sink(late_cutoff, late_keys, late_ts, late_vals,
                                 late_n, mode == AGG_SUM);
  radix_window_insert_impl(
      keys, ts, vals, tkeys, tvals, max_ts, error_flag, gcursors, ev_packed,
      ev_vals, ov_cursor, ov_packed, ov_vals, align_ms, len_ms, mode, ts_base,
      region_bits, off_ms, {}, {}, &sink);
}

// Split radix insert for the per-step Python engine's pipelined
// path: `radix_scatter_only` launches the (memset + per-segment
// scatter) on the CURRENT stream — the caller runs it under a side
// torch.cuda.Stream — and `radix_agg_only` drains a buffer set into
// the table on whatever stream is current.  Stream/event
// orchestration (scatter N+1 overlapping agg N, buffer-parity reuse
// fences, NCCL completion ordering) lives in Python with torch
// events, which keeps it per-state and lets the exchange wait be
// recorded on the side stream only.
// Returns what radix_agg_only must be told about the entries: the
// call's entry base when they are hashed, else ENTRY_W_CLASSIC.  With
// `compact` the call may write compact entries and returns the pair
// (entry base, ENTRY_FMT_*) instead, both for radix_agg_only; without
// it the entries are never compact and the base alone says which of
// the other two formats they have.
pybind11::object radix_scatter_only(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t nslots,
    int64_t align_ms,
    int64_t len_ms,
    int64_t mode,
    int64_t ts_base,
    int64_t region_bits,
    int64_t off_ms,
    std::vector<int64_t> seg_counts,
    std::vector<int64_t> seg_bases,
    bool compact = false) {
  auto result = [&](const CountEntries& ce) -> pybind11::object {
    if (!compact) return pybind11::int_(ce.agg_w());
    return pybind11::make_tuple(ce.agg_w(), ce.fmt());
  };
  if (off_ms <= 0) off_ms = len_ms;
  TORCH_CHECK(off_ms <= len_ms, "window offset must be <= length");
  check_dev(keys, torch::kInt32, "keys");
  bool seg32 = !seg_counts.empty();
  bool ts32 = ts.scalar_type() == torch::kInt32;
  if (seg32) {
    TORCH_CHECK(seg_counts.size() == seg_bases.size(),
                "seg_counts/seg_bases length mismatch");
    check_dev(ts, torch::kInt32, "ts32");
  } else if (!ts32) {
    check_dev(ts, torch::kInt64, "ts");
  }
  int64_t n = keys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  int64_t nb = nslots >> region_bits;
  const int64_t* vptr = nullptr;
  if (mode == AGG_SUM) {
    TORCH_CHECK(vals.has_value(), "sum mode requires vals");
    vptr = vals->data_ptr<int64_t>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  dim3 block(256);
  uint64_t win_m2, win_maxfast;
  magic_div_u64(off_ms <= 0 ? len_ms : off_ms, &win_m2, &win_maxfast);

  // Same variant/segmentation decision as radix_agg_only (both read
  // the env once per call; one process = one configuration).
  ScatterKind kind = scatter_kind_env();
  int64_t xf = off_ms < len_ms ? (len_ms + off_ms - 1) / off_ms : 1;
  TORCH_CHECK(xf <= 64, "sliding expansion > 64x; use a larger offset");
  if (kind == SCAT_DIRECT && xf > 1) kind = SCAT_FIXED;
  int coarse = scatter_coarse_bits(kind);
  int seg_bits = (int)region_bits + coarse;
  int64_t nseg = nslots >> seg_bits;
  size_t staged_lds = (size_t)nseg * SC_GRAN * 8 *
                          (mode == AGG_SUM ? 2 : 1) +
                      4 * (size_t)nseg * sizeof(int);
  while (kind == SCAT_STAGED &&
         (nseg < 1 || staged_lds > 160 * 1024 || seg_bits > 13)) {
    if (coarse > 0 && seg_bits > 13) {
      coarse -= 1;
    } else {
      kind = SCAT_FIXED;
      coarse = 0;
    }
    seg_bits = (int)region_bits + coarse;
    nseg = nslots >> seg_bits;
    staged_lds = (size_t)nseg * SC_GRAN * 8 * (mode == AGG_SUM ? 2 : 1) +
                 4 * (size_t)nseg * sizeof(int);
  }
  if (seg_bits > 13) {
    coarse = 0;
    seg_bits = (int)region_bits;
    nseg = nb;
  }
  int64_t cap = ev_packed.numel() / nseg;
  if (kind == SCAT_STAGED) {
    cap &= ~(int64_t)(SC_GRAN - 1);
    if (cap < SC_GRAN) {
      kind = SCAT_FIXED;
      coarse = 0;
      seg_bits = (int)region_bits;
      nseg = nb;
      cap = ev_packed.numel() / nseg;
    }
  }
  TORCH_CHECK(cap * nseg >= 2 * n * xf || cap >= n * xf,
              "scatter buffers too small");
  size_t hist_lds = (size_t)nseg * sizeof(int);
  HIP_CHECK(hipMemsetAsync(
      gcursors.data_ptr<int32_t>(), 0, (size_t)nseg * sizeof(int), stream));
  HIP_CHECK(hipMemsetAsync(
      ov_cursor.data_ptr<int32_t>(), 0, sizeof(int), stream));
  if (n == 0) return result(CountEntries{});

  struct Seg {
    int64_t off, n, base;
  };
  std::vector<Seg> segs;
  if (seg32) {
    int64_t off = 0;
    for (size_t i = 0; i < seg_counts.size(); ++i) {
      if (seg_counts[i] > 0) segs.push_back({off, seg_counts[i], seg_bases[i]});
      off += seg_counts[i];
    }
  } else {
    segs.push_back({0, n, ts_base});
  }
  if (segs.empty()) return result(CountEntries{});
  const CountEntries ce = plan_count_entries(
      kind == SCAT_STAGED && mode == AGG_COUNT, xf,
      ev_packed.data_ptr<int64_t>(), nseg, cap, seg_bits, seg32 || ts32,
      align_ms, len_ms, segs[0].base, compact);
  unsigned scat_threads = 256;
  // `extra`: the trailing late-tracking arguments of the staged and
  // fixed kernels (always off on this path).
  auto scat = [&](auto kern, auto tsptr, const Seg& sg, unsigned gx,
                  size_t lds, auto... extra) {
    hipLaunchKernelGGL(
        kern, dim3(gx), dim3(scat_threads), lds,
        stream, keys.data_ptr<int32_t>() + sg.off, tsptr + sg.off,
        vptr != nullptr ? vptr + sg.off : nullptr, sg.n, align_ms, len_ms,
        off_ms, sg.base, mask, seg_bits, cap, gcursors.data_ptr<int32_t>(),
        (uint64_t*)ev_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ev_vals.data_ptr<int64_t>() : nullptr,
        ov_cursor.data_ptr<int32_t>(),
        (uint64_t*)ov_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ov_vals.data_ptr<int64_t>() : nullptr,
        ov_packed.numel(),
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), win_m2, win_maxfast, extra...);
  };
  auto scat_any = [&](auto tsptr, const Seg& sg) {
    using TSV = std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
    if (kind == SCAT_STAGED) {
      if (mode == AGG_COUNT) {
        launch_count_staged<TSV>(
            stream, keys.data_ptr<int32_t>() + sg.off, tsptr + sg.off, sg.n,
            xf, align_ms, len_ms, off_ms, sg.base, mask, seg_bits, nseg, cap,
            gcursors.data_ptr<int32_t>(),
            (uint64_t*)ev_packed.data_ptr<int64_t>(),
            ov_cursor.data_ptr<int32_t>(),
            (uint64_t*)ov_packed.data_ptr<int64_t>(), ov_packed.numel(),
            (unsigned long long*)max_ts.data_ptr<int64_t>(),
            error_flag.data_ptr<int32_t>(), win_m2, win_maxfast,
            /*overlapped=*/true, ce);
      } else {
        unsigned gs = (unsigned)((sg.n + 4095) / 4096);
        if (gs > 1024) gs = 1024;
        if (gs < 1) gs = 1;
        scat(k_radix_scatter_staged<AGG_SUM, TSV>, tsptr, sg, gs,
             staged_lds, NO_LATE_ARGS);
      }
    } else if (kind == SCAT_DIRECT) {
      unsigned gx = (unsigned)n_blocks(sg.n, 256);
      if (mode == AGG_COUNT)
        scat(k_radix_scatter_direct<AGG_COUNT, TSV>, tsptr, sg, gx, 0);
      else
        scat(k_radix_scatter_direct<AGG_SUM, TSV>, tsptr, sg, gx, 0);
    } else {
      unsigned gx = (unsigned)n_blocks(sg.n, 256);
      if (mode == AGG_COUNT)
        scat(k_radix_scatter_fixed<AGG_COUNT, TSV>, tsptr, sg, gx,
             2 * hist_lds, NO_LATE_ARGS);
      else
        scat(k_radix_scatter_fixed<AGG_SUM, TSV>, tsptr, sg, gx,
             2 * hist_lds, NO_LATE_ARGS);
    }
  };
  for (const Seg& sg : segs) {
    if (seg32 || ts32) scat_any(ts.data_ptr<int32_t>(), sg);
    else scat_any(ts.data_ptr<int64_t>(), sg);
  }
  return result(ce);
}

// `entry_w`, `entry_fmt`: what the radix_scatter_only call that filled
// these buffers returned.  Without `entry_fmt` the base alone tells
// classic from hashed entries.
void radix_agg_only(
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t mode,
    int64_t region_bits,
    int64_t entry_w = ENTRY_W_CLASSIC,
    int64_t entry_fmt = -1,
    c10::optional<torch::Tensor> spill_total = c10::nullopt) {
  if (mode != AGG_COUNT) entry_w = ENTRY_W_CLASSIC;
  if (entry_fmt < 0 || mode != AGG_COUNT)
    entry_fmt =
        entry_w != ENTRY_W_CLASSIC ? ENTRY_FMT_HASHED : ENTRY_FMT_CLASSIC;
  int64_t nslots = tkeys.numel();
  int64_t nb = nslots >> region_bits;
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  // Mirror radix_scatter_only's segmentation decision.
  ScatterKind kind = scatter_kind_env();
  int coarse = scatter_coarse_bits(kind);
  int seg_bits = (int)region_bits + coarse;
  int64_t nseg = nslots >> seg_bits;
  size_t staged_lds = (size_t)nseg * SC_GRAN * 8 *
                          (mode == AGG_SUM ? 2 : 1) +
                      4 * (size_t)nseg * sizeof(int);
  while (kind == SCAT_STAGED &&
         (nseg < 1 || staged_lds > 160 * 1024 || seg_bits > 13)) {
    if (coarse > 0 && seg_bits > 13) {
      coarse -= 1;
    } else {
      kind = SCAT_FIXED;
      coarse = 0;
    }
    seg_bits = (int)region_bits + coarse;
    nseg = nslots >> seg_bits;
    staged_lds = (size_t)nseg * SC_GRAN * 8 * (mode == AGG_SUM ? 2 : 1) +
                 4 * (size_t)nseg * sizeof(int);
  }
  if (seg_bits > 13) {
    seg_bits = (int)region_bits;
    nseg = nb;
  }
  int64_t cap = ev_packed.numel() / nseg;
  if (kind == SCAT_STAGED) {
    cap &= ~(int64_t)(SC_GRAN - 1);
    if (cap < SC_GRAN) {
      kind = SCAT_FIXED;
      seg_bits = (int)region_bits;
      nseg = nb;
      cap = ev_packed.numel() / nseg;
    }
  }
  size_t agg_lds = (size_t)16 << seg_bits;
  dim3 agg_block(seg_bits >= 12 ? 1024 : 256);
  auto agg = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, dim3((unsigned)nseg), agg_block, agg_lds, stream,
        (const uint64_t*)ev_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ev_vals.data_ptr<int64_t>() : nullptr,
        gcursors.data_ptr<int32_t>(), cap,
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
        (int)region_bits, seg_bits, error_flag.data_ptr<int32_t>());
  };
  if (mode == AGG_COUNT) {
    launch_count_agg(
        stream, (const uint64_t*)ev_packed.data_ptr<int64_t>(),
        gcursors.data_ptr<int32_t>(), cap,
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
        (int)region_bits, seg_bits, nseg, error_flag.data_ptr<int32_t>(),
        entry_w, (int)entry_fmt);
  } else {
    agg(k_radix_agg<AGG_SUM>);
  }
  auto ov = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, overflow_agg_grid(), dim3(256), 0, stream,
        (const uint64_t*)ov_packed.data_ptr<int64_t>(),
        mode == AGG_SUM ? ov_vals.data_ptr<int64_t>() : nullptr,
        ov_cursor.data_ptr<int32_t>(), ov_packed.numel(),
        (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
        (int)region_bits, error_flag.data_ptr<int32_t>(),
        spill_total_ptr(spill_total));
  };
  if (mode == AGG_COUNT) ov(k_overflow_agg<AGG_COUNT>);
  else ov(k_overflow_agg<AGG_SUM>);
}

void radix_v2_window_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcur,    // int32 [V2_COARSE]
    torch::Tensor gres,    // int32 [V2_COARSE]
    torch::Tensor ev,      // int64 [V2_COARSE * cap_c]
    torch::Tensor ev_res,  // int64 [V2_COARSE * res_cap]
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int64_t region_bits) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(ts, torch::kInt64, "ts");
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  int64_t cap_c = ev.numel() / V2_COARSE;
  TORCH_CHECK(cap_c % 8 == 0, "coarse capacity must be 8-aligned");
  int64_t res_cap = ev_res.numel() / V2_COARSE;
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  gcur.zero_();
  gres.zero_();
  hipLaunchKernelGGL(
      k_scatter_coarse, dim3(256), dim3(512), 0, stream,
      keys.data_ptr<int32_t>(), ts.data_ptr<int64_t>(), n, align_ms,
      len_ms, ts_base, mask, (int)region_bits, cap_c, res_cap,
      gcur.data_ptr<int32_t>(), gres.data_ptr<int32_t>(),
      (uint64_t*)ev.data_ptr<int64_t>(),
      (uint64_t*)ev_res.data_ptr<int64_t>(),
      (unsigned long long*)max_ts.data_ptr<int64_t>(),
      error_flag.data_ptr<int32_t>());
  int slices = 8;
  hipLaunchKernelGGL(
      k_agg_cached, dim3(V2_COARSE * slices), dim3(256), 0, stream,
      (const uint64_t*)ev.data_ptr<int64_t>(),
      (const uint64_t*)ev_res.data_ptr<int64_t>(),
      gcur.data_ptr<int32_t>(), gres.data_ptr<int32_t>(), cap_c, res_cap,
      slices, (uint64_t*)tkeys.data_ptr<int64_t>(),
      (unsigned long long*)tvals.data_ptr<int64_t>(), mask,
      (int)region_bits, error_flag.data_ptr<int32_t>());
}

// One launch shape for every close that reclaims (see k_close_migrate).
static void launch_close_migrate(
    hipStream_t stream, const torch::Tensor& tkeys,
    const torch::Tensor& tvals, int64_t win_hi, const torch::Tensor& nkeys,
    const torch::Tensor& nvals, int64_t region_bits,
    const torch::Tensor& out_keys, const torch::Tensor& out_wins,
    const torch::Tensor& out_vals, const torch::Tensor& out_n,
    const torch::Tensor& error_flag) {
  int64_t nslots = tkeys.numel();
  int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  if (nchunks < 1) nchunks = 1;
  unsigned grid = (unsigned)(nchunks < CM_MAX_GRID ? nchunks : CM_MAX_GRID);
  hipLaunchKernelGGL(
      k_close_migrate, dim3(grid), dim3(CM_BLK), 0, stream,
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const unsigned long long*)tvals.data_ptr<int64_t>(), nslots, win_hi,
      (uint64_t*)nkeys.data_ptr<int64_t>(),
      (unsigned long long*)nvals.data_ptr<int64_t>(),
      (uint64_t)(nslots - 1), (int)region_bits,
      out_keys.data_ptr<int32_t>(), out_wins.data_ptr<int32_t>(),
      out_vals.data_ptr<int64_t>(), out_n.data_ptr<int32_t>(),
      out_keys.numel(), error_flag.data_ptr<int32_t>());
}

int64_t close_extract(
    torch::Tensor tkeys,
    torch::Tensor tvals,
    int64_t win_lo,
    int64_t win_hi,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_vals,
    torch::Tensor out_n) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(tvals, torch::kInt64, "tvals");
  check_dev(out_keys, torch::kInt32, "out_keys");
  check_dev(out_wins, torch::kInt32, "out_wins");
  check_dev(out_vals, torch::kInt64, "out_vals");
  check_dev(out_n, torch::kInt32, "out_n");
  int64_t nslots = tkeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(nslots, 256));
  hipLaunchKernelGGL(
      k_close_extract, grid, block, 0, stream,
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const unsigned long long*)tvals.data_ptr<int64_t>(), nslots, win_lo,
      win_hi, out_keys.data_ptr<int32_t>(),
      out_wins.data_ptr<int32_t>(), out_vals.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), out_keys.numel());
  return 0;
}

void close_migrate(
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor nkeys,
    torch::Tensor nvals,
    int64_t win_hi,
    int64_t region_bits,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    torch::Tensor error_flag) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(nkeys, torch::kInt64, "nkeys");
  check_dev(tvals, torch::kInt64, "tvals");
  check_dev(nvals, torch::kInt64, "nvals");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nkeys.numel() == nslots, "table size mismatch");
  launch_close_migrate(
      at::hip::getCurrentHIPStream(), tkeys, tvals, win_hi, nkeys, nvals,
      region_bits, out_keys, out_wins, out_vals, out_n, error_flag);
}

static void stats_insert_impl(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    const LateSink* late) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(ts, torch::kInt64, "ts");
  check_dev(vals, torch::kInt64, "vals");
  check_dev(tkeys, torch::kInt64, "tkeys");
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  auto launch = [&](auto kern, auto... extra) {
    hipLaunchKernelGGL(
        kern, grid, block, 0, stream, keys.data_ptr<int32_t>(),
        ts.data_ptr<int64_t>(), vals.data_ptr<int64_t>(),
        n, (uint64_t*)tkeys.data_ptr<int64_t>(),
        (long long*)tcnt.data_ptr<int64_t>(),
        (long long*)tsum.data_ptr<int64_t>(),
        (long long*)tmin.data_ptr<int64_t>(),
        (long long*)tmax.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
        align_ms, len_ms, ts_base,
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), extra...);
  };
  if (late != nullptr)
    launch(k_stats_insert<true>, late->cutoff, late->keys, late->ts,
           late->vals, late->n, late->cap);
  else
    launch(k_stats_insert<false>, NO_LATE_ARGS);
}

void stats_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base) {
  stats_insert_impl(keys, ts, vals, tkeys, tcnt, tsum, tmin, tmax, max_ts,
                    error_flag, align_ms, len_ms, ts_base, nullptr);
}

// Late-tracking form of stats_insert (see window_agg_insert_late).
void stats_insert_late(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int64_t late_cutoff,
    torch::Tensor late_keys,
    torch::Tensor late_ts,
    torch::Tensor late_vals,
    torch::Tensor late_n) {
  c10::optional<torch::Tensor> lv(late_vals);
  LateSink sink =
      make_late_sink(late_cutoff, late_keys, late_ts, lv, late_n, true);
  stats_insert_impl(keys, ts, vals, tkeys, tcnt, tsum, tmin, tmax, max_ts,
                    error_flag, align_ms, len_ms, ts_base, &sink);
}

static void radix_stats_insert_impl(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int64_t region_bits,
    const LateSink* late) {
  check_dev(keys, torch::kInt32, "keys");
  bool ts32 = ts.scalar_type() == torch::kInt32;
  if (!ts32) check_dev(ts, torch::kInt64, "ts");
  check_dev(vals, torch::kInt64, "vals");
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(region_bits > 0 && region_bits <= 10,
              "stats radix needs 0 < region_bits <= 10 (40 B/slot LDS)");
  int64_t nb = nslots >> region_bits;
  TORCH_CHECK(nb >= 1 && nb <= 8192, "region count out of range");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));

  // Same scatter-variant decision as the window path; the stats agg
  // stages 40 B/LDS slot, capping coarse segments at lds_bits 11.
  ScatterKind kind = scatter_kind_env();
  // Late tracking lives in the fixed and staged kernels only.
  if (late != nullptr && kind == SCAT_DIRECT) kind = SCAT_FIXED;
  int coarse = scatter_coarse_bits(kind);
  int seg_bits = (int)region_bits + coarse;
  int64_t nseg = nslots >> seg_bits;
  size_t staged_lds = (size_t)nseg * SC_GRAN * 8 * 2 +
                      4 * (size_t)nseg * sizeof(int);
  // Two more ints of static LDS in the LATE staged scatter.
  const size_t late_lds = late != nullptr ? 2 * sizeof(int) : 0;
  while (kind == SCAT_STAGED &&
         (nseg < 1 || staged_lds + late_lds > 160 * 1024 ||
          seg_bits > 11)) {
    if (coarse > 0 && seg_bits > 11) {
      coarse -= 1;
    } else {
      kind = SCAT_FIXED;
      coarse = 0;
    }
    seg_bits = (int)region_bits + coarse;
    nseg = nslots >> seg_bits;
    staged_lds = (size_t)nseg * SC_GRAN * 8 * 2 +
                 4 * (size_t)nseg * sizeof(int);
  }
  if (seg_bits > 11) {
    coarse = 0;
    seg_bits = (int)region_bits;
    nseg = nb;
  }
  int64_t cap = ev_packed.numel() / nseg;
  if (kind == SCAT_STAGED) {
    cap &= ~(int64_t)(SC_GRAN - 1);
    if (cap < SC_GRAN) {
      kind = SCAT_FIXED;
      coarse = 0;
      seg_bits = (int)region_bits;
      nseg = nb;
      cap = ev_packed.numel() / nseg;
    }
  }
  TORCH_CHECK(cap * nseg >= 2 * n || cap >= n,
              "scatter buffers too small (need ~2x batch)");
  TORCH_CHECK(ev_vals.numel() >= nseg * cap, "ev_vals too small");
  gcursors.narrow(0, 0, nseg).zero_();
  ov_cursor.zero_();
  size_t hist_lds = (size_t)nseg * sizeof(int);
  uint64_t win_m2, win_maxfast;
  magic_div_u64(len_ms, &win_m2, &win_maxfast);
  auto scat_any = [&](auto tsptr) {
    using TSV = std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
    if (kind == SCAT_STAGED) {
      unsigned gs = (unsigned)((n + 8191) / 8192);
      if (gs > 1024) gs = 1024;
      if (gs < 1) gs = 1;
      auto staged = [&](auto kern, auto... extra) {
      hipLaunchKernelGGL(
          kern, dim3(gs),
          dim3(512), staged_lds,
          stream, keys.data_ptr<int32_t>(), tsptr,
          vals.data_ptr<int64_t>(), n, align_ms, len_ms, len_ms, ts_base,
          mask,
          seg_bits, cap, gcursors.data_ptr<int32_t>(),
          (uint64_t*)ev_packed.data_ptr<int64_t>(),
          ev_vals.data_ptr<int64_t>(), ov_cursor.data_ptr<int32_t>(),
          (uint64_t*)ov_packed.data_ptr<int64_t>(),
          ov_vals.data_ptr<int64_t>(), ov_packed.numel(),
          (unsigned long long*)max_ts.data_ptr<int64_t>(),
          error_flag.data_ptr<int32_t>(), win_m2, win_maxfast, extra...);
      };
      if (late != nullptr)
        staged((k_radix_scatter_staged<AGG_SUM, TSV, 16, 512, true>),
               late->cutoff, late->keys, late->ts, late->vals, late->n,
               late->cap);
      else
        staged((k_radix_scatter_staged<AGG_SUM, TSV, 16, 512>),
               NO_LATE_ARGS);
    } else {
      auto fixed = [&](auto kern, auto... extra) {
      hipLaunchKernelGGL(
          kern, grid, block,
          2 * hist_lds, stream,
          keys.data_ptr<int32_t>(), tsptr,
          vals.data_ptr<int64_t>(), n, align_ms, len_ms, len_ms, ts_base,
          mask,
          seg_bits, cap, gcursors.data_ptr<int32_t>(),
          (uint64_t*)ev_packed.data_ptr<int64_t>(), ev_vals.data_ptr<int64_t>(),
          ov_cursor.data_ptr<int32_t>(),
          (uint64_t*)ov_packed.data_ptr<int64_t>(), ov_vals.data_ptr<int64_t>(),
          ov_packed.numel(),
          (unsigned long long*)max_ts.data_ptr<int64_t>(),
          error_flag.data_ptr<int32_t>(), win_m2, win_maxfast, extra...);
      };
      if (late != nullptr)
        fixed((k_radix_scatter_fixed<AGG_SUM, TSV, true>), late->cutoff,
              late->keys, late->ts, late->vals, late->n, late->cap);
      else
        fixed((k_radix_scatter_fixed<AGG_SUM, TSV>), NO_LATE_ARGS);
    }
  };
  if (ts32) scat_any(ts.data_ptr<int32_t>());
  else scat_any(ts.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());

  auto offsets = at::arange(
      nseg, at::TensorOptions().dtype(at::kInt).device(keys.device()));
  offsets = offsets * (int)cap;
  size_t agg_lds = (size_t)40 << seg_bits;
  dim3 agg_block(seg_bits >= 11 ? 1024 : 256);
  hipLaunchKernelGGL(
      k_radix_agg_stats, dim3((unsigned)nseg), agg_block, agg_lds, stream,
      (const uint64_t*)ev_packed.data_ptr<int64_t>(),
      ev_vals.data_ptr<int64_t>(), offsets.data_ptr<int32_t>(),
      gcursors.data_ptr<int32_t>(), (uint64_t*)tkeys.data_ptr<int64_t>(),
      (long long*)tcnt.data_ptr<int64_t>(),
      (long long*)tsum.data_ptr<int64_t>(),
      (long long*)tmin.data_ptr<int64_t>(),
      (long long*)tmax.data_ptr<int64_t>(), cap, mask, (int)region_bits,
      seg_bits, error_flag.data_ptr<int32_t>());

  hipLaunchKernelGGL(
      k_overflow_agg_stats, dim3(64), block, 0, stream,
      (const uint64_t*)ov_packed.data_ptr<int64_t>(),
      ov_vals.data_ptr<int64_t>(), ov_cursor.data_ptr<int32_t>(),
      ov_packed.numel(), (uint64_t*)tkeys.data_ptr<int64_t>(),
      (long long*)tcnt.data_ptr<int64_t>(),
      (long long*)tsum.data_ptr<int64_t>(),
      (long long*)tmin.data_ptr<int64_t>(),
      (long long*)tmax.data_ptr<int64_t>(), mask,
      error_flag.data_ptr<int32_t>());
}

void radix_stats_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int64_t region_bits) {
  radix_stats_insert_impl(
      keys, ts, vals, tkeys, tcnt, tsum, tmin, tmax, max_ts, error_flag,
      gcursors, ev_packed, ev_vals, ov_cursor, ov_packed, ov_vals, align_ms,
      len_ms, ts_base, region_bits, nullptr);
}

// Late-tracking form of radix_stats_insert (see window_agg_insert_late).
void radix_stats_insert_late(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    int64_t region_bits,
    int64_t late_cutoff,
    torch::Tensor late_keys,
    torch::Tensor late_ts,
    torch::Tensor late_vals,
    torch::Tensor late_n) {
  c10::optional<torch::Tensor> lv(late_vals);
  LateSink sink =
      make_late_sink(late_cutoff, late_keys, late_ts, lv, late_n, true);
  radix_stats_insert_impl(
      keys, ts, vals, tkeys, tcnt, tsum, tmin, tmax, max_ts, error_flag,
      gcursors, ev_packed, ev_vals, ov_cursor, ov_packed, ov_vals, align_ms,
      len_ms, ts_base, region_bits, &sink);
}

void stats_fixup(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor cnt_delta,
    torch::Tensor sum_delta,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    int64_t align_ms,
    int64_t len_ms) {
  int64_t n = keys.numel();
  if (n == 0) return;
  int64_t nslots = tkeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  hipLaunchKernelGGL(
      k_stats_fixup, grid, block, 0, stream, keys.data_ptr<int32_t>(),
      ts.data_ptr<int64_t>(), cnt_delta.data_ptr<int64_t>(),
      sum_delta.data_ptr<int64_t>(), n,
      (uint64_t*)tkeys.data_ptr<int64_t>(),
      (long long*)tcnt.data_ptr<int64_t>(),
      (long long*)tsum.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
      align_ms, len_ms);
}

void stats_extract(
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    int64_t win_lo,
    int64_t win_hi,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_cnt,
    torch::Tensor out_sum,
    torch::Tensor out_min,
    torch::Tensor out_max,
    torch::Tensor out_n) {
  int64_t nslots = tkeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(nslots, 256));
  hipLaunchKernelGGL(
      k_stats_extract, grid, block, 0, stream,
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const long long*)tcnt.data_ptr<int64_t>(),
      (const long long*)tsum.data_ptr<int64_t>(),
      (const long long*)tmin.data_ptr<int64_t>(),
      (const long long*)tmax.data_ptr<int64_t>(), nslots, win_lo,
      win_hi, out_keys.data_ptr<int32_t>(),
      out_wins.data_ptr<int32_t>(), out_cnt.data_ptr<int64_t>(),
      out_sum.data_ptr<int64_t>(), out_min.data_ptr<int64_t>(),
      out_max.data_ptr<int64_t>(), out_n.data_ptr<int32_t>(),
      out_keys.numel());
}

// Stats close with reclamation (see k_stats_close_migrate); the launch
// shape of launch_close_migrate.
void stats_close_migrate(
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor nkeys,
    torch::Tensor ncnt,
    torch::Tensor nsum,
    torch::Tensor nmin,
    torch::Tensor nmax,
    int64_t win_lo,
    int64_t win_hi,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_cnt,
    torch::Tensor out_sum,
    torch::Tensor out_min,
    torch::Tensor out_max,
    torch::Tensor out_n,
    torch::Tensor error_flag) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(nkeys, torch::kInt64, "nkeys");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nslots > 0 && (nslots & (nslots - 1)) == 0,
              "table size must be a power of two");
  TORCH_CHECK(nkeys.numel() == nslots, "table size mismatch");
  const torch::Tensor* vals[] = {&tcnt, &tsum, &tmin, &tmax,
                                 &ncnt, &nsum, &nmin, &nmax};
  for (const torch::Tensor* t : vals) {
    check_dev(*t, torch::kInt64, "stats value array");
    TORCH_CHECK(t->numel() == nslots, "table size mismatch");
  }
  check_dev(out_keys, torch::kInt32, "out_keys");
  check_dev(out_wins, torch::kInt32, "out_wins");
  check_dev(out_n, torch::kInt32, "out_n");
  check_dev(error_flag, torch::kInt32, "error_flag");
  TORCH_CHECK(out_n.numel() >= 1 && error_flag.numel() >= 1,
              "out_n and error_flag must hold one element");
  int64_t cap = out_keys.numel();
  TORCH_CHECK(out_wins.numel() == cap, "output size mismatch");
  const torch::Tensor* outs[] = {&out_cnt, &out_sum, &out_min, &out_max};
  for (const torch::Tensor* t : outs) {
    check_dev(*t, torch::kInt64, "stats output column");
    TORCH_CHECK(t->numel() == cap, "output size mismatch");
  }
  int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  unsigned grid = (unsigned)(nchunks < CM_MAX_GRID ? nchunks : CM_MAX_GRID);
  hipLaunchKernelGGL(
      k_stats_close_migrate, dim3(grid), dim3(CM_BLK), 0,
      at::hip::getCurrentHIPStream(),
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const long long*)tcnt.data_ptr<int64_t>(),
      (const long long*)tsum.data_ptr<int64_t>(),
      (const long long*)tmin.data_ptr<int64_t>(),
      (const long long*)tmax.data_ptr<int64_t>(), nslots, win_lo, win_hi,
      (uint64_t*)nkeys.data_ptr<int64_t>(),
      (long long*)ncnt.data_ptr<int64_t>(),
      (long long*)nsum.data_ptr<int64_t>(),
      (long long*)nmin.data_ptr<int64_t>(),
      (long long*)nmax.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
      out_keys.data_ptr<int32_t>(), out_wins.data_ptr<int32_t>(),
      out_cnt.data_ptr<int64_t>(), out_sum.data_ptr<int64_t>(),
      out_min.data_ptr<int64_t>(), out_max.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), cap, error_flag.data_ptr<int32_t>());
}

// Sliding stats close (see k_stats_pane_close): folds the panes of the
// windows in [win_lo, win_hi) into the fold table `f*` and migrates
// the panes at or above `pane_keep` into the fresh table `n*`.  The
// launch shape of stats_close_migrate.
void stats_pane_close(
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor tsum,
    torch::Tensor tmin,
    torch::Tensor tmax,
    torch::Tensor nkeys,
    torch::Tensor ncnt,
    torch::Tensor nsum,
    torch::Tensor nmin,
    torch::Tensor nmax,
    torch::Tensor fkeys,
    torch::Tensor fcnt,
    torch::Tensor fsum,
    torch::Tensor fmin,
    torch::Tensor fmax,
    int64_t win_lo,
    int64_t win_hi,
    int64_t pane_keep,
    int64_t panes_per_window,
    int64_t panes_per_offset,
    torch::Tensor error_flag) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(nkeys, torch::kInt64, "nkeys");
  check_dev(fkeys, torch::kInt64, "fkeys");
  int64_t nslots = tkeys.numel();
  int64_t fslots = fkeys.numel();
  TORCH_CHECK(nslots > 0 && (nslots & (nslots - 1)) == 0,
              "table size must be a power of two");
  TORCH_CHECK(fslots > 0 && (fslots & (fslots - 1)) == 0,
              "fold table size must be a power of two");
  TORCH_CHECK(nkeys.numel() == nslots, "table size mismatch");
  TORCH_CHECK(nkeys.data_ptr() != tkeys.data_ptr() &&
                  fkeys.data_ptr() != tkeys.data_ptr() &&
                  fkeys.data_ptr() != nkeys.data_ptr(),
              "the three tables must be distinct");
  const torch::Tensor* vals[] = {&tcnt, &tsum, &tmin, &tmax,
                                 &ncnt, &nsum, &nmin, &nmax};
  for (const torch::Tensor* t : vals) {
    check_dev(*t, torch::kInt64, "stats value array");
    TORCH_CHECK(t->numel() == nslots, "table size mismatch");
  }
  const torch::Tensor* fvals[] = {&fcnt, &fsum, &fmin, &fmax};
  for (const torch::Tensor* t : fvals) {
    check_dev(*t, torch::kInt64, "fold value array");
    TORCH_CHECK(t->numel() == fslots, "fold table size mismatch");
  }
  check_dev(error_flag, torch::kInt32, "error_flag");
  TORCH_CHECK(error_flag.numel() >= 1, "error_flag must hold one element");
  TORCH_CHECK(panes_per_offset >= 1 && panes_per_window >= panes_per_offset &&
                  panes_per_window <= 64,
              "need 1 <= panes per offset <= panes per window <= 64");
  int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  unsigned grid = (unsigned)(nchunks < CM_MAX_GRID ? nchunks : CM_MAX_GRID);
  hipLaunchKernelGGL(
      k_stats_pane_close, dim3(grid), dim3(CM_BLK), 0,
      at::hip::getCurrentHIPStream(),
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const long long*)tcnt.data_ptr<int64_t>(),
      (const long long*)tsum.data_ptr<int64_t>(),
      (const long long*)tmin.data_ptr<int64_t>(),
      (const long long*)tmax.data_ptr<int64_t>(), nslots, win_lo, win_hi,
      pane_keep, panes_per_window, panes_per_offset,
      (uint64_t*)nkeys.data_ptr<int64_t>(),
      (long long*)ncnt.data_ptr<int64_t>(),
      (long long*)nsum.data_ptr<int64_t>(),
      (long long*)nmin.data_ptr<int64_t>(),
      (long long*)nmax.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
      (uint64_t*)fkeys.data_ptr<int64_t>(),
      (long long*)fcnt.data_ptr<int64_t>(),
      (long long*)fsum.data_ptr<int64_t>(),
      (long long*)fmin.data_ptr<int64_t>(),
      (long long*)fmax.data_ptr<int64_t>(), (uint64_t)(fslots - 1),
      error_flag.data_ptr<int32_t>());
}

void join_insert(
    torch::Tensor keys,
    torch::Tensor vals,
    int64_t side,
    int64_t n_sides,
    torch::Tensor tkeys,
    torch::Tensor tval0,
    torch::Tensor tval1,
    torch::Tensor tflags,
    torch::Tensor out_keys,
    torch::Tensor out_v0,
    torch::Tensor out_v1,
    torch::Tensor out_n,
    torch::Tensor error_flag) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(vals, torch::kInt64, "vals");
  check_dev(tflags, torch::kInt32, "tflags");
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(n_sides == 2, "device join currently supports 2 sides");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  hipLaunchKernelGGL(
      k_join_insert, grid, block, 0, stream, keys.data_ptr<int32_t>(),
      vals.data_ptr<int64_t>(), n, (int)side, (int)n_sides,
      (uint64_t*)tkeys.data_ptr<int64_t>(),
      (long long*)tval0.data_ptr<int64_t>(),
      (long long*)tval1.data_ptr<int64_t>(), tflags.data_ptr<int32_t>(),
      (uint64_t)(nslots - 1), out_keys.data_ptr<int32_t>(),
      out_v0.data_ptr<int64_t>(), out_v1.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), out_keys.numel(),
      error_flag.data_ptr<int32_t>());
}

void radix_join_insert(
    torch::Tensor keys,
    torch::Tensor zeros_ts,  // int64 [>= n] of zeros (key-only packing)
    torch::Tensor vals,
    int64_t side,
    int64_t n_sides,
    torch::Tensor tkeys,
    torch::Tensor tval0,
    torch::Tensor tval1,
    torch::Tensor tflags,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    torch::Tensor out_keys,
    torch::Tensor out_v0,
    torch::Tensor out_v1,
    torch::Tensor out_n,
    torch::Tensor max_ts_scratch,
    torch::Tensor error_flag,
    int64_t region_bits) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(vals, torch::kInt64, "vals");
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(n_sides == 2, "device join currently supports 2 sides");
  TORCH_CHECK(region_bits > 0 && region_bits <= 12, "bad region_bits");
  // Scatter segments one bit coarser than table regions
  // (BYTEWAX_JOIN_COARSE): halves the scatter's cursor LDS (better
  // occupancy, longer runs); the dedup/merge kernel probes the
  // global table by key, so segments need not match regions.
  int64_t coarse = 1;
  if (const char* c = std::getenv("BYTEWAX_JOIN_COARSE")) {
    if (c[0] >= '0' && c[0] <= '3' && c[1] == '\0') coarse = c[0] - '0';
  }
  int64_t seg_bits = region_bits + coarse;
  int64_t nb = nslots >> seg_bits;
  if (nb < 1) {
    nb = 1;
    seg_bits = 0;
    while (((int64_t)1 << seg_bits) < nslots) ++seg_bits;
  }
  int64_t cap = ev_packed.numel() / nb;
  // Staged (line-granule) scatter when the per-region capacity
  // supports it; the fixed variant otherwise.
  ScatterKind kind = scatter_kind_env() == SCAT_FIXED ? SCAT_FIXED
                                                      : SCAT_STAGED;
  size_t staged_lds =
      (size_t)nb * SC_GRAN * 8 * 2 + 4 * (size_t)nb * sizeof(int);
  if (kind == SCAT_STAGED) {
    cap &= ~(int64_t)(SC_GRAN - 1);
    if (cap < SC_GRAN || staged_lds > 160 * 1024) {
      kind = SCAT_FIXED;
      cap = ev_packed.numel() / nb;
    }
  }
  TORCH_CHECK(cap * nb >= 2 * n || cap >= n, "scatter buffers too small");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  gcursors.narrow(0, 0, nb).zero_();
  ov_cursor.zero_();
  size_t hist_lds = (size_t)nb * sizeof(int);
  // Key-only packing: ts == 0, align 0, huge window -> win = 0.
  // 512-thread workgroups + grid 1024: same tuning as the stats SUM
  // scatter (profiles/r02 call 29: the scatter is 63% of join time).
  if (kind == SCAT_STAGED) {
    unsigned gs = (unsigned)((n + 8191) / 8192);
    if (gs > 1024) gs = 1024;
    if (gs < 1) gs = 1;
    hipLaunchKernelGGL(
        (k_radix_scatter_staged<AGG_SUM, int64_t, 16, 512>), dim3(gs),
        dim3(512), staged_lds,
        stream, keys.data_ptr<int32_t>(), zeros_ts.data_ptr<int64_t>(),
        vals.data_ptr<int64_t>(), n, 0, (int64_t)1 << 40,
        (int64_t)1 << 40, 0, mask,
        (int)seg_bits, cap, gcursors.data_ptr<int32_t>(),
        (uint64_t*)ev_packed.data_ptr<int64_t>(), ev_vals.data_ptr<int64_t>(),
        ov_cursor.data_ptr<int32_t>(),
        (uint64_t*)ov_packed.data_ptr<int64_t>(), ov_vals.data_ptr<int64_t>(),
        ov_packed.numel(),
        (unsigned long long*)max_ts_scratch.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), (uint64_t)1 << 24, ~(uint64_t)0,
        NO_LATE_ARGS);
  } else {
    hipLaunchKernelGGL(
        k_radix_scatter_fixed<AGG_SUM>, grid, block, 2 * hist_lds, stream,
        keys.data_ptr<int32_t>(), zeros_ts.data_ptr<int64_t>(),
        vals.data_ptr<int64_t>(), n, 0, (int64_t)1 << 40, (int64_t)1 << 40,
        0, mask,
        (int)seg_bits, cap, gcursors.data_ptr<int32_t>(),
        (uint64_t*)ev_packed.data_ptr<int64_t>(), ev_vals.data_ptr<int64_t>(),
        ov_cursor.data_ptr<int32_t>(),
        (uint64_t*)ov_packed.data_ptr<int64_t>(), ov_vals.data_ptr<int64_t>(),
        ov_packed.numel(),
        (unsigned long long*)max_ts_scratch.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), (uint64_t)1 << 24, ~(uint64_t)0,
        NO_LATE_ARGS);
  }
  // LDS staging sized one bit above the segment's table span
  // (2^seg_bits cells per segment); headroom keeps the in-LDS probe
  // chains short at high per-segment cardinality.
  int lds_bits = (int)seg_bits + 1;
  if (lds_bits < 6) lds_bits = 6;
  if (lds_bits > 12) lds_bits = 12;
  // 8 B key + 8 B value + 4 B event count per LDS slot.
  size_t join_lds = (size_t)20 << lds_bits;
  if (join_lds_env() && join_lds <= 144 * 1024) {
    // 1024 threads/workgroup: the merge kernel is LDS-atomic latency
    // bound, so more waves in flight per block hide it (sweep r02
    // call 31: 256 -> 17.3, 512 -> 20.2, 1024 -> 20.5 Ge/s;
    // BYTEWAX_JOIN_THREADS overrides).
    int jthreads = 1024;
    if (const char* t = std::getenv("BYTEWAX_JOIN_THREADS")) {
      int v = std::atoi(t);
      if (v == 256 || v == 512 || v == 1024) jthreads = v;
    }
    auto launch_lds = [&](auto kern, int thr) {
      hipLaunchKernelGGL(
          kern, dim3((unsigned)nb), dim3(thr), join_lds, stream,
          (const uint64_t*)ev_packed.data_ptr<int64_t>(),
          ev_vals.data_ptr<int64_t>(), gcursors.data_ptr<int32_t>(), cap,
          (int)side, (int)n_sides, (uint64_t*)tkeys.data_ptr<int64_t>(),
          (long long*)tval0.data_ptr<int64_t>(),
          (long long*)tval1.data_ptr<int64_t>(), tflags.data_ptr<int32_t>(),
          mask, (int)region_bits, lds_bits, out_keys.data_ptr<int32_t>(),
          out_v0.data_ptr<int64_t>(), out_v1.data_ptr<int64_t>(),
          out_n.data_ptr<int32_t>(), out_keys.numel(),
          error_flag.data_ptr<int32_t>());
    };
    if (jthreads == 1024) launch_lds(k_join_region_lds<1024>, 1024);
    else if (jthreads == 512) launch_lds(k_join_region_lds<512>, 512);
    else launch_lds(k_join_region_lds<256>, 256);
  } else {
    hipLaunchKernelGGL(
        k_join_region, dim3((unsigned)nb), block, 0, stream,
        (const uint64_t*)ev_packed.data_ptr<int64_t>(),
        ev_vals.data_ptr<int64_t>(), gcursors.data_ptr<int32_t>(), cap,
        (int)side, (int)n_sides, (uint64_t*)tkeys.data_ptr<int64_t>(),
        (long long*)tval0.data_ptr<int64_t>(),
        (long long*)tval1.data_ptr<int64_t>(), tflags.data_ptr<int32_t>(),
        mask, (int)region_bits, out_keys.data_ptr<int32_t>(),
        out_v0.data_ptr<int64_t>(), out_v1.data_ptr<int64_t>(),
        out_n.data_ptr<int32_t>(), out_keys.numel(),
        error_flag.data_ptr<int32_t>());
  }
  hipLaunchKernelGGL(
      k_join_overflow, dim3(64), block, 0, stream,
      (const uint64_t*)ov_packed.data_ptr<int64_t>(),
      ov_vals.data_ptr<int64_t>(), ov_cursor.data_ptr<int32_t>(),
      ov_packed.numel(), (int)side, (int)n_sides,
      (uint64_t*)tkeys.data_ptr<int64_t>(),
      (long long*)tval0.data_ptr<int64_t>(),
      (long long*)tval1.data_ptr<int64_t>(), tflags.data_ptr<int32_t>(),
      mask, (int)region_bits, out_keys.data_ptr<int32_t>(),
      out_v0.data_ptr<int64_t>(), out_v1.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), out_keys.numel(),
      error_flag.data_ptr<int32_t>());
}

// Batch-level session merge: when the gap is at least the batch's
// time span, no session boundary can fall INSIDE the batch, so each
// key's per-batch (count, min_ts, max_ts) — computed by the radix
// stats kernels at full speed — is merged as one unit.  Requires
// watermark-ordered batches (each batch's events at/after the
// previous batch's), the same contract as the sorted walk.
__global__ void k_session_merge_batch(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ cnt,
    const int64_t* __restrict__ mn_ts,
    const int64_t* __restrict__ mx_ts,
    const int* __restrict__ n_rows,
    int64_t ts_shift,  // add to mn/mx (zero-based batch timestamps)
    int64_t gap_ms,
    uint64_t* __restrict__ skeys,
    long long* __restrict__ sstart,
    long long* __restrict__ slast,
    long long* __restrict__ sacc,
    uint64_t mask,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_start,
    int64_t* __restrict__ out_end,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t out_cap,
    unsigned long long* __restrict__ max_ts,
    int* __restrict__ error_flag) {
  int64_t n = *n_rows;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  int64_t local_max = 0;
  for (; i < n; i += stride) {
    uint64_t key = (uint64_t)(uint32_t)keys[i];
    uint64_t slot = session_find_or_claim(skeys, mask, key);
    if (slot == ~0ULL) {
      atomicOr(error_flag, 1);
      continue;
    }
    long long lo = mn_ts[i] + ts_shift;
    long long hi = mx_ts[i] + ts_shift;
    long long c = cnt[i];
    if (hi > local_max) local_max = hi;
    long long last = slast[slot];
    if (last >= 0 && lo - last > gap_ms) {
      int idx = atomicAdd(out_n, 1);
      if (idx < out_cap) {
        out_keys[idx] = (int32_t)(uint32_t)key;
        out_start[idx] = sstart[slot];
        out_end[idx] = last;
        out_vals[idx] = sacc[slot];
      } else {
        atomicOr(error_flag, 1);
      }
      last = -1;
    }
    if (last < 0) {
      sstart[slot] = lo;
      sacc[slot] = c;
    } else {
      sacc[slot] += c;
    }
    slast[slot] = hi;
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int64_t other = __shfl_down((long long)local_max, off);
    if (other > local_max) local_max = other;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0 && local_max > 0) {
    atomicMax(max_ts, (unsigned long long)local_max);
  }
}

__global__ void k_session_restore(
    const int32_t* __restrict__ keys,
    const int64_t* __restrict__ start,
    const int64_t* __restrict__ last,
    const int64_t* __restrict__ acc,
    int64_t n,
    uint64_t* __restrict__ skeys,
    long long* __restrict__ sstart,
    long long* __restrict__ slast,
    long long* __restrict__ sacc,
    uint64_t mask,
    int* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    uint64_t slot = session_find_or_claim(
        skeys, mask, (uint64_t)(uint32_t)keys[i]);
    if (slot == ~0ULL) {
      atomicOr(error_flag, 1);
      continue;
    }
    sstart[slot] = start[i];
    slast[slot] = last[i];
    sacc[slot] = acc[i];
  }
}

// Fused radix session aggregation (the fast path's round-2 rework):
// an AGG_TS scatter partitions (key, t) pairs into per-segment runs;
// one block then LDS-aggregates its segment's per-key
// (count, min_ts, max_ts) and merges each distinct key ONCE into the
// session table with the k_session_merge_batch semantics.  Replaces
// the stats-table round trip (insert + extract + merge + 5 table
// clears per batch).  Contract: gap >= batch time span and
// watermark-ordered batches (same as the batch merge).  min/max
// guards keep multi-merge (overflow spill) within one batch exact.
__device__ inline void session_merge_cell(
    uint64_t* skeys, long long* sstart, long long* slast,
    long long* sacc, uint64_t mask, uint64_t key, long long lo,
    long long hi, long long c, int64_t gap_ms,
    int32_t* out_keys, int64_t* out_start, int64_t* out_end,
    int64_t* out_vals, int* out_n, int64_t out_cap, int* error_flag) {
  uint64_t slot = session_find_or_claim(skeys, mask, key);
  if (slot == ~0ULL) {
    atomicOr(error_flag, 1);
    return;
  }
  long long last = slast[slot];
  if (last >= 0 && lo - last > gap_ms) {
    int idx = atomicAdd(out_n, 1);
    if (idx < out_cap) {
      out_keys[idx] = (int32_t)(uint32_t)key;
      out_start[idx] = sstart[slot];
      out_end[idx] = last;
      out_vals[idx] = sacc[slot];
    } else {
      atomicOr(error_flag, 1);
    }
    last = -1;
  }
  if (last < 0) {
    sstart[slot] = lo;
    sacc[slot] = c;
    slast[slot] = hi;
  } else {
    sacc[slot] += c;
    if (lo < sstart[slot]) sstart[slot] = lo;
    if (hi > slast[slot]) slast[slot] = hi;
  }
}

__global__ __launch_bounds__(1024) void k_radix_session_agg(
    const uint64_t* __restrict__ ev_packed,  // keys (AGG_TS packing)
    const int64_t* __restrict__ ev_vals,     // absolute timestamps
    const int* __restrict__ offsets,
    const int* __restrict__ counts,
    int64_t clamp_cap,
    int lds_bits,
    uint64_t* __restrict__ skeys,
    long long* __restrict__ sstart,
    long long* __restrict__ slast,
    long long* __restrict__ sacc,
    uint64_t mask,
    int64_t gap_ms,
    int* __restrict__ ov_cursor,
    uint64_t* __restrict__ ov_packed,
    int64_t* __restrict__ ov_vals,
    int64_t ov_cap,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_start,
    int64_t* __restrict__ out_end,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  extern __shared__ char smem[];
  int slots = 1 << lds_bits;
  uint64_t* lkeys = (uint64_t*)smem;
  long long* lcnt = (long long*)(smem + (size_t)slots * 8);
  long long* lmn = lcnt + slots;
  long long* lmx = lmn + slots;
  for (int s = threadIdx.x; s < slots; s += blockDim.x) {
    lkeys[s] = EMPTY_SLOT;
    lcnt[s] = 0;
    lmn[s] = 0x7FFFFFFFFFFFFFFFLL;
    lmx[s] = -0x7FFFFFFFFFFFFFFFLL;
  }
  __syncthreads();
  int b = blockIdx.x;
  int cnt = counts[b];
  if (clamp_cap > 0 && cnt > (int)clamp_cap) cnt = (int)clamp_cap;
  int start = offsets[b];
  for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
    uint64_t key = ev_packed[start + j];
    if (key == EMPTY_SLOT) continue;  // staged-scatter pad
    long long t = ev_vals[start + j];
    uint64_t h64 = mix64(key);
    int lh = (int)((h64 >> 32) & (slots - 1));
    bool done = false;
    for (int p = 0; p < slots; ++p) {
      uint64_t cur = lkeys[lh];
      if (cur == EMPTY_SLOT) {
        uint64_t prev = atomicCAS(
            (unsigned long long*)&lkeys[lh], EMPTY_SLOT, key);
        cur = (prev == EMPTY_SLOT) ? key : prev;
      }
      if (cur == key) {
        atomicAdd((unsigned long long*)&lcnt[lh], 1ULL);
        atomicMin(&lmn[lh], t);
        atomicMax(&lmx[lh], t);
        done = true;
        break;
      }
      lh = (lh + 1) & (slots - 1);
    }
    if (!done) {
      // LDS staging full: spill to the (sequential) overflow walk.
      int opos = atomicAdd(ov_cursor, 1);
      if (opos < ov_cap) {
        ov_packed[opos] = key;
        ov_vals[opos] = t;
      } else {
        atomicOr(error_flag, 1);
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < slots; s += blockDim.x) {
    if (lkeys[s] == EMPTY_SLOT) continue;
    session_merge_cell(
        skeys, sstart, slast, sacc, mask, lkeys[s], lmn[s], lmx[s],
        lcnt[s], gap_ms, out_keys, out_start, out_end, out_vals, out_n,
        out_cap, error_flag);
  }
}

// Sequential overflow walk: one thread merges spilled (key, t) pairs
// per event — order within the batch does not matter under the
// gap >= span contract (no close can trigger between same-batch
// merges; min/max guards keep start/last exact).  Slow by design;
// reached only under extreme key skew or LDS overflow.
__global__ void k_session_ov_walk(
    const uint64_t* __restrict__ ov_packed,
    const int64_t* __restrict__ ov_vals,
    const int* __restrict__ ov_cursor,
    int64_t ov_cap,
    uint64_t* __restrict__ skeys,
    long long* __restrict__ sstart,
    long long* __restrict__ slast,
    long long* __restrict__ sacc,
    uint64_t mask,
    int64_t gap_ms,
    int32_t* __restrict__ out_keys,
    int64_t* __restrict__ out_start,
    int64_t* __restrict__ out_end,
    int64_t* __restrict__ out_vals,
    int* __restrict__ out_n,
    int64_t out_cap,
    int* __restrict__ error_flag) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t n = *ov_cursor;
  if (n > ov_cap) n = ov_cap;
  for (int64_t i = 0; i < n; ++i) {
    session_merge_cell(
        skeys, sstart, slast, sacc, mask, ov_packed[i], ov_vals[i],
        ov_vals[i], 1, gap_ms, out_keys, out_start, out_end, out_vals,
        out_n, out_cap, error_flag);
  }
}

void session_insert(
    torch::Tensor keys,  // SORTED by (key, ts)
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor seg_start,
    torch::Tensor seg_end,
    torch::Tensor skeys,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor out_keys,
    torch::Tensor out_start,
    torch::Tensor out_end,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t gap_ms,
    int64_t mode) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(ts, torch::kInt64, "ts");
  int64_t nslots = skeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  int64_t n_segs = seg_start.numel();
  if (n_segs == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n_segs, 256));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, grid, block, 0, stream, keys.data_ptr<int32_t>(),
        ts.data_ptr<int64_t>(),
        mode == AGG_SUM ? vals->data_ptr<int64_t>() : nullptr,
        seg_start.data_ptr<int64_t>(), seg_end.data_ptr<int64_t>(),
        n_segs, gap_ms, (uint64_t*)skeys.data_ptr<int64_t>(),
        (long long*)sstart.data_ptr<int64_t>(),
        (long long*)slast.data_ptr<int64_t>(),
        (long long*)sacc.data_ptr<int64_t>(),
        (uint64_t)(nslots - 1), out_keys.data_ptr<int32_t>(),
        out_start.data_ptr<int64_t>(), out_end.data_ptr<int64_t>(),
        out_vals.data_ptr<int64_t>(), out_n.data_ptr<int32_t>(),
        out_keys.numel(),
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>());
  };
  if (mode == AGG_COUNT) launch(k_session_insert<AGG_COUNT>);
  else launch(k_session_insert<AGG_SUM>);
}

void session_close_migrate(
    torch::Tensor skeys,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor dst_keys,
    torch::Tensor dst_start,
    torch::Tensor dst_last,
    torch::Tensor dst_acc,
    torch::Tensor out_keys,
    torch::Tensor out_start,
    torch::Tensor out_end,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    torch::Tensor error_flag,
    int64_t horizon_ms) {
  int64_t nslots = skeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  hipLaunchKernelGGL(
      k_session_close_migrate, dim3(n_blocks(nslots, 256)), block, 0,
      stream, (const uint64_t*)skeys.data_ptr<int64_t>(),
      (const long long*)sstart.data_ptr<int64_t>(),
      (const long long*)slast.data_ptr<int64_t>(),
      (const long long*)sacc.data_ptr<int64_t>(), nslots, horizon_ms,
      (uint64_t*)dst_keys.data_ptr<int64_t>(),
      (long long*)dst_start.data_ptr<int64_t>(),
      (long long*)dst_last.data_ptr<int64_t>(),
      (long long*)dst_acc.data_ptr<int64_t>(),
      (uint64_t)(nslots - 1), out_keys.data_ptr<int32_t>(),
      out_start.data_ptr<int64_t>(), out_end.data_ptr<int64_t>(),
      out_vals.data_ptr<int64_t>(), out_n.data_ptr<int32_t>(),
      out_keys.numel(), error_flag.data_ptr<int32_t>());
}

void session_merge_batch(
    torch::Tensor keys,
    torch::Tensor cnt,
    torch::Tensor mn_ts,
    torch::Tensor mx_ts,
    torch::Tensor n_rows,
    torch::Tensor skeys,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor out_keys,
    torch::Tensor out_start,
    torch::Tensor out_end,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t ts_shift,
    int64_t gap_ms) {
  int64_t nslots = skeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  hipLaunchKernelGGL(
      k_session_merge_batch, dim3(n_blocks(out_keys.numel(), 256)),
      block, 0, stream, keys.data_ptr<int32_t>(),
      cnt.data_ptr<int64_t>(), mn_ts.data_ptr<int64_t>(),
      mx_ts.data_ptr<int64_t>(), n_rows.data_ptr<int32_t>(), ts_shift,
      gap_ms, (uint64_t*)skeys.data_ptr<int64_t>(),
      (long long*)sstart.data_ptr<int64_t>(),
      (long long*)slast.data_ptr<int64_t>(),
      (long long*)sacc.data_ptr<int64_t>(),
      (uint64_t)(nslots - 1), out_keys.data_ptr<int32_t>(),
      out_start.data_ptr<int64_t>(), out_end.data_ptr<int64_t>(),
      out_vals.data_ptr<int64_t>(), out_n.data_ptr<int32_t>(),
      out_keys.numel(),
      (unsigned long long*)max_ts.data_ptr<int64_t>(),
      error_flag.data_ptr<int32_t>());
}

void session_restore(
    torch::Tensor keys,
    torch::Tensor start,
    torch::Tensor last,
    torch::Tensor acc,
    torch::Tensor skeys,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor error_flag) {
  check_dev(keys, torch::kInt32, "keys");
  int64_t n = keys.numel();
  if (n == 0) return;
  int64_t nslots = skeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  hipLaunchKernelGGL(
      k_session_restore, dim3(n_blocks(n, 256)), block, 0, stream,
      keys.data_ptr<int32_t>(), start.data_ptr<int64_t>(),
      last.data_ptr<int64_t>(), acc.data_ptr<int64_t>(), n,
      (uint64_t*)skeys.data_ptr<int64_t>(),
      (long long*)sstart.data_ptr<int64_t>(),
      (long long*)slast.data_ptr<int64_t>(),
      (long long*)sacc.data_ptr<int64_t>(),
      (uint64_t)(nslots - 1), error_flag.data_ptr<int32_t>());
}

// Collapse a (key, ts)-sorted batch into runs.  Returns
// {run_key, run_start, run_last, run_acc, n_runs}; the run columns
// are sized for the worst case (one run per event) and `n_runs` stays
// on the device, so the call never synchronises.
std::vector<torch::Tensor> session_run_collapse(
    torch::Tensor keys,  // SORTED by (key, ts)
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    int64_t gap_ms,
    int64_t mode) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(ts, torch::kInt64, "ts");
  int64_t n = keys.numel();
  TORCH_CHECK(n > 0, "session_run_collapse needs a non-empty batch");
  TORCH_CHECK(ts.numel() == n, "keys/ts length mismatch");
  TORCH_CHECK(gap_ms >= 0, "gap must not be negative");
  TORCH_CHECK(mode == AGG_COUNT || mode == AGG_SUM, "count or sum only");
  const int64_t* vals_p = nullptr;
  if (mode == AGG_SUM) {
    TORCH_CHECK(vals.has_value(), "sum sessions need a vals column");
    check_dev(*vals, torch::kInt64, "vals");
    TORCH_CHECK(vals->numel() == n, "keys/vals length mismatch");
    vals_p = vals->data_ptr<int64_t>();
  }
  int64_t nblk = (n + SESS_RUN_BLK - 1) / SESS_RUN_BLK;
  TORCH_CHECK(nblk < (1LL << 31), "batch too large");
  auto i32 = keys.options().dtype(torch::kInt32);
  auto i64 = keys.options().dtype(torch::kInt64);
  auto block_heads = torch::empty({nblk}, i32);
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid((unsigned)nblk), block(SESS_RUN_BLK);
  hipLaunchKernelGGL(
      k_session_run_count, grid, block, 0, stream,
      keys.data_ptr<int32_t>(), ts.data_ptr<int64_t>(), n, gap_ms,
      block_heads.data_ptr<int32_t>());
  auto incl = block_heads.cumsum(0, torch::kInt64);
  auto block_off = incl - block_heads;
  auto n_runs = incl.slice(0, nblk - 1, nblk).contiguous();
  auto run_key = torch::empty({n}, i32);
  auto run_start = torch::empty({n}, i64);
  auto run_last = torch::empty({n}, i64);
  auto run_acc = torch::zeros({n}, i64);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, grid, block, 0, stream, keys.data_ptr<int32_t>(),
        ts.data_ptr<int64_t>(), vals_p, n, gap_ms,
        block_off.data_ptr<int64_t>(), run_key.data_ptr<int32_t>(),
        (long long*)run_start.data_ptr<int64_t>(),
        (long long*)run_last.data_ptr<int64_t>(),
        (unsigned long long*)run_acc.data_ptr<int64_t>());
  };
  if (mode == AGG_COUNT) launch(k_session_run_collapse<AGG_COUNT>);
  else launch(k_session_run_collapse<AGG_SUM>);
  return {run_key, run_start, run_last, run_acc, n_runs};
}

// Merge runs (sorted by (key, start), gap-separated per key) into the
// multi-session table.  Also the restore path: snapshot rows are runs.
void session_run_merge(
    torch::Tensor run_key,
    torch::Tensor run_start,
    torch::Tensor run_last,
    torch::Tensor run_acc,
    torch::Tensor n_runs,
    torch::Tensor skeys,
    torch::Tensor scnt,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t gap_ms,
    int64_t max_open) {
  check_dev(run_key, torch::kInt32, "run_key");
  check_dev(run_start, torch::kInt64, "run_start");
  check_dev(run_last, torch::kInt64, "run_last");
  check_dev(run_acc, torch::kInt64, "run_acc");
  check_dev(n_runs, torch::kInt64, "n_runs");
  check_dev(scnt, torch::kInt32, "scnt");
  int64_t cap = run_key.numel();
  if (cap == 0) return;
  TORCH_CHECK(run_start.numel() >= cap && run_last.numel() >= cap &&
                  run_acc.numel() >= cap && n_runs.numel() == 1,
              "run columns shorter than run_key");
  int64_t nslots = skeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(scnt.numel() == nslots &&
                  sstart.numel() == nslots * max_open &&
                  slast.numel() == nslots * max_open &&
                  sacc.numel() == nslots * max_open,
              "session table shape does not match max_open");
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(
        kern, dim3(n_blocks(cap, WAVE)), dim3(WAVE), 0, stream,
        run_key.data_ptr<int32_t>(),
        (const long long*)run_start.data_ptr<int64_t>(),
        (const long long*)run_last.data_ptr<int64_t>(),
        (const long long*)run_acc.data_ptr<int64_t>(),
        n_runs.data_ptr<int64_t>(), cap, gap_ms,
        (uint64_t*)skeys.data_ptr<int64_t>(), scnt.data_ptr<int32_t>(),
        (long long*)sstart.data_ptr<int64_t>(),
        (long long*)slast.data_ptr<int64_t>(),
        (long long*)sacc.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>());
  };
  switch (max_open) {
    case 4: launch(k_session_run_merge<4>); break;
    case 8: launch(k_session_run_merge<8>); break;
    case 16: launch(k_session_run_merge<16>); break;
    case 32: launch(k_session_run_merge<32>); break;
    default: TORCH_CHECK(false, "max_open must be 4, 8, 16 or 32");
  }
}

void session_multi_close_migrate(
    torch::Tensor skeys,
    torch::Tensor scnt,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor dst_keys,
    torch::Tensor dst_cnt,
    torch::Tensor dst_start,
    torch::Tensor dst_last,
    torch::Tensor dst_acc,
    torch::Tensor out_keys,
    torch::Tensor out_start,
    torch::Tensor out_end,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    torch::Tensor error_flag,
    int64_t horizon_ms,
    int64_t max_open) {
  check_dev(scnt, torch::kInt32, "scnt");
  check_dev(dst_cnt, torch::kInt32, "dst_cnt");
  int64_t nslots = skeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(max_open >= 1 && max_open <= 32, "bad max_open");
  TORCH_CHECK(dst_keys.numel() == nslots && scnt.numel() == nslots &&
                  dst_cnt.numel() == nslots,
              "session tables differ in size");
  for (const auto& t : {sstart, slast, sacc, dst_start, dst_last, dst_acc}) {
    TORCH_CHECK(t.numel() == nslots * max_open,
                "session table shape does not match max_open");
  }
  int64_t out_cap = out_keys.numel();
  TORCH_CHECK(out_start.numel() >= out_cap && out_end.numel() >= out_cap &&
                  out_vals.numel() >= out_cap,
              "out columns shorter than out_keys");
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      k_session_multi_close_migrate, dim3(n_blocks(nslots, 256)),
      dim3(256), 0, stream, (const uint64_t*)skeys.data_ptr<int64_t>(),
      scnt.data_ptr<int32_t>(),
      (const long long*)sstart.data_ptr<int64_t>(),
      (const long long*)slast.data_ptr<int64_t>(),
      (const long long*)sacc.data_ptr<int64_t>(), nslots, (int)max_open,
      horizon_ms, (uint64_t*)dst_keys.data_ptr<int64_t>(),
      dst_cnt.data_ptr<int32_t>(),
      (long long*)dst_start.data_ptr<int64_t>(),
      (long long*)dst_last.data_ptr<int64_t>(),
      (long long*)dst_acc.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
      out_keys.data_ptr<int32_t>(), out_start.data_ptr<int64_t>(),
      out_end.data_ptr<int64_t>(), out_vals.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), out_cap,
      error_flag.data_ptr<int32_t>());
}

void join_extract(
    torch::Tensor tkeys,
    torch::Tensor tval0,
    torch::Tensor tval1,
    torch::Tensor tflags,
    torch::Tensor out_keys,
    torch::Tensor out_v0,
    torch::Tensor out_v1,
    torch::Tensor out_flags,
    torch::Tensor out_n) {
  int64_t nslots = tkeys.numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(nslots, 256));
  hipLaunchKernelGGL(
      k_join_extract, grid, block, 0, stream,
      (uint64_t*)tkeys.data_ptr<int64_t>(),
      (long long*)tval0.data_ptr<int64_t>(),
      (long long*)tval1.data_ptr<int64_t>(), tflags.data_ptr<int32_t>(),
      nslots, out_keys.data_ptr<int32_t>(), out_v0.data_ptr<int64_t>(),
      out_v1.data_ptr<int64_t>(), out_flags.data_ptr<int32_t>(),
      out_n.data_ptr<int32_t>(), out_keys.numel());
}

// One side's batch into the windowed-join table: the stamp, elect and
// commit launches of k_wjoin_stamp on the current stream.  `tts` and
// `tval` are the side's arrays, `ev_slot` a scratch of at least n
// int32.  `ts` is absolute int64 or int32 deltas against `ts_base`.
static void wjoin_insert_impl(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tts,
    torch::Tensor tval,
    torch::Tensor telect,
    torch::Tensor ev_slot,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    bool first,
    const LateSink* late) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(vals, torch::kInt64, "vals");
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(tts, torch::kInt64, "tts");
  check_dev(tval, torch::kInt64, "tval");
  check_dev(telect, torch::kInt32, "telect");
  check_dev(ev_slot, torch::kInt32, "ev_slot");
  check_dev(max_ts, torch::kInt64, "max_ts");
  check_dev(error_flag, torch::kInt32, "error_flag");
  const bool ts32 = ts.scalar_type() == torch::kInt32;
  check_dev(ts, ts32 ? torch::kInt32 : torch::kInt64, "ts");
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nslots > 0 && (nslots & (nslots - 1)) == 0,
              "table size must be a power of two");
  // ev_slot holds slot indices as int32.
  TORCH_CHECK(nslots <= (int64_t)1 << 30, "table too large");
  TORCH_CHECK(tts.numel() == nslots && tval.numel() == nslots &&
                  telect.numel() == nslots,
              "table size mismatch");
  TORCH_CHECK(ts.numel() == n && vals.numel() == n, "column size mismatch");
  TORCH_CHECK(ev_slot.numel() >= n, "ev_slot too small");
  // Row indices are bid as int32 below the election sentinels.
  TORCH_CHECK(n < (int64_t)WJ_OPEN, "batch too large");
  TORCH_CHECK(len_ms > 0, "window length must be positive");
  TORCH_CHECK(max_ts.numel() >= 1 && error_flag.numel() >= 1,
              "max_ts and error_flag must hold one element");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  auto run = [&](auto first_c, auto* tsp) {
    constexpr bool F = decltype(first_c)::value;
    using TSV = std::remove_cv_t<std::remove_pointer_t<decltype(tsp)>>;
    auto stamp = [&](auto kern, auto... extra) {
      hipLaunchKernelGGL(
          kern, grid, block, 0, stream, keys.data_ptr<int32_t>(), tsp,
          (const int64_t*)vals.data_ptr<int64_t>(), n,
          (uint64_t*)tkeys.data_ptr<int64_t>(),
          (long long*)tts.data_ptr<int64_t>(), telect.data_ptr<int32_t>(),
          (uint64_t)(nslots - 1), align_ms, len_ms, ts_base,
          ev_slot.data_ptr<int32_t>(),
          (unsigned long long*)max_ts.data_ptr<int64_t>(),
          error_flag.data_ptr<int32_t>(), extra...);
    };
    if (late != nullptr)
      stamp(k_wjoin_stamp<F, TSV, true>, late->cutoff, late->keys, late->ts,
            late->vals, late->n, late->cap);
    else
      stamp(k_wjoin_stamp<F, TSV, false>, NO_LATE_ARGS);
    hipLaunchKernelGGL(
        (k_wjoin_elect<F, TSV>), grid, block, 0, stream, tsp, n, ts_base,
        (const long long*)tts.data_ptr<int64_t>(),
        telect.data_ptr<int32_t>(),
        (const int32_t*)ev_slot.data_ptr<int32_t>());
    hipLaunchKernelGGL(
        (k_wjoin_commit<F>), grid, block, 0, stream,
        (const int64_t*)vals.data_ptr<int64_t>(), n,
        (long long*)tval.data_ptr<int64_t>(), telect.data_ptr<int32_t>(),
        (const int32_t*)ev_slot.data_ptr<int32_t>());
  };
  auto by_ts = [&](auto first_c) {
    if (ts32)
      run(first_c, (const int32_t*)ts.data_ptr<int32_t>());
    else
      run(first_c, (const int64_t*)ts.data_ptr<int64_t>());
  };
  if (first)
    by_ts(std::true_type{});
  else
    by_ts(std::false_type{});
}

void wjoin_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tts,
    torch::Tensor tval,
    torch::Tensor telect,
    torch::Tensor ev_slot,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    bool first) {
  wjoin_insert_impl(keys, ts, vals, tkeys, tts, tval, telect, ev_slot, max_ts,
                    error_flag, align_ms, len_ms, ts_base, first, nullptr);
}

// Late-tracking form of wjoin_insert (see window_agg_insert_late): an
// event with absolute t < late_cutoff goes to the late buffer with its
// value and takes no part in the stamp, elect or commit pass.
void wjoin_insert_late(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tts,
    torch::Tensor tval,
    torch::Tensor telect,
    torch::Tensor ev_slot,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base,
    bool first,
    int64_t late_cutoff,
    torch::Tensor late_keys,
    torch::Tensor late_ts,
    torch::Tensor late_vals,
    torch::Tensor late_n) {
  c10::optional<torch::Tensor> lv(late_vals);
  LateSink sink =
      make_late_sink(late_cutoff, late_keys, late_ts, lv, late_n, true);
  wjoin_insert_impl(keys, ts, vals, tkeys, tts, tval, telect, ev_slot, max_ts,
                    error_flag, align_ms, len_ms, ts_base, first, &sink);
}

static void check_wjoin_table(
    const torch::Tensor& tkeys, const torch::Tensor* const* cols, int ncols) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nslots > 0 && (nslots & (nslots - 1)) == 0,
              "table size must be a power of two");
  for (int i = 0; i < ncols; ++i) {
    check_dev(*cols[i], torch::kInt64, "window join table array");
    TORCH_CHECK(cols[i]->numel() == nslots, "table size mismatch");
  }
}

// Windowed-join close with reclamation (see k_wjoin_close_migrate);
// the launch shape of stats_close_migrate.  `ts_none` is the stamp of
// an absent side.
void wjoin_close_migrate(
    torch::Tensor tkeys,
    torch::Tensor tts0,
    torch::Tensor tts1,
    torch::Tensor tv0,
    torch::Tensor tv1,
    torch::Tensor nkeys,
    torch::Tensor nts0,
    torch::Tensor nts1,
    torch::Tensor nv0,
    torch::Tensor nv1,
    int64_t win_lo,
    int64_t win_hi,
    int64_t ts_none,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_v0,
    torch::Tensor out_v1,
    torch::Tensor out_mask,
    torch::Tensor out_n,
    torch::Tensor error_flag) {
  const torch::Tensor* live[] = {&tts0, &tts1, &tv0, &tv1};
  const torch::Tensor* fresh[] = {&nts0, &nts1, &nv0, &nv1};
  check_wjoin_table(tkeys, live, 4);
  check_wjoin_table(nkeys, fresh, 4);
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nkeys.numel() == nslots, "table size mismatch");
  check_dev(out_keys, torch::kInt32, "out_keys");
  check_dev(out_wins, torch::kInt32, "out_wins");
  check_dev(out_mask, torch::kInt32, "out_mask");
  check_dev(out_v0, torch::kInt64, "out_v0");
  check_dev(out_v1, torch::kInt64, "out_v1");
  check_dev(out_n, torch::kInt32, "out_n");
  check_dev(error_flag, torch::kInt32, "error_flag");
  TORCH_CHECK(out_n.numel() >= 1 && error_flag.numel() >= 1,
              "out_n and error_flag must hold one element");
  int64_t cap = out_keys.numel();
  TORCH_CHECK(out_wins.numel() == cap && out_mask.numel() == cap &&
                  out_v0.numel() == cap && out_v1.numel() == cap,
              "output size mismatch");
  int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  unsigned grid = (unsigned)(nchunks < CM_MAX_GRID ? nchunks : CM_MAX_GRID);
  hipLaunchKernelGGL(
      k_wjoin_close_migrate, dim3(grid), dim3(CM_BLK), 0,
      at::hip::getCurrentHIPStream(),
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const long long*)tts0.data_ptr<int64_t>(),
      (const long long*)tts1.data_ptr<int64_t>(),
      (const long long*)tv0.data_ptr<int64_t>(),
      (const long long*)tv1.data_ptr<int64_t>(), nslots, win_lo, win_hi,
      (long long)ts_none, (uint64_t*)nkeys.data_ptr<int64_t>(),
      (long long*)nts0.data_ptr<int64_t>(),
      (long long*)nts1.data_ptr<int64_t>(),
      (long long*)nv0.data_ptr<int64_t>(),
      (long long*)nv1.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
      out_keys.data_ptr<int32_t>(), out_wins.data_ptr<int32_t>(),
      out_v0.data_ptr<int64_t>(), out_v1.data_ptr<int64_t>(),
      out_mask.data_ptr<int32_t>(), out_n.data_ptr<int32_t>(), cap,
      error_flag.data_ptr<int32_t>());
}

// Non-mutating extract of the windowed-join cells in [win_lo, win_hi)
// (see k_wjoin_extract).
void wjoin_extract(
    torch::Tensor tkeys,
    torch::Tensor tts0,
    torch::Tensor tts1,
    torch::Tensor tv0,
    torch::Tensor tv1,
    int64_t win_lo,
    int64_t win_hi,
    int64_t ts_none,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_v0,
    torch::Tensor out_v1,
    torch::Tensor out_t0,
    torch::Tensor out_t1,
    torch::Tensor out_mask,
    torch::Tensor out_n) {
  const torch::Tensor* live[] = {&tts0, &tts1, &tv0, &tv1};
  check_wjoin_table(tkeys, live, 4);
  int64_t nslots = tkeys.numel();
  check_dev(out_keys, torch::kInt32, "out_keys");
  check_dev(out_wins, torch::kInt32, "out_wins");
  check_dev(out_mask, torch::kInt32, "out_mask");
  check_dev(out_n, torch::kInt32, "out_n");
  TORCH_CHECK(out_n.numel() >= 1, "out_n must hold one element");
  int64_t cap = out_keys.numel();
  TORCH_CHECK(out_wins.numel() == cap && out_mask.numel() == cap,
              "output size mismatch");
  const torch::Tensor* outs[] = {&out_v0, &out_v1, &out_t0, &out_t1};
  for (const torch::Tensor* t : outs) {
    check_dev(*t, torch::kInt64, "window join output column");
    TORCH_CHECK(t->numel() == cap, "output size mismatch");
  }
  hipLaunchKernelGGL(
      k_wjoin_extract, dim3(n_blocks(nslots, 256)), dim3(256), 0,
      at::hip::getCurrentHIPStream(),
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const long long*)tts0.data_ptr<int64_t>(),
      (const long long*)tts1.data_ptr<int64_t>(),
      (const long long*)tv0.data_ptr<int64_t>(),
      (const long long*)tv1.data_ptr<int64_t>(), nslots, win_lo, win_hi,
      (long long)ts_none, out_keys.data_ptr<int32_t>(),
      out_wins.data_ptr<int32_t>(), out_v0.data_ptr<int64_t>(),
      out_v1.data_ptr<int64_t>(), out_t0.data_ptr<int64_t>(),
      out_t1.data_ptr<int64_t>(), out_mask.data_ptr<int32_t>(),
      out_n.data_ptr<int32_t>(), cap);
}

// Checks shared by the two passes of the sliding join close; returns
// the grid.  `max_blocks` (0: the usual cap) lets a caller force the
// grid stride on a small table.
static unsigned check_wjoin_pane_close(
    const torch::Tensor& tkeys, const torch::Tensor& fkeys,
    const torch::Tensor* const* fcols, int64_t panes_per_window,
    int64_t panes_per_offset, const torch::Tensor& error_flag,
    int64_t max_blocks) {
  check_wjoin_table(fkeys, fcols, 4);
  TORCH_CHECK(fkeys.data_ptr() != tkeys.data_ptr(),
              "the pane table and the fold table must be distinct");
  check_dev(error_flag, torch::kInt32, "error_flag");
  TORCH_CHECK(error_flag.numel() >= 1, "error_flag must hold one element");
  TORCH_CHECK(panes_per_offset >= 1 && panes_per_window >= panes_per_offset &&
                  panes_per_window <= 64,
              "need 1 <= panes per offset <= panes per window <= 64");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must not be negative");
  int64_t cap = max_blocks > 0 && max_blocks < CM_MAX_GRID ? max_blocks
                                                           : CM_MAX_GRID;
  int64_t nchunks = (tkeys.numel() + CM_CHUNK - 1) / CM_CHUNK;
  return (unsigned)(nchunks < cap ? nchunks : cap);
}

// Stamp pass of the sliding join close (see k_wjoin_pane_stamp): folds
// the stamps of the panes of the windows in [win_lo, win_hi) into the
// fold table `f*` and migrates the panes at or above `pane_keep` into
// the fresh table `n*`.  wjoin_pane_commit has to follow on the stream.
void wjoin_pane_stamp(
    torch::Tensor tkeys,
    torch::Tensor tts0,
    torch::Tensor tts1,
    torch::Tensor tv0,
    torch::Tensor tv1,
    torch::Tensor nkeys,
    torch::Tensor nts0,
    torch::Tensor nts1,
    torch::Tensor nv0,
    torch::Tensor nv1,
    torch::Tensor fkeys,
    torch::Tensor fts0,
    torch::Tensor fts1,
    torch::Tensor fv0,
    torch::Tensor fv1,
    int64_t win_lo,
    int64_t win_hi,
    int64_t pane_keep,
    int64_t panes_per_window,
    int64_t panes_per_offset,
    bool first,
    torch::Tensor error_flag,
    int64_t max_blocks) {
  const torch::Tensor* live[] = {&tts0, &tts1, &tv0, &tv1};
  const torch::Tensor* fresh[] = {&nts0, &nts1, &nv0, &nv1};
  const torch::Tensor* fold[] = {&fts0, &fts1, &fv0, &fv1};
  check_wjoin_table(tkeys, live, 4);
  check_wjoin_table(nkeys, fresh, 4);
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nkeys.numel() == nslots, "table size mismatch");
  TORCH_CHECK(nkeys.data_ptr() != tkeys.data_ptr() &&
                  fkeys.data_ptr() != nkeys.data_ptr(),
              "the three tables must be distinct");
  unsigned grid = check_wjoin_pane_close(
      tkeys, fkeys, fold, panes_per_window, panes_per_offset, error_flag,
      max_blocks);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(
        kernel, dim3(grid), dim3(CM_BLK), 0, at::hip::getCurrentHIPStream(),
        (const uint64_t*)tkeys.data_ptr<int64_t>(),
        (const long long*)tts0.data_ptr<int64_t>(),
        (const long long*)tts1.data_ptr<int64_t>(),
        (const long long*)tv0.data_ptr<int64_t>(),
        (const long long*)tv1.data_ptr<int64_t>(), nslots, win_lo, win_hi,
        pane_keep, panes_per_window, panes_per_offset,
        (uint64_t*)nkeys.data_ptr<int64_t>(),
        (long long*)nts0.data_ptr<int64_t>(),
        (long long*)nts1.data_ptr<int64_t>(),
        (long long*)nv0.data_ptr<int64_t>(),
        (long long*)nv1.data_ptr<int64_t>(), (uint64_t)(nslots - 1),
        (uint64_t*)fkeys.data_ptr<int64_t>(),
        (long long*)fts0.data_ptr<int64_t>(),
        (long long*)fts1.data_ptr<int64_t>(),
        (uint64_t)(fkeys.numel() - 1), error_flag.data_ptr<int32_t>());
  };
  if (first) {
    launch(k_wjoin_pane_stamp<true>);
  } else {
    launch(k_wjoin_pane_stamp<false>);
  }
}

// Commit pass of the sliding join close (see k_wjoin_pane_commit), over
// the pane table wjoin_pane_stamp has just read, with the same window
// range and geometry.
void wjoin_pane_commit(
    torch::Tensor tkeys,
    torch::Tensor tts0,
    torch::Tensor tts1,
    torch::Tensor tv0,
    torch::Tensor tv1,
    torch::Tensor fkeys,
    torch::Tensor fts0,
    torch::Tensor fts1,
    torch::Tensor fv0,
    torch::Tensor fv1,
    int64_t win_lo,
    int64_t win_hi,
    int64_t panes_per_window,
    int64_t panes_per_offset,
    bool first,
    torch::Tensor error_flag,
    int64_t max_blocks) {
  const torch::Tensor* live[] = {&tts0, &tts1, &tv0, &tv1};
  const torch::Tensor* fold[] = {&fts0, &fts1, &fv0, &fv1};
  check_wjoin_table(tkeys, live, 4);
  unsigned grid = check_wjoin_pane_close(
      tkeys, fkeys, fold, panes_per_window, panes_per_offset, error_flag,
      max_blocks);
  hipLaunchKernelGGL(
      k_wjoin_pane_commit, dim3(grid), dim3(CM_BLK), 0,
      at::hip::getCurrentHIPStream(),
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const long long*)tts0.data_ptr<int64_t>(),
      (const long long*)tts1.data_ptr<int64_t>(),
      (const long long*)tv0.data_ptr<int64_t>(),
      (const long long*)tv1.data_ptr<int64_t>(), tkeys.numel(), win_lo,
      win_hi, panes_per_window, panes_per_offset,
      (long long)(first ? INT64_MAX : INT64_MIN),
      (const uint64_t*)fkeys.data_ptr<int64_t>(),
      (const long long*)fts0.data_ptr<int64_t>(),
      (const long long*)fts1.data_ptr<int64_t>(),
      (long long*)fv0.data_ptr<int64_t>(),
      (long long*)fv1.data_ptr<int64_t>(), (uint64_t)(fkeys.numel() - 1),
      error_flag.data_ptr<int32_t>());
}

// Checks of one product-join table and one side's log; returns the
// log's capacity in entries.  `log` is int64 [2 * capacity]: 16-byte
// entries (packed cell word, value).  `log_n` is the int32 cursor pair
// of the two sides.
static int64_t check_wjprod(
    const torch::Tensor& tkeys, const torch::Tensor& tcnt,
    const torch::Tensor& log, const torch::Tensor& log_n, int64_t side) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(tcnt, torch::kInt32, "tcnt");
  check_dev(log, torch::kInt64, "log");
  check_dev(log_n, torch::kInt32, "log_n");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nslots > 0 && (nslots & (nslots - 1)) == 0,
              "table size must be a power of two");
  // slot_cell holds list indices below nslots as int32.
  TORCH_CHECK(nslots <= (int64_t)1 << 30, "table too large");
  TORCH_CHECK(tcnt.numel() == 2 * nslots, "table size mismatch");
  TORCH_CHECK(side == 0 || side == 1, "side must be 0 or 1");
  TORCH_CHECK(log_n.numel() == 2, "log_n must hold one cursor per side");
  TORCH_CHECK(log.numel() % 2 == 0, "log must hold whole entries");
  // The cursor is an int32.
  TORCH_CHECK(log.numel() / 2 < (int64_t)INT32_MAX, "log too large");
  TORCH_CHECK((((uintptr_t)log.data_ptr()) & 15) == 0 &&
                  (((uintptr_t)tcnt.data_ptr()) & 7) == 0,
              "log and counts must be 16- and 8-byte aligned");
  return log.numel() / 2;
}

// One side's batch into the product-join table and the side's log (see
// k_wjprod_insert): one launch.  The caller guarantees that the log
// has room for the batch.  `ts` is absolute int64 or int32 deltas
// against `ts_base`.
void wjprod_insert(
    torch::Tensor keys,
    torch::Tensor ts,
    torch::Tensor vals,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor log,
    torch::Tensor log_n,
    int64_t side,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t align_ms,
    int64_t len_ms,
    int64_t ts_base) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(vals, torch::kInt64, "vals");
  check_dev(max_ts, torch::kInt64, "max_ts");
  check_dev(error_flag, torch::kInt32, "error_flag");
  const bool ts32 = ts.scalar_type() == torch::kInt32;
  check_dev(ts, ts32 ? torch::kInt32 : torch::kInt64, "ts");
  int64_t log_cap = check_wjprod(tkeys, tcnt, log, log_n, side);
  int64_t n = keys.numel();
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(ts.numel() == n && vals.numel() == n, "column size mismatch");
  TORCH_CHECK(len_ms > 0, "window length must be positive");
  TORCH_CHECK(max_ts.numel() >= 1 && error_flag.numel() >= 1,
              "max_ts and error_flag must hold one element");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  auto run = [&](auto* tsp) {
    using TSV = std::remove_cv_t<std::remove_pointer_t<decltype(tsp)>>;
    hipLaunchKernelGGL(
        k_wjprod_insert<TSV>, dim3(n_blocks(n, 256)), dim3(256), 0, stream,
        keys.data_ptr<int32_t>(), tsp,
        (const int64_t*)vals.data_ptr<int64_t>(), n,
        (uint64_t*)tkeys.data_ptr<int64_t>(), tcnt.data_ptr<int32_t>(),
        (uint64_t)(nslots - 1), (int)side,
        (ulonglong2*)log.data_ptr<int64_t>(),
        log_n.data_ptr<int32_t>() + side, log_cap, align_ms, len_ms, ts_base,
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>());
  };
  if (ts32)
    run((const int32_t*)ts.data_ptr<int32_t>());
  else
    run((const int64_t*)ts.data_ptr<int64_t>());
}

// Plan pass of the product-join close (see k_wjprod_plan): lists the
// cells of [win_lo, win_hi) into `cell_pk` / `cell_n` (nslots and
// 2 * nslots long) and counts them in `cells_n`, which the caller has
// zeroed.
void wjprod_plan(
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    int64_t win_lo,
    int64_t win_hi,
    torch::Tensor cell_pk,
    torch::Tensor cell_n,
    torch::Tensor slot_cell,
    torch::Tensor cells_n) {
  check_dev(tkeys, torch::kInt64, "tkeys");
  check_dev(tcnt, torch::kInt32, "tcnt");
  check_dev(cell_pk, torch::kInt64, "cell_pk");
  check_dev(cell_n, torch::kInt32, "cell_n");
  check_dev(slot_cell, torch::kInt32, "slot_cell");
  check_dev(cells_n, torch::kInt32, "cells_n");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nslots > 0 && (nslots & (nslots - 1)) == 0,
              "table size must be a power of two");
  TORCH_CHECK(nslots <= (int64_t)1 << 30, "table too large");
  TORCH_CHECK(tcnt.numel() == 2 * nslots && cell_pk.numel() == nslots &&
                  cell_n.numel() == 2 * nslots &&
                  slot_cell.numel() == nslots && cells_n.numel() >= 1,
              "table size mismatch");
  TORCH_CHECK((((uintptr_t)tcnt.data_ptr()) & 7) == 0 &&
                  (((uintptr_t)cell_n.data_ptr()) & 7) == 0,
              "counts must be 8-byte aligned");
  int64_t nchunks = (nslots + CM_CHUNK - 1) / CM_CHUNK;
  unsigned grid = (unsigned)(nchunks < CM_MAX_GRID ? nchunks : CM_MAX_GRID);
  hipLaunchKernelGGL(
      k_wjprod_plan, dim3(grid), dim3(CM_BLK), 0,
      at::hip::getCurrentHIPStream(),
      (const uint64_t*)tkeys.data_ptr<int64_t>(),
      (const int*)tcnt.data_ptr<int32_t>(), nslots, win_lo, win_hi,
      (uint64_t*)cell_pk.data_ptr<int64_t>(), cell_n.data_ptr<int32_t>(),
      slot_cell.data_ptr<int32_t>(), cells_n.data_ptr<int32_t>());
}

// Gather pass of the product-join close over the first `n` entries of
// one side's log (see k_wjprod_gather).  `ncells` is the plan's count,
// `val_end` the inclusive prefix sums of n0 + n1 over its list and
// `arena` at least val_end[ncells - 1] long.  `n*` is the fresh state:
// an empty table, and logs with empty cursors at the call for side 0.
void wjprod_gather(
    torch::Tensor log,
    int64_t n,
    int64_t side,
    torch::Tensor tkeys,
    torch::Tensor tcnt,
    torch::Tensor log_n,
    int64_t win_lo,
    int64_t win_hi,
    torch::Tensor slot_cell,
    torch::Tensor cell_n,
    torch::Tensor val_end,
    int64_t ncells,
    torch::Tensor arena,
    torch::Tensor nkeys,
    torch::Tensor ncnt,
    torch::Tensor nlog,
    torch::Tensor nlog_n,
    torch::Tensor error_flag) {
  int64_t log_cap = check_wjprod(tkeys, tcnt, log, log_n, side);
  int64_t nlog_cap = check_wjprod(nkeys, ncnt, nlog, nlog_n, side);
  int64_t nslots = tkeys.numel();
  TORCH_CHECK(nkeys.numel() == nslots, "table size mismatch");
  check_dev(slot_cell, torch::kInt32, "slot_cell");
  check_dev(cell_n, torch::kInt32, "cell_n");
  check_dev(val_end, torch::kInt64, "val_end");
  check_dev(arena, torch::kInt64, "arena");
  check_dev(error_flag, torch::kInt32, "error_flag");
  TORCH_CHECK(error_flag.numel() >= 1, "error_flag must hold one element");
  TORCH_CHECK(n >= 0 && n <= log_cap, "more entries than the log holds");
  // Every migrated entry has a place.
  TORCH_CHECK(nlog_cap >= n, "fresh log smaller than the live entries");
  TORCH_CHECK(ncells >= 0 && ncells <= nslots && slot_cell.numel() == nslots &&
                  cell_n.numel() >= 2 * ncells && val_end.numel() >= ncells,
              "plan size mismatch");
  if (n == 0) return;
  hipLaunchKernelGGL(
      k_wjprod_gather, dim3(n_blocks(n, 256)), dim3(256), 0,
      at::hip::getCurrentHIPStream(),
      (const ulonglong2*)log.data_ptr<int64_t>(), n, (int)side,
      (const uint64_t*)tkeys.data_ptr<int64_t>(), tcnt.data_ptr<int32_t>(),
      (uint64_t)(nslots - 1), win_lo, win_hi,
      (const int*)slot_cell.data_ptr<int32_t>(),
      (const int*)cell_n.data_ptr<int32_t>(),
      (const int64_t*)val_end.data_ptr<int64_t>(), ncells,
      arena.data_ptr<int64_t>(), arena.numel(),
      (uint64_t*)nkeys.data_ptr<int64_t>(), ncnt.data_ptr<int32_t>(),
      (ulonglong2*)nlog.data_ptr<int64_t>(),
      nlog_n.data_ptr<int32_t>() + side, nlog_cap,
      error_flag.data_ptr<int32_t>());
}

// Expand pass of the product-join close (see k_wjprod_expand): the
// `nrows` rows of the plan's `ncells` cells into output columns of
// exactly that length.  `row_end` is the inclusive prefix sum of
// max(n0, 1) * max(n1, 1) over the list, `row_end[ncells - 1] ==
// nrows`.
void wjprod_expand(
    int64_t nrows,
    int64_t ncells,
    torch::Tensor row_end,
    torch::Tensor val_end,
    torch::Tensor cell_pk,
    torch::Tensor cell_n,
    torch::Tensor arena,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_v0,
    torch::Tensor out_v1,
    torch::Tensor out_mask) {
  check_dev(row_end, torch::kInt64, "row_end");
  check_dev(val_end, torch::kInt64, "val_end");
  check_dev(cell_pk, torch::kInt64, "cell_pk");
  check_dev(cell_n, torch::kInt32, "cell_n");
  check_dev(arena, torch::kInt64, "arena");
  check_dev(out_keys, torch::kInt32, "out_keys");
  check_dev(out_wins, torch::kInt32, "out_wins");
  check_dev(out_mask, torch::kInt32, "out_mask");
  check_dev(out_v0, torch::kInt64, "out_v0");
  check_dev(out_v1, torch::kInt64, "out_v1");
  TORCH_CHECK(nrows >= 0 && ncells >= 0 && (nrows == 0 || ncells > 0),
              "rows without cells");
  TORCH_CHECK(row_end.numel() >= ncells && val_end.numel() >= ncells &&
                  cell_pk.numel() >= ncells && cell_n.numel() >= 2 * ncells,
              "plan size mismatch");
  TORCH_CHECK(out_keys.numel() == nrows && out_wins.numel() == nrows &&
                  out_mask.numel() == nrows && out_v0.numel() == nrows &&
                  out_v1.numel() == nrows,
              "output size mismatch");
  if (nrows == 0) return;
  hipLaunchKernelGGL(
      k_wjprod_expand, dim3(n_blocks(nrows, 256)), dim3(256), 0,
      at::hip::getCurrentHIPStream(), nrows, ncells,
      (const int64_t*)row_end.data_ptr<int64_t>(),
      (const int64_t*)val_end.data_ptr<int64_t>(),
      (const uint64_t*)cell_pk.data_ptr<int64_t>(),
      (const int*)cell_n.data_ptr<int32_t>(),
      (const int64_t*)arena.data_ptr<int64_t>(),
      out_keys.data_ptr<int32_t>(), out_wins.data_ptr<int32_t>(),
      out_v0.data_ptr<int64_t>(), out_v1.data_ptr<int64_t>(),
      out_mask.data_ptr<int32_t>());
}

int64_t filter_compact(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    torch::Tensor mask,
    torch::Tensor out_keys,
    torch::Tensor out_ts,
    torch::Tensor out_vals,
    torch::Tensor out_n) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(ts, torch::kInt64, "ts");
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8 ||
                  mask.scalar_type() == torch::kBool,
              "mask must be bool/uint8");
  int64_t n = keys.numel();
  if (n == 0) return 0;
  const int64_t* vptr = nullptr;
  if (vals.has_value()) vptr = vals->data_ptr<int64_t>();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  hipLaunchKernelGGL(
      k_filter_compact, grid, block, 0, stream, keys.data_ptr<int32_t>(),
      ts.data_ptr<int64_t>(), vptr, (const uint8_t*)mask.data_ptr(), n,
      out_keys.data_ptr<int32_t>(), out_ts.data_ptr<int64_t>(),
      out_vals.data_ptr<int64_t>(), out_n.data_ptr<int32_t>());
  return 0;
}

void bucket_hist(torch::Tensor keys, int64_t world, torch::Tensor counts) {
  check_dev(keys, torch::kInt32, "keys");
  check_dev(counts, torch::kInt32, "counts");
  int64_t n = keys.numel();
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  hipLaunchKernelGGL(
      k_bucket_hist, grid, block, (int)(world * sizeof(int)), stream,
      keys.data_ptr<int32_t>(), n, (int)world, counts.data_ptr<int32_t>());
}

void bucket_scatter(
    torch::Tensor keys,
    torch::Tensor ts,
    c10::optional<torch::Tensor> vals,
    int64_t world,
    torch::Tensor cursors,
    torch::Tensor out_keys,
    torch::Tensor out_ts,
    torch::Tensor out_vals) {
  check_dev(keys, torch::kInt32, "keys");
  bool ts32 = ts.scalar_type() == torch::kInt32;
  if (!ts32) check_dev(ts, torch::kInt64, "ts");
  TORCH_CHECK(out_ts.scalar_type() == ts.scalar_type(),
              "out_ts dtype must match ts");
  check_dev(cursors, torch::kInt32, "cursors");
  int64_t n = keys.numel();
  if (n == 0) return;
  const int64_t* vptr = nullptr;
  if (vals.has_value()) {
    check_dev(*vals, torch::kInt64, "vals");
    vptr = vals->data_ptr<int64_t>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  if (ts32) {
    hipLaunchKernelGGL(
        k_bucket_scatter<int32_t>, grid, block, 0, stream,
        keys.data_ptr<int32_t>(), ts.data_ptr<int32_t>(), vptr, n,
        (int)world, cursors.data_ptr<int32_t>(),
        out_keys.data_ptr<int32_t>(), out_ts.data_ptr<int32_t>(),
        out_vals.data_ptr<int64_t>());
  } else {
    hipLaunchKernelGGL(
        k_bucket_scatter<int64_t>, grid, block, 0, stream,
        keys.data_ptr<int32_t>(), ts.data_ptr<int64_t>(), vptr, n,
        (int)world, cursors.data_ptr<int32_t>(),
        out_keys.data_ptr<int32_t>(), out_ts.data_ptr<int64_t>(),
        out_vals.data_ptr<int64_t>());
  }
}

// ---------------------------------------------------------------------------
// Native step-loop executor: runs the steady-state columnar window
// pipeline (source batch -> fused insert -> watermark close) for a
// whole run of steps with NO Python between steps.  This is the role
// the reference's Rust `step_or_park` worker loop plays
// (reference src/worker.rs:68-83), specialized for the device path:
// the host thread is just a kernel-launch engine on one HIP stream.
// Returns the total number of closed-window rows; per-step host
// launch timestamps (ns) are written into `step_ns_out` for latency
// percentiles.  The GIL is released for the duration.
// ---------------------------------------------------------------------------

int64_t native_run_window_steps(
    std::vector<torch::Tensor> key_pool,
    std::vector<torch::Tensor> ts_pool,
    int64_t start_step,
    int64_t n_steps,
    int64_t sim_ms_per_batch,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t wait_ms,
    int64_t mode,
    bool dedup,
    int64_t closed_horizon_in,
    torch::Tensor step_ns_out,  // int64 CPU tensor [n_steps]
    // int64 CPU tensor [3]: closed_horizon, rows, table-swap parity
    torch::Tensor state_out,
    int64_t region_bits,
    bool use_radix,
    c10::optional<torch::Tensor> gcursors,
    c10::optional<torch::Tensor> ev_packed,
    c10::optional<torch::Tensor> ev_vals,
    c10::optional<torch::Tensor> ov_cursor,
    c10::optional<torch::Tensor> ov_packed,
    c10::optional<torch::Tensor> ov_vals,
    torch::Tensor alt_tkeys,
    torch::Tensor alt_tvals,
    bool use_radix_v2,
    c10::optional<torch::Tensor> v2_gcur,
    c10::optional<torch::Tensor> v2_gres,
    c10::optional<torch::Tensor> v2_ev,
    c10::optional<torch::Tensor> v2_ev_res,
    bool pipelined = false,
    c10::optional<torch::Tensor> gcursors2 = c10::nullopt,
    c10::optional<torch::Tensor> ev_packed2 = c10::nullopt,
    c10::optional<torch::Tensor> ov_cursor2 = c10::nullopt,
    c10::optional<torch::Tensor> ov_packed2 = c10::nullopt) {
  TORCH_CHECK(!key_pool.empty(), "empty key pool");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  int64_t n = key_pool[0].numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  int64_t* step_ns =
      step_ns_out.numel() >= n_steps ? step_ns_out.data_ptr<int64_t>()
                                     : nullptr;

  int64_t closed_horizon = closed_horizon_in;
  int64_t total_rows = 0;
  int pool = (int)key_pool.size();
  // Double-buffered tables: close = emit + migrate live cells into the
  // (pre-reset) alternate table, then swap and reset the old one.
  torch::Tensor cur_k = tkeys, cur_v = tvals;
  torch::Tensor alt_k = alt_tkeys, alt_v = alt_tvals;
  int swap_parity = 0;

  // Pinned host scalar for the close-count readback.
  int* h_n = nullptr;
  HIP_CHECK(hipHostMalloc((void**)&h_n, sizeof(int), hipHostMallocDefault));

  // Pipelined radix: the scatter of step N+1 runs on its own stream,
  // into the OTHER of two region-buffer sets, while the aggregation
  // of step N drains the first on the main stream — the ~0.4 ms agg
  // hides entirely behind the ~1.4 ms scatter.  Events serialize
  // scatter(N)->agg(N) and agg(N)->scatter(N+2) (buffer reuse).
  bool pipe = pipelined && use_radix && !use_radix_v2 &&
              gcursors2.has_value();
  hipStream_t sc_stream = nullptr;
  hipEvent_t ev_sc[2] = {nullptr, nullptr};
  hipEvent_t ev_ag[2] = {nullptr, nullptr};
  int64_t nb = 0, cap = 0, nseg = 0;
  int seg_bits = (int)region_bits;
  ScatterKind kind = SCAT_FIXED;
  size_t staged_lds = 0;
  uint64_t mask = (uint64_t)(nslots - 1);
  uint64_t win_m2 = 0, win_maxfast = 0;
  if (pipe) {
    nb = nslots >> region_bits;
    TORCH_CHECK(ev_packed2->numel() == ev_packed->numel(),
                "pipelined scatter buffers must match");
    magic_div_u64(len_ms, &win_m2, &win_maxfast);
    // Same scatter-variant/segmentation decision as radix_window_insert
    // (COUNT mode here).
    kind = scatter_kind_env();
    int coarse = scatter_coarse_bits(kind);
    seg_bits = (int)region_bits + coarse;
    nseg = nslots >> seg_bits;
    staged_lds =
        (size_t)nseg * SC_GRAN * 8 + 4 * (size_t)nseg * sizeof(int);
    while (kind == SCAT_STAGED &&
           (nseg < 1 || staged_lds > 160 * 1024 || seg_bits > 13)) {
      if (coarse > 0 && seg_bits > 13) {
        coarse -= 1;
      } else {
        kind = SCAT_FIXED;
        coarse = 0;
      }
      seg_bits = (int)region_bits + coarse;
      nseg = nslots >> seg_bits;
      staged_lds =
          (size_t)nseg * SC_GRAN * 8 + 4 * (size_t)nseg * sizeof(int);
    }
    if (seg_bits > 13) {
      seg_bits = (int)region_bits;
      nseg = nb;
    }
    cap = ev_packed->numel() / nseg;
    if (kind == SCAT_STAGED) {
      cap &= ~(int64_t)(SC_GRAN - 1);
      if (cap < SC_GRAN) {
        kind = SCAT_FIXED;
        seg_bits = (int)region_bits;
        nseg = nb;
        cap = ev_packed->numel() / nseg;
      }
    }
    HIP_CHECK(hipStreamCreateWithFlags(&sc_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      HIP_CHECK(hipEventCreateWithFlags(&ev_sc[i], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&ev_ag[i], hipEventDisableTiming));
    }
  }

  {
    pybind11::gil_scoped_release release;
    for (int64_t s = 0; s < n_steps; ++s) {
      if (step_ns != nullptr) {
        step_ns[s] = std::chrono::duration_cast<std::chrono::nanoseconds>(
                         std::chrono::steady_clock::now().time_since_epoch())
                         .count();
      }
      int64_t step = start_step + s;
      auto& keys = key_pool[step % pool];
      auto& ts = ts_pool[step % pool];
      int64_t base = align_ms + step * sim_ms_per_batch;
      if (use_radix_v2) {
        radix_v2_window_insert(
            keys, ts, cur_k, cur_v, max_ts, error_flag, *v2_gcur,
            *v2_gres, *v2_ev, *v2_ev_res, align_ms, len_ms, base,
            region_bits);
      } else if (pipe) {
        int par = (int)(step & 1);
        torch::Tensor& gcur = par ? *gcursors2 : *gcursors;
        torch::Tensor& evp = par ? *ev_packed2 : *ev_packed;
        torch::Tensor& ovc = par ? *ov_cursor2 : *ov_cursor;
        torch::Tensor& ovp = par ? *ov_packed2 : *ov_packed;
        if (s >= 2) {
          // Buffer reuse: the agg that read this parity's buffers two
          // steps ago must have drained them.
          HIP_CHECK(hipStreamWaitEvent(sc_stream, ev_ag[par], 0));
        }
        HIP_CHECK(hipMemsetAsync(
            gcur.data_ptr<int32_t>(), 0, (size_t)nseg * sizeof(int),
            sc_stream));
        HIP_CHECK(hipMemsetAsync(
            ovc.data_ptr<int32_t>(), 0, sizeof(int), sc_stream));
        // One scatter call per step: its own entry base.
        const CountEntries ce = plan_count_entries(
            kind == SCAT_STAGED, 1, evp.data_ptr<int64_t>(), nseg, cap,
            seg_bits, ts.scalar_type() == torch::kInt32, align_ms, len_ms,
            base);
        auto scat_step = [&](auto tsptr) {
          using TSV =
              std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
          if (kind == SCAT_STAGED) {
            launch_count_staged<TSV>(
                sc_stream, keys.data_ptr<int32_t>(), tsptr, n, 1, align_ms,
                len_ms, len_ms, base, mask, seg_bits, nseg, cap,
                gcur.data_ptr<int32_t>(), (uint64_t*)evp.data_ptr<int64_t>(),
                ovc.data_ptr<int32_t>(), (uint64_t*)ovp.data_ptr<int64_t>(),
                ovp.numel(), (unsigned long long*)max_ts.data_ptr<int64_t>(),
                error_flag.data_ptr<int32_t>(), win_m2, win_maxfast,
                /*overlapped=*/true, ce);
          } else if (kind == SCAT_DIRECT) {
            hipLaunchKernelGGL(
                (k_radix_scatter_direct<AGG_COUNT, TSV>), grid, block, 0,
                sc_stream, keys.data_ptr<int32_t>(), tsptr,
                (const int64_t*)nullptr, n, align_ms, len_ms, len_ms, base,
                mask,
                seg_bits, cap, gcur.data_ptr<int32_t>(),
                (uint64_t*)evp.data_ptr<int64_t>(), (int64_t*)nullptr,
                ovc.data_ptr<int32_t>(), (uint64_t*)ovp.data_ptr<int64_t>(),
                (int64_t*)nullptr, ovp.numel(),
                (unsigned long long*)max_ts.data_ptr<int64_t>(),
                error_flag.data_ptr<int32_t>(), win_m2, win_maxfast);
          } else {
            size_t hist_lds = (size_t)nseg * sizeof(int);
            hipLaunchKernelGGL(
                (k_radix_scatter_fixed<AGG_COUNT, TSV>), grid, block,
                2 * hist_lds,
                sc_stream, keys.data_ptr<int32_t>(), tsptr,
                (const int64_t*)nullptr, n, align_ms, len_ms, len_ms, base, mask,
                seg_bits, cap, gcur.data_ptr<int32_t>(),
                (uint64_t*)evp.data_ptr<int64_t>(), (int64_t*)nullptr,
                ovc.data_ptr<int32_t>(), (uint64_t*)ovp.data_ptr<int64_t>(),
                (int64_t*)nullptr, ovp.numel(),
                (unsigned long long*)max_ts.data_ptr<int64_t>(),
                error_flag.data_ptr<int32_t>(), win_m2, win_maxfast,
                NO_LATE_ARGS);
          }
        };
        if (ts.scalar_type() == torch::kInt32)
          scat_step(ts.data_ptr<int32_t>());
        else scat_step(ts.data_ptr<int64_t>());
        HIP_CHECK(hipEventRecord(ev_sc[par], sc_stream));
        HIP_CHECK(hipStreamWaitEvent(stream, ev_sc[par], 0));
        launch_count_agg(
            stream, (const uint64_t*)evp.data_ptr<int64_t>(),
            gcur.data_ptr<int32_t>(), cap,
            (uint64_t*)cur_k.data_ptr<int64_t>(),
            (unsigned long long*)cur_v.data_ptr<int64_t>(), mask,
            (int)region_bits, seg_bits, nseg,
            error_flag.data_ptr<int32_t>(), ce.agg_w(), ce.fmt());
        hipLaunchKernelGGL(
            k_overflow_agg<AGG_COUNT>, overflow_agg_grid(), block, 0, stream,
            (const uint64_t*)ovp.data_ptr<int64_t>(),
            (const int64_t*)nullptr, ovc.data_ptr<int32_t>(), ovp.numel(),
            (uint64_t*)cur_k.data_ptr<int64_t>(),
            (unsigned long long*)cur_v.data_ptr<int64_t>(), mask,
            (int)region_bits, error_flag.data_ptr<int32_t>(),
            (unsigned long long*)nullptr);
        HIP_CHECK(hipEventRecord(ev_ag[par], stream));
      } else if (use_radix) {
        radix_window_insert(
            keys, ts, c10::nullopt, cur_k, cur_v, max_ts, error_flag,
            *gcursors, *ev_packed, *ev_vals, *ov_cursor, *ov_packed,
            *ov_vals, align_ms, len_ms, AGG_COUNT, base, region_bits);
      } else {
        auto launch = [&](auto kern, auto tsptr) {
          hipLaunchKernelGGL(
              kern, grid, block, 0, stream, keys.data_ptr<int32_t>(),
              tsptr, (const int64_t*)nullptr, n,
              (uint64_t*)cur_k.data_ptr<int64_t>(),
              (unsigned long long*)cur_v.data_ptr<int64_t>(),
              (uint64_t)(nslots - 1), align_ms, len_ms, len_ms, base,
              (int)region_bits,
              (unsigned long long*)max_ts.data_ptr<int64_t>(),
              error_flag.data_ptr<int32_t>(), (const int64_t*)nullptr,
              NO_LATE_ARGS);
        };
        auto disp = [&](auto tsptr) {
          using TSV =
              std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
          if (dedup)
            launch(k_window_agg_insert<AGG_COUNT, true, TSV>, tsptr);
          else launch(k_window_agg_insert<AGG_COUNT, false, TSV>, tsptr);
        };
        if (ts.scalar_type() == torch::kInt32)
          disp(ts.data_ptr<int32_t>());
        else disp(ts.data_ptr<int64_t>());
      }

      int64_t wm = base + sim_ms_per_batch - 1;
      int64_t horizon = (wm - wait_ms - align_ms) / len_ms;
      if (horizon > closed_horizon) {
        HIP_CHECK(hipMemsetAsync(out_n.data_ptr<int32_t>(), 0, sizeof(int), stream));
        launch_close_migrate(
            stream, cur_k, cur_v, horizon, alt_k, alt_v, region_bits,
            out_keys, out_wins, out_vals, out_n, error_flag);
        HIP_CHECK(hipMemcpyAsync(h_n, out_n.data_ptr<int32_t>(), sizeof(int),
                       hipMemcpyDeviceToHost, stream));
        std::swap(cur_k, alt_k);
        std::swap(cur_v, alt_v);
        swap_parity ^= 1;
        // Reset the retired table asynchronously for the next close.
        HIP_CHECK(hipMemsetAsync(alt_k.data_ptr<int64_t>(), 0xFF,
                                 (size_t)nslots * 8, stream));
        HIP_CHECK(hipMemsetAsync(alt_v.data_ptr<int64_t>(), 0,
                                 (size_t)nslots * 8, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        total_rows += *h_n;
        closed_horizon = horizon;
      }
    }
    if (sc_stream != nullptr) {
      HIP_CHECK(hipStreamSynchronize(sc_stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  if (sc_stream != nullptr) {
    for (int i = 0; i < 2; ++i) {
      HIP_CHECK(hipEventDestroy(ev_sc[i]));
      HIP_CHECK(hipEventDestroy(ev_ag[i]));
    }
    HIP_CHECK(hipStreamDestroy(sc_stream));
  }
  HIP_CHECK(hipHostFree(h_n));
  auto* st = state_out.data_ptr<int64_t>();
  st[0] = closed_horizon;
  st[1] = total_rows;
  st[2] = swap_parity;
  return total_rows;
}

// hipGraph variant of the native step loop: one pool cycle of
// {insert, ts-bump} kernels is captured once and replayed per group —
// the host cost of a whole pool of steps collapses to one
// hipGraphLaunch.  Timestamps advance via the device-side offset
// scalar so the captured graph stays valid across replays.  Window
// closes happen between replays (their steps are arithmetic).
// COUNT mode, single-pass insert only (the latency-oriented path).
int64_t native_run_window_steps_graph(
    std::vector<torch::Tensor> key_pool,
    std::vector<torch::Tensor> ts_pool,
    int64_t start_step,
    int64_t n_steps,
    int64_t sim_ms_per_batch,
    torch::Tensor tkeys,
    torch::Tensor tvals,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    torch::Tensor out_keys,
    torch::Tensor out_wins,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    int64_t align_ms,
    int64_t len_ms,
    int64_t wait_ms,
    int64_t closed_horizon_in,
    torch::Tensor state_out,  // int64 CPU [3]
    int64_t region_bits,
    torch::Tensor alt_tkeys,
    torch::Tensor alt_tvals,
    torch::Tensor ts_base_dev) {  // int64 device scalar
  TORCH_CHECK(!key_pool.empty(), "empty key pool");
  int64_t nslots = tkeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  int64_t n = key_pool[0].numel();
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  int pool = (int)key_pool.size();
  uint64_t mask = (uint64_t)(nslots - 1);

  // The device offset starts at the first step's base.
  ts_base_dev.fill_(align_ms + start_step * sim_ms_per_batch);

  auto launch_insert_on = [&](int j, hipStream_t st) {
    hipLaunchKernelGGL(
        (k_window_agg_insert<AGG_COUNT, false>), grid, block, 0, st,
        key_pool[j].data_ptr<int32_t>(), ts_pool[j].data_ptr<int64_t>(),
        (const int64_t*)nullptr, n, (uint64_t*)tkeys.data_ptr<int64_t>(),
        (unsigned long long*)tvals.data_ptr<int64_t>(), mask, align_ms,
        len_ms, len_ms, 0, (int)region_bits,
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(),
        (const int64_t*)ts_base_dev.data_ptr<int64_t>(), NO_LATE_ARGS);
    hipLaunchKernelGGL(
        k_bump, dim3(1), dim3(1), 0, st,
        ts_base_dev.data_ptr<int64_t>(), sim_ms_per_batch);
  };
  auto launch_insert = [&](int j) { launch_insert_on(j, stream); };

  // NOTE: inserts always target `tkeys`/`tvals` (the tensors captured
  // into the graph), so closes must migrate live cells back into the
  // SAME tensors — a double swap: cur -> alt -> cur with a reset in
  // between keeps probe-chain hygiene while preserving buffer
  // identity for the graph.
  int64_t closed_horizon = closed_horizon_in;
  int64_t total_rows = 0;
  int* h_n = nullptr;
  HIP_CHECK(hipHostMalloc((void**)&h_n, sizeof(int), hipHostMallocDefault));

  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  {
    pybind11::gil_scoped_release release;
    // Capture must happen on a non-default stream; the replays run on
    // the torch stream.
    hipStream_t cs = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    for (int j = 0; j < pool; ++j) launch_insert_on(j, cs);
    HIP_CHECK(hipStreamEndCapture(cs, &graph));
    HIP_CHECK(hipStreamDestroy(cs));
    HIP_CHECK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));

    auto horizon_after = [&](int64_t step) {
      int64_t wm = align_ms + (step + 1) * sim_ms_per_batch - 1;
      return (wm - wait_ms - align_ms) / len_ms;
    };
    auto do_close = [&](int64_t horizon) {
      HIP_CHECK(hipMemsetAsync(out_n.data_ptr<int32_t>(), 0, sizeof(int),
                               stream));
      // Migrate live cells out and back so the graph's captured table
      // pointers stay authoritative.
      launch_close_migrate(
          stream, tkeys, tvals, horizon, alt_tkeys, alt_tvals, region_bits,
          out_keys, out_wins, out_vals, out_n, error_flag);
      HIP_CHECK(hipMemcpyAsync(h_n, out_n.data_ptr<int32_t>(), sizeof(int),
                               hipMemcpyDeviceToHost, stream));
      // Reset the primary and migrate back (no emissions: horizon
      // below everything live now).
      HIP_CHECK(hipMemsetAsync(tkeys.data_ptr<int64_t>(), 0xFF,
                               (size_t)nslots * 8, stream));
      HIP_CHECK(hipMemsetAsync(tvals.data_ptr<int64_t>(), 0,
                               (size_t)nslots * 8, stream));
      launch_close_migrate(
          stream, alt_tkeys, alt_tvals, (int64_t)(-(1LL << 40)), tkeys,
          tvals, region_bits, out_keys, out_wins, out_vals, out_n,
          error_flag);
      HIP_CHECK(hipMemsetAsync(alt_tkeys.data_ptr<int64_t>(), 0xFF,
                               (size_t)nslots * 8, stream));
      HIP_CHECK(hipMemsetAsync(alt_tvals.data_ptr<int64_t>(), 0,
                               (size_t)nslots * 8, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      total_rows += *h_n;
      closed_horizon = horizon;
    };

    int64_t s = 0;
    while (s < n_steps) {
      bool group_ok = (n_steps - s) >= pool &&
                      horizon_after(start_step + s + pool - 1) ==
                          closed_horizon;
      if (group_ok) {
        HIP_CHECK(hipGraphLaunch(gexec, stream));
        s += pool;
      } else {
        launch_insert((int)((start_step + s) % pool));
        int64_t h = horizon_after(start_step + s);
        s += 1;
        if (h > closed_horizon) do_close(h);
      }
    }
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  HIP_CHECK(hipGraphExecDestroy(gexec));
  HIP_CHECK(hipGraphDestroy(graph));
  HIP_CHECK(hipHostFree(h_n));
  auto* st = state_out.data_ptr<int64_t>();
  st[0] = closed_horizon;
  st[1] = total_rows;
  st[2] = 0;  // table identity preserved
  return total_rows;
}

// Fused radix session insert: AGG_TS scatter -> per-segment LDS
// session aggregation -> sequential overflow walk.  One call per
// batch; emissions accumulate in the out buffers until drained.
void session_radix_insert(
    torch::Tensor keys,
    torch::Tensor ts,  // int32 template or int64 absolute
    int64_t ts_base,
    int64_t gap_ms,
    torch::Tensor skeys,
    torch::Tensor sstart,
    torch::Tensor slast,
    torch::Tensor sacc,
    torch::Tensor gcursors,
    torch::Tensor ev_packed,
    torch::Tensor ev_vals,
    torch::Tensor ov_cursor,
    torch::Tensor ov_packed,
    torch::Tensor ov_vals,
    torch::Tensor out_keys,
    torch::Tensor out_start,
    torch::Tensor out_end,
    torch::Tensor out_vals,
    torch::Tensor out_n,
    torch::Tensor max_ts,
    torch::Tensor error_flag,
    int64_t seg_bits) {
  check_dev(keys, torch::kInt32, "keys");
  bool ts32 = ts.scalar_type() == torch::kInt32;
  if (!ts32) check_dev(ts, torch::kInt64, "ts");
  int64_t n = keys.numel();
  int64_t nslots = skeys.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "table size must be 2^k");
  TORCH_CHECK(seg_bits > 0 && seg_bits < 40, "bad seg_bits");
  int64_t nseg = nslots >> seg_bits;
  TORCH_CHECK(nseg >= 1 && nseg <= 8192, "segment count out of range");
  TORCH_CHECK(gcursors.numel() >= nseg, "gcursors too small");
  int64_t cap = ev_packed.numel() / nseg;
  bool staged = true;
  cap &= ~(int64_t)(SC_GRAN - 1);
  if (cap < SC_GRAN) {
    staged = false;
    cap = ev_packed.numel() / nseg;
  }
  TORCH_CHECK(cap * nseg >= 2 * n || cap >= n,
              "session scatter buffers too small");
  TORCH_CHECK(ev_vals.numel() >= nseg * cap, "ev_vals too small");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t mask = (uint64_t)(nslots - 1);
  gcursors.narrow(0, 0, nseg).zero_();
  ov_cursor.zero_();
  uint64_t win_m2, win_maxfast;
  magic_div_u64((int64_t)1 << 40, &win_m2, &win_maxfast);
  size_t staged_lds = (size_t)nseg * SC_GRAN * 8 * 2 +
                      4 * (size_t)nseg * sizeof(int);
  auto scat512 = [&](auto kern, auto tsptr, unsigned gx, size_t lds) {
    hipLaunchKernelGGL(
        kern, dim3(gx), dim3(512), lds, stream,
        keys.data_ptr<int32_t>(), tsptr, (const int64_t*)nullptr, n, 0,
        (int64_t)1 << 40, (int64_t)1 << 40, ts_base, mask, (int)seg_bits,
        cap,
        gcursors.data_ptr<int32_t>(),
        (uint64_t*)ev_packed.data_ptr<int64_t>(),
        ev_vals.data_ptr<int64_t>(), ov_cursor.data_ptr<int32_t>(),
        (uint64_t*)ov_packed.data_ptr<int64_t>(),
        ov_vals.data_ptr<int64_t>(), ov_packed.numel(),
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), win_m2, win_maxfast, NO_LATE_ARGS);
  };
  auto scat = [&](auto kern, auto tsptr, unsigned gx, size_t lds) {
    hipLaunchKernelGGL(
        kern, dim3(gx), dim3(256), lds, stream,
        keys.data_ptr<int32_t>(), tsptr, (const int64_t*)nullptr, n, 0,
        (int64_t)1 << 40, (int64_t)1 << 40, ts_base, mask, (int)seg_bits, cap,
        gcursors.data_ptr<int32_t>(),
        (uint64_t*)ev_packed.data_ptr<int64_t>(),
        ev_vals.data_ptr<int64_t>(), ov_cursor.data_ptr<int32_t>(),
        (uint64_t*)ov_packed.data_ptr<int64_t>(),
        ov_vals.data_ptr<int64_t>(), ov_packed.numel(),
        (unsigned long long*)max_ts.data_ptr<int64_t>(),
        error_flag.data_ptr<int32_t>(), win_m2, win_maxfast, NO_LATE_ARGS);
  };
  auto scat_any = [&](auto tsptr) {
    using TSV = std::remove_const_t<std::remove_pointer_t<decltype(tsptr)>>;
    if (staged && staged_lds <= 160 * 1024) {
      unsigned gs = (unsigned)((n + 8191) / 8192);
      if (gs > 1024) gs = 1024;
      if (gs < 1) gs = 1;
      scat512(k_radix_scatter_staged<AGG_TS, TSV, 16, 512>, tsptr, gs,
              staged_lds);
    } else {
      size_t hist_lds = (size_t)nseg * sizeof(int);
      scat(k_radix_scatter_fixed<AGG_TS, TSV>, tsptr,
           (unsigned)n_blocks(n, 256), 2 * hist_lds);
    }
  };
  if (ts32) scat_any(ts.data_ptr<int32_t>());
  else scat_any(ts.data_ptr<int64_t>());

  auto offsets = at::arange(
      nseg, at::TensorOptions().dtype(at::kInt).device(keys.device()));
  offsets = offsets * (int)cap;
  // LDS staging sized ~2x the expected distinct keys per segment.
  int lds_bits = 12;
  while ((int64_t)1 << lds_bits > nslots >> 1 && lds_bits > 6) lds_bits--;
  size_t agg_lds = (size_t)32 << lds_bits;
  hipLaunchKernelGGL(
      k_radix_session_agg, dim3((unsigned)nseg),
      dim3(lds_bits >= 12 ? 1024 : 256), agg_lds, stream,
      (const uint64_t*)ev_packed.data_ptr<int64_t>(),
      ev_vals.data_ptr<int64_t>(), offsets.data_ptr<int32_t>(),
      gcursors.data_ptr<int32_t>(), cap, lds_bits,
      (uint64_t*)skeys.data_ptr<int64_t>(),
      (long long*)sstart.data_ptr<int64_t>(),
      (long long*)slast.data_ptr<int64_t>(),
      (long long*)sacc.data_ptr<int64_t>(), mask, gap_ms,
      ov_cursor.data_ptr<int32_t>(),
      (uint64_t*)ov_packed.data_ptr<int64_t>(),
      ov_vals.data_ptr<int64_t>(), ov_packed.numel(),
      out_keys.data_ptr<int32_t>(), out_start.data_ptr<int64_t>(),
      out_end.data_ptr<int64_t>(), out_vals.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), out_keys.numel(),
      error_flag.data_ptr<int32_t>());
  hipLaunchKernelGGL(
      k_session_ov_walk, dim3(1), dim3(64), 0, stream,
      (const uint64_t*)ov_packed.data_ptr<int64_t>(),
      ov_vals.data_ptr<int64_t>(), ov_cursor.data_ptr<int32_t>(),
      ov_packed.numel(), (uint64_t*)skeys.data_ptr<int64_t>(),
      (long long*)sstart.data_ptr<int64_t>(),
      (long long*)slast.data_ptr<int64_t>(),
      (long long*)sacc.data_ptr<int64_t>(), mask, gap_ms,
      out_keys.data_ptr<int32_t>(), out_start.data_ptr<int64_t>(),
      out_end.data_ptr<int64_t>(), out_vals.data_ptr<int64_t>(),
      out_n.data_ptr<int32_t>(), out_keys.numel(),
      error_flag.data_ptr<int32_t>());
}

// ---- String dictionary wrappers ----

int64_t dict_encode(
    torch::Tensor bytes,    // uint8 device [total_bytes]
    torch::Tensor offs,     // int64 device [n+1]
    torch::Tensor dlo,      // int64 device [nslots] (init EMPTY)
    torch::Tensor dhi,      // int64 device [nslots]
    torch::Tensor dids,     // int32 device [nslots]
    torch::Tensor counter,  // int32 device [1]
    torch::Tensor new_ids,  // int32 device [new_cap]
    torch::Tensor new_idx,  // int32 device [new_cap]
    torch::Tensor new_n,    // int32 device [1]
    torch::Tensor out_ids,  // int32 device [n]
    torch::Tensor error_flag) {
  check_dev(bytes, torch::kUInt8, "bytes");
  check_dev(offs, torch::kInt64, "offs");
  check_dev(dlo, torch::kInt64, "dlo");
  check_dev(out_ids, torch::kInt32, "out_ids");
  int64_t n = offs.numel() - 1;
  int64_t nslots = dlo.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "dict size must be 2^k");
  if (n == 0) return 0;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  uint64_t mask = (uint64_t)(nslots - 1);
  new_n.zero_();
  hipLaunchKernelGGL(
      k_dict_insert, grid, block, 0, stream,
      bytes.data_ptr<uint8_t>(), offs.data_ptr<int64_t>(), n,
      (uint64_t*)dlo.data_ptr<int64_t>(),
      (uint64_t*)dhi.data_ptr<int64_t>(), dids.data_ptr<int32_t>(), mask,
      counter.data_ptr<int32_t>(), new_ids.data_ptr<int32_t>(),
      new_idx.data_ptr<int32_t>(), new_n.data_ptr<int32_t>(),
      new_ids.numel(), error_flag.data_ptr<int32_t>());
  hipLaunchKernelGGL(
      k_dict_lookup, grid, block, 0, stream,
      bytes.data_ptr<uint8_t>(), offs.data_ptr<int64_t>(), n,
      (const uint64_t*)dlo.data_ptr<int64_t>(),
      (const uint64_t*)dhi.data_ptr<int64_t>(), dids.data_ptr<int32_t>(),
      mask, out_ids.data_ptr<int32_t>(), error_flag.data_ptr<int32_t>());
  return n;
}

void dict_restore(
    torch::Tensor bytes,
    torch::Tensor offs,
    torch::Tensor ids,  // int32 device [n] pinned id per string
    torch::Tensor dlo,
    torch::Tensor dhi,
    torch::Tensor dids,
    torch::Tensor error_flag) {
  check_dev(bytes, torch::kUInt8, "bytes");
  check_dev(offs, torch::kInt64, "offs");
  check_dev(ids, torch::kInt32, "ids");
  int64_t n = offs.numel() - 1;
  int64_t nslots = dlo.numel();
  TORCH_CHECK((nslots & (nslots - 1)) == 0, "dict size must be 2^k");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      k_dict_insert_pinned, dim3(n_blocks(n, 256)), dim3(256), 0, stream,
      bytes.data_ptr<uint8_t>(), offs.data_ptr<int64_t>(),
      ids.data_ptr<int32_t>(), n, (uint64_t*)dlo.data_ptr<int64_t>(),
      (uint64_t*)dhi.data_ptr<int64_t>(), dids.data_ptr<int32_t>(),
      (uint64_t)(nslots - 1), error_flag.data_ptr<int32_t>());
}

// Pack a str batch into per-destination-rank wire segments for the
// all-to-allv string exchange (owner = content hash % world).
// Returns nothing; fills `counts` (strings/rank), `byte_counts`
// (bytes/rank), `send_lens`/`send_ts`/`send_vals` (bucket-major wire
// order) and `send_bytes`.  All device work stays on the current
// stream (cumsums included); callers read counts to host for the
// collective split sizes.
void str_exchange_pack(
    torch::Tensor bytes,   // uint8 [total]
    torch::Tensor offs,    // int64 [n+1]
    torch::Tensor ts,      // int64 [n]
    c10::optional<torch::Tensor> vals,  // int64 [n]
    int64_t world,
    torch::Tensor counts,       // int32 [world] out (zeroed here)
    torch::Tensor byte_counts,  // int64 [world] out (zeroed here)
    torch::Tensor send_lens,    // int32 [n] out
    torch::Tensor send_ts,      // int64 [n] out
    torch::Tensor send_vals,    // int64 [n or 0] out
    torch::Tensor send_bytes    // uint8 [total] out
) {
  check_dev(bytes, torch::kUInt8, "bytes");
  check_dev(offs, torch::kInt64, "offs");
  check_dev(ts, torch::kInt64, "ts");
  check_dev(send_lens, torch::kInt32, "send_lens");
  int64_t n = offs.numel() - 1;
  TORCH_CHECK(world >= 1, "world must be >= 1");
  TORCH_CHECK(send_lens.numel() >= n, "send_lens too small");
  TORCH_CHECK(send_bytes.numel() >= bytes.numel(), "send_bytes too small");
  counts.zero_();
  byte_counts.zero_();
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dim3 block(256);
  dim3 grid(n_blocks(n, 256));
  hipLaunchKernelGGL(
      k_str_bucket_hist, grid, block, 0, stream,
      bytes.data_ptr<uint8_t>(), offs.data_ptr<int64_t>(), n, (int)world,
      counts.data_ptr<int32_t>(),
      (long long*)byte_counts.data_ptr<int64_t>());
  auto cursors =
      (torch::cumsum(counts, 0, torch::kInt32) - counts).contiguous();
  const int64_t* vptr =
      vals.has_value() ? vals->data_ptr<int64_t>() : nullptr;
  auto src_idx = torch::empty(
      {n}, torch::TensorOptions()
               .dtype(torch::kInt32)
               .device(bytes.device()));
  hipLaunchKernelGGL(
      k_str_meta_scatter, grid, block, 0, stream,
      bytes.data_ptr<uint8_t>(), offs.data_ptr<int64_t>(),
      ts.data_ptr<int64_t>(), vptr, n, (int)world,
      cursors.data_ptr<int32_t>(), send_lens.data_ptr<int32_t>(),
      send_ts.data_ptr<int64_t>(),
      vptr != nullptr ? send_vals.data_ptr<int64_t>() : nullptr,
      src_idx.data_ptr<int32_t>());
  auto lens64 = send_lens.narrow(0, 0, n).to(torch::kInt64);
  auto send_offs = (torch::cumsum(lens64, 0) - lens64).contiguous();
  hipLaunchKernelGGL(
      k_str_byte_gather, grid, block, 0, stream,
      bytes.data_ptr<uint8_t>(), offs.data_ptr<int64_t>(),
      src_idx.data_ptr<int32_t>(), send_offs.data_ptr<int64_t>(), n,
      send_bytes.data_ptr<uint8_t>());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("str_exchange_pack", &str_exchange_pack,
        "pack a str batch into per-rank wire segments (content-hash "
        "owner) for the all-to-allv string exchange");
  m.def("session_radix_insert", &session_radix_insert,
        "fused radix session insert: AGG_TS scatter + per-segment LDS "
        "session aggregation + sequential overflow walk");
  m.def("dict_encode", &dict_encode,
        "device string-dictionary encode: 2-phase insert+lookup");
  m.def("dict_restore", &dict_restore,
        "device string-dictionary restore with pinned ids");
  m.def("window_agg_insert", &window_agg_insert,
        "Fused window-id + hash-insert + watermark over an event batch");
  m.def("radix_v2_window_insert", &radix_v2_window_insert,
        "Experimental two-level radix with full-line LDS-staged "
        "scatter (COUNT mode)");
  m.def("radix_scatter_only", &radix_scatter_only,
        "Scatter stage of the radix insert on the current stream; returns "
        "the entry base for radix_agg_only, or with compact=True the pair "
        "(entry base, entry format)",
        pybind11::arg("keys"), pybind11::arg("ts"), pybind11::arg("vals"),
        pybind11::arg("max_ts"), pybind11::arg("error_flag"),
        pybind11::arg("gcursors"), pybind11::arg("ev_packed"),
        pybind11::arg("ev_vals"), pybind11::arg("ov_cursor"),
        pybind11::arg("ov_packed"), pybind11::arg("ov_vals"),
        pybind11::arg("nslots"), pybind11::arg("align_ms"),
        pybind11::arg("len_ms"), pybind11::arg("mode"),
        pybind11::arg("ts_base"), pybind11::arg("region_bits"),
        pybind11::arg("off_ms"), pybind11::arg("seg_counts"),
        pybind11::arg("seg_bases"), pybind11::arg("compact") = false);
  m.def("radix_agg_only", &radix_agg_only,
        "Aggregation stage of the radix insert on the current stream",
        pybind11::arg("tkeys"), pybind11::arg("tvals"),
        pybind11::arg("error_flag"), pybind11::arg("gcursors"),
        pybind11::arg("ev_packed"), pybind11::arg("ev_vals"),
        pybind11::arg("ov_cursor"), pybind11::arg("ov_packed"),
        pybind11::arg("ov_vals"), pybind11::arg("mode"),
        pybind11::arg("region_bits"),
        pybind11::arg("entry_w") = (int64_t)ENTRY_W_CLASSIC,
        pybind11::arg("entry_fmt") = (int64_t)-1,
        pybind11::arg("spill_total") = pybind11::none());
  m.def("window_agg_insert_late", &window_agg_insert_late,
        "Single-pass window insert that diverts events below the late "
        "cutoff to a late buffer");
  m.def("radix_window_insert_late", &radix_window_insert_late,
        "Radix window insert that diverts events below the late cutoff "
        "to a late buffer");
  m.def("stats_insert_late", &stats_insert_late,
        "Stats insert that diverts events below the late cutoff to a "
        "late buffer");
  m.def("radix_stats_insert_late", &radix_stats_insert_late,
        "Radix stats insert that diverts events below the late cutoff "
        "to a late buffer");
  m.def("radix_window_insert", &radix_window_insert,
        "Radix-partitioned LDS-staged keyed window aggregation",
        pybind11::arg("keys"), pybind11::arg("ts"), pybind11::arg("vals"),
        pybind11::arg("tkeys"), pybind11::arg("tvals"),
        pybind11::arg("max_ts"), pybind11::arg("error_flag"),
        pybind11::arg("gcursors"), pybind11::arg("ev_packed"),
        pybind11::arg("ev_vals"), pybind11::arg("ov_cursor"),
        pybind11::arg("ov_packed"), pybind11::arg("ov_vals"),
        pybind11::arg("align_ms"), pybind11::arg("len_ms"),
        pybind11::arg("mode"), pybind11::arg("ts_base"),
        pybind11::arg("region_bits"), pybind11::arg("off_ms"),
        pybind11::arg("seg_counts"), pybind11::arg("seg_bases"),
        pybind11::arg("spill_total") = pybind11::none(),
        pybind11::arg("compact") = true);
  m.def("close_migrate", &close_migrate,
        "Window close with reclamation: emit closed cells and migrate "
        "live cells into a fresh table");
  m.def("close_extract", &close_extract,
        "Extract (and clear) closed windows from the keyed state table");
  m.def("stats_insert", &stats_insert,
        "Keyed running count/sum/min/max over an event batch (1BRC)");
  m.def("radix_stats_insert", &radix_stats_insert,
        "Radix-partitioned LDS-staged keyed stats aggregation");
  m.def("stats_fixup", &stats_fixup,
        "Add count/sum deltas to existing stats slots (recovery)");
  m.def("stats_extract", &stats_extract,
        "Extract (and clear) keyed stats below a window horizon");
  m.def("stats_close_migrate", &stats_close_migrate,
        "Stats close with reclamation: emit due cells, migrate live "
        "cells into a fresh table, drop cells below the closed horizon");
  m.def("stats_pane_close", &stats_pane_close,
        "Sliding stats close: fold the panes of due windows into a fold "
        "table, migrate live panes into a fresh table, drop dead panes");
  m.def("radix_join_insert", &radix_join_insert,
        "Region-partitioned stream join insert (L2-local table ops)");
  m.def("join_insert", &join_insert,
        "Stream-stream hash join insert; emits completed pairs");
  m.def("session_insert", &session_insert,
        "Gap-based session aggregation over a (key, ts)-sorted batch");
  m.def("session_close_migrate", &session_close_migrate,
        "Emit sessions idle past the horizon; migrate live cells");
  m.def("session_restore", &session_restore,
        "Rebuild session cells from a host spill");
  m.def("session_run_collapse", &session_run_collapse,
        "Collapse a (key, ts)-sorted batch into gap-separated runs");
  m.def("session_run_merge", &session_run_merge,
        "Merge sorted runs into the multi-session table (also restore)");
  m.def("session_multi_close_migrate", &session_multi_close_migrate,
        "Emit each cell's closable prefix; migrate the open sessions");
  m.def("session_merge_batch", &session_merge_batch,
        "Merge per-key per-batch (count, min_ts, max_ts) rows into "
        "the session table (gap >= batch span fast path)");
  m.def("join_extract", &join_extract,
        "Extract live join state (recovery snapshot)");
  m.def("wjoin_insert", &wjoin_insert,
        "Windowed join: insert one side's batch (stamp, elect, commit)");
  m.def("wjoin_insert_late", &wjoin_insert_late,
        "Windowed join insert that diverts events below the late cutoff "
        "to a late buffer");
  m.def("wjoin_close_migrate", &wjoin_close_migrate,
        "Windowed join close: emit [win_lo, win_hi), migrate the cells "
        "at or above win_hi");
  m.def("wjoin_extract", &wjoin_extract,
        "Windowed join: extract live cells with stamps (non-mutating)");
  m.def("wjoin_pane_stamp", &wjoin_pane_stamp,
        "Sliding windowed join close, stamp pass: fold the pane stamps of "
        "due windows into a fold table, migrate live panes, drop dead ones");
  m.def("wjoin_pane_commit", &wjoin_pane_commit,
        "Sliding windowed join close, commit pass: the pane that holds a "
        "fold stamp stores its value");
  m.def("wjprod_insert", &wjprod_insert,
        "Windowed product join: count and append one side's batch");
  m.def("wjprod_plan", &wjprod_plan,
        "Windowed product join close, plan pass: list the due cells");
  m.def("wjprod_gather", &wjprod_gather,
        "Windowed product join close, gather pass over one side's log: "
        "due values into the arena, live entries into the fresh state");
  m.def("wjprod_expand", &wjprod_expand,
        "Windowed product join close, expand pass: one row per pair");
  m.def("filter_compact", &filter_compact,
        "Stream compaction of a RecordBatch by a boolean mask");
  m.def("bucket_hist", &bucket_hist, "Per-destination counts for exchange");
  m.def("bucket_scatter", &bucket_scatter,
        "Scatter events into per-destination segments for all-to-allv");
  m.def("native_run_window_steps_graph", &native_run_window_steps_graph,
        "hipGraph-captured native step loop (latency mode: one graph "
        "launch per pool cycle)");
  m.def("native_run_window_steps", &native_run_window_steps,
        "Run N steps of the columnar window pipeline with no Python "
        "between steps (native step loop)");
}
