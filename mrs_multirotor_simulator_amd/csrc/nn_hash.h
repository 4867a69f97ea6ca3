// nn_hash.h — the per-call spatial hash of UAV positions (nearest.hip builds it: bin, scan, scatter) as its readers see it: the sorted
// record, the cell coordinate, the bucket hash with and without world labels, and where a bucket's records begin.  Shared by the kernels of
// nearest.hip (k-nearest rows, proximity cost) and range_scan_uavs.hip (scans that see other UAVs), so that the bin side and every probe
// side form cells and buckets with the same text.  Device code only; the host builds a hash through mrs_host::nn_hash (host_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrs_nn {

constexpr int    SCAN_LOG    = 11;            // log2 of the counts per chunk of the two-level bucket scan (2048)
constexpr double CELL_LIMIT  = 1073741824.0;  // 2^30: clamped cell coordinates, +-1 stays inside int32
constexpr double CELL_MARGIN = 1e-6;          // edge = radius (1 + margin): covers the rounding of x * inv_edge up to |x * inv_edge| = 2^30

struct NnRec {  // one sorted record: position, global index and world label (32 B)
  double  x, y, z;
  int32_t idx, pad;  // pad: the world label (0 when the swarm has none)
};

// one built hash, as a kernel of another unit reads it (mrs_host::nn_hash)
struct NnHash {
  const NnRec*   rec;
  const int32_t *cnt, *start, *bsum;
  double         inv_edge;
  uint32_t       tmask;
  int32_t        n;
};

__device__ __forceinline__ int cell_coord(double x, double inv_edge) {
  const double c = floor(x * inv_edge);  // (+-inf for an overflowing product: clamped like any far cell)
  return (int)fmin(fmax(c, -CELL_LIMIT), CELL_LIMIT);
}

// wm: a mixed image of the world label (0 for label 0 and for swarms without labels: the hash they always had)
__device__ __forceinline__ uint32_t world_mix(uint32_t w) {
  w *= 0x9E3779B1u;
  w ^= w >> 16;
  w *= 0x85EBCA6Bu;
  w ^= w >> 13;
  return w;
}
// A world-aware kernel is the same kernel template with the label column as a trailing argument pack of one: the instantiation with the
// empty pack has the arguments and the code it always had.
__device__ __forceinline__ const uint32_t* world_labels() { return nullptr; }
__device__ __forceinline__ const uint32_t* world_labels(const uint32_t* p) { return p; }
__device__ __forceinline__ uint32_t bucket_of(int cx, int cy, int cz, uint32_t tmask) {
  uint32_t h = ((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u);
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  return h & tmask;
}
__device__ __forceinline__ uint32_t bucket_of(int cx, int cy, int cz, uint32_t tmask, uint32_t wm) {  // (world-aware)
  uint32_t h = ((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u) ^ wm;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  return h & tmask;
}
template <bool WORLDS> __device__ __forceinline__ uint32_t bucket_of_x(int cx, int cy, int cz, uint32_t tmask, uint32_t wm) {
  if constexpr (WORLDS) return bucket_of(cx, cy, cz, tmask, wm); else return bucket_of(cx, cy, cz, tmask);
}

// first record of bucket b: the two levels of the bucket scan added on the fly
__device__ __forceinline__ int bucket_begin(const int32_t* start, const int32_t* bsum, uint32_t b) { return start[b] + bsum[b >> SCAN_LOG]; }

}  // namespace mrs_nn
