// snapshot.hip — whole-state snapshots of UAVs in caller-owned device records (mrs_uav_snapshot_t, include/mrs_swarm.h "state
// snapshots"): save packs the state columns F_X .. F_PID+23, the CRASHED / TAKEOFF / VPREV_SPLIT flags and the airframe into one 496-B
// record per UAV; load writes records back, optionally through an index (one record to many UAVs: forks).  Data movement only.
//
// Two forms of each kernel.  The lane form is one lane per UAV with per-lane stores, as k_gather_rows.  The tile form takes 64 UAVs
// per block: each column is one coalesced 512-B request, the tile is transposed through LDS and leaves as its 31 744 contiguous record
// bytes in 16-B stores (load: an indexed gather of whole records in 16-B loads, then the transpose back).  The LDS row is padded to
// an odd number of 8-B words.  Which form runs: MEASUREMENTS §7.4 and pick_tile() below.
#include "host_internal.h"

namespace {

constexpr int kCols   = F_CMD;       // 60 state columns, F_X .. F_PID+23
constexpr int kWords  = kCols + 2;   // 8-B words per record: the columns, then flags | airframe and magic | reserved
constexpr int kChunks = kWords / 2;  // 16-B chunks per record
constexpr int kTile   = 64;          // UAVs per block of the tile form
constexpr int kPitch  = kWords + 1;  // LDS words per UAV of a tile: odd, so that 64-bit accesses at a stride of one row spread over banks
constexpr int kBlock  = 256;
constexpr int kWaves  = kBlock / kTile;                        // 4: wave w of a tile takes the columns w, w + 4, ...
constexpr int kColsPerWave = kCols / kWaves;                   // 15
constexpr int kChunkRounds = (kTile * kChunks + kBlock - 1) / kBlock;  // 8 (the last one partial: 1984 chunks per tile)
static_assert(kCols % kWaves == 0, "columns split evenly over the waves of a tile");
static_assert(sizeof(mrs_uav_snapshot_t) == 8 * kWords, "mrs_uav_snapshot_t: 60 doubles + 4 words");
static_assert(kWords % 2 == 0 && kPitch % 2 == 1, "record of whole 16-B chunks, odd LDS pitch");

constexpr uint32_t kKeptFlags = ~(FLAG_CRASHED | FLAG_TAKEOFF | FLAG_VPREV_SPLIT);

__device__ __forceinline__ uint32_t snap_flags(uint32_t fl) {
  return ((fl & FLAG_CRASHED) ? (uint32_t)MRS_SNAP_CRASHED : 0u) | ((fl & FLAG_TAKEOFF) ? (uint32_t)MRS_SNAP_TAKEOFF : 0u) |
         ((fl & FLAG_VPREV_SPLIT) ? (uint32_t)MRS_SNAP_VPREV_SPLIT : 0u);
}
__device__ __forceinline__ uint32_t flag_bits(uint32_t sf) {
  return ((sf & MRS_SNAP_CRASHED) ? FLAG_CRASHED : 0u) | ((sf & MRS_SNAP_TAKEOFF) ? FLAG_TAKEOFF : 0u) |
         ((sf & MRS_SNAP_VPREV_SPLIT) ? FLAG_VPREV_SPLIT : 0u);
}
// the column a record word is read from: v_prev is v unless the UAV's v_prev was split from it (F_VPREV is stale otherwise)
__device__ __forceinline__ int src_col(int c, uint32_t fl) {
  return (c >= F_VPREV && c < F_R && !(fl & FLAG_VPREV_SPLIT)) ? c - (F_VPREV - F_V) : c;
}
// the two trailing words of a record: flags | airframe << 32, magic | 0 << 32
__device__ __forceinline__ unsigned long long tail0(uint32_t fl) { return (unsigned long long)snap_flags(fl) | ((unsigned long long)(fl >> FLAG_TYPE_SHIFT) << 32); }
constexpr unsigned long long kTail1 = MRS_SNAP_MAGIC;

// status of destination UAV i reading record r (r < 0: index -1 or out of range, already decided) from its trailing words
__device__ __forceinline__ uint8_t load_status(unsigned long long w0, unsigned long long w1, uint32_t fl) {
  if ((uint32_t)w1 != MRS_SNAP_MAGIC) return MRS_SNAP_BAD_MAGIC;
  if ((uint32_t)(w0 >> 32) != (fl >> FLAG_TYPE_SHIFT)) return MRS_SNAP_BAD_AIRFRAME;
  return MRS_SNAP_LOADED;
}
// which record destination row k reads: >= 0, or -(status) when it reads none
__device__ __forceinline__ long long pick_record(const int32_t* index, int k, long long n_records) {
  if (!index) return k;
  const int32_t r = index[k];
  if (r == -1) return -(long long)MRS_SNAP_SKIPPED;
  if (r < 0 || (long long)r >= n_records) return -(long long)MRS_SNAP_BAD_INDEX;
  return r;
}

// ---- lane form ----
__global__ void __launch_bounds__(kBlock) k_save_lane(SwarmDev sw, int first, int count, unsigned long long* rec) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int          i  = first + k;
  const size_t       np = (size_t)sw.npad;
  const uint32_t     fl = sw.F[i];
  unsigned long long* o = rec + (size_t)k * kWords;
#pragma unroll
  for (int c = 0; c < kCols; c++) o[c] = (unsigned long long)__double_as_longlong(sw.S[(size_t)src_col(c, fl) * np + i]);
  o[kCols]     = tail0(fl);
  o[kCols + 1] = kTail1;
}

__global__ void __launch_bounds__(kBlock) k_load_lane(SwarmDev sw, int first, int count, const unsigned long long* rec, long long n_records,
                                                      const int32_t* index, uint8_t* status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int       i  = first + k;
  const size_t    np = (size_t)sw.npad;
  const uint32_t  fl = sw.F[i];
  const long long r  = pick_record(index, k, n_records);
  uint8_t         st = (uint8_t)(-r);
  const unsigned long long* src = rec + (size_t)(r < 0 ? 0 : r) * kWords;
  if (r >= 0) st = load_status(src[kCols], src[kCols + 1], fl);
  if (status) status[k] = st;
  if (st != MRS_SNAP_LOADED) return;
#pragma unroll
  for (int c = 0; c < kCols; c++) sw.S[(size_t)c * np + i] = __longlong_as_double((long long)src[c]);
  sw.F[i] = (fl & kKeptFlags) | flag_bits((uint32_t)src[kCols]);
}

// ---- tile form: 64 UAVs per block of 256 lanes (4 waves) ----
__global__ void __launch_bounds__(kBlock) k_save_tile(SwarmDev sw, int first, int count, ulonglong2* rec) {
  __shared__ unsigned long long t[kTile * kPitch];
  const int    base = blockIdx.x * kTile;
  const int    m    = min(kTile, count - base);
  const int    u    = threadIdx.x & (kTile - 1);
  const int    wv   = threadIdx.x / kTile;
  const size_t np   = (size_t)sw.npad;
  if (u < m) {
    const int      i  = first + base + u;
    const uint32_t fl = sw.F[i];
#pragma unroll
    for (int j = 0; j < kColsPerWave; j++) {  // column c of the tile: one 512-B request per wave, 15 in flight
      const int c = wv + kWaves * j;
      t[u * kPitch + c] = (unsigned long long)__double_as_longlong(sw.S[(size_t)src_col(c, fl) * np + i]);
    }
    if (wv == 0) {
      t[u * kPitch + kCols]     = tail0(fl);
      t[u * kPitch + kCols + 1] = kTail1;
    }
  }
  __syncthreads();
  ulonglong2* dst = rec + (size_t)base * kChunks;  // the tile's records, contiguous
#pragma unroll
  for (int j = 0; j < kChunkRounds; j++) {
    const int q = threadIdx.x + kBlock * j;
    if (q >= m * kChunks) break;
    const int r = q / kChunks, w = 2 * (q - r * kChunks);
    dst[q] = make_ulonglong2(t[r * kPitch + w], t[r * kPitch + w + 1]);
  }
}

__global__ void __launch_bounds__(kBlock) k_load_tile(SwarmDev sw, int first, int count, const ulonglong2* rec, long long n_records,
                                                      const int32_t* index, uint8_t* status) {
  __shared__ unsigned long long t[kTile * kPitch];
  __shared__ long long          src[kTile];  // record of each UAV of the tile, or -(status)
  const int    base = blockIdx.x * kTile;
  const int    m    = min(kTile, count - base);
  const int    u    = threadIdx.x & (kTile - 1);
  const int    wv   = threadIdx.x / kTile;
  const size_t np   = (size_t)sw.npad;
  if (threadIdx.x < m) src[threadIdx.x] = pick_record(index, base + threadIdx.x, n_records);
  __syncthreads();
  // whole records, 16 B per lane: every load of the lane issued before the first LDS write
  ulonglong2 v[kChunkRounds];
  int        at[kChunkRounds];  // LDS word of the chunk, -1: nothing to write
#pragma unroll
  for (int j = 0; j < kChunkRounds; j++) {
    const int       q = threadIdx.x + kBlock * j;
    const int       r = min(q / kChunks, kTile - 1), w = q - r * kChunks;  // (r clamped: the last round runs past the tile)
    const long long s = q < m * kChunks ? src[r] : -1;
    at[j]             = s >= 0 ? r * kPitch + 2 * w : -1;
    if (s >= 0) v[j] = rec[(size_t)s * kChunks + w];
  }
#pragma unroll
  for (int j = 0; j < kChunkRounds; j++) {
    if (at[j] >= 0) {
      t[at[j]]     = v[j].x;
      t[at[j] + 1] = v[j].y;
    }
  }
  __syncthreads();
  if (wv == 0 && u < m) {  // status, from the record's trailing words (in LDS now) and the UAV's own flag word
    const int       i  = first + base + u;
    const uint32_t  fl = sw.F[i];
    const long long s  = src[u];
    const uint8_t   st = s < 0 ? (uint8_t)(-s) : load_status(t[u * kPitch + kCols], t[u * kPitch + kCols + 1], fl);
    if (status) status[base + u] = st;
    if (st == MRS_SNAP_LOADED) sw.F[i] = (fl & kKeptFlags) | flag_bits((uint32_t)t[u * kPitch + kCols]);
    else src[u] = -1;
  }
  __syncthreads();
  if (u < m && src[u] >= 0) {
    const int i = first + base + u;
#pragma unroll
    for (int j = 0; j < kColsPerWave; j++) {
      const int c = wv + kWaves * j;
      sw.S[(size_t)c * np + i] = __longlong_as_double((long long)t[u * kPitch + c]);
    }
  }
}

inline dim3 lanes_of(int count) { return dim3((unsigned)((count + kBlock - 1) / kBlock)); }
inline dim3 tiles_of(int count) { return dim3((unsigned)((count + kTile - 1) / kTile)); }

// MRS_SNAP_FORM=lane / tile forces a form (measurement aid; read per call)
bool pick_tile() {
  const char* e = getenv("MRS_SNAP_FORM");
  if (e && !strcmp(e, "lane")) return false;
  if (e && !strcmp(e, "tile")) return true;
  return true;
}

int check_records(const mrs_swarm* s, const void* p, size_t n, const char* what) {
  if (p && ((uintptr_t)p & 15u)) return fail(MRS_ERR_ARG, std::string(what) + ": records must be 16-B aligned");
  return check_device_ptr(s, p, n * sizeof(mrs_uav_snapshot_t), what);
}

}  // namespace

extern "C" {

int mrs_swarm_save_device(mrs_swarm_t* s, int32_t first, int32_t count, mrs_uav_snapshot_t* dev_records, void* ext_stream) {
  MRS_ENTER(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_save_device: not on a sharded swarm");
  if (count == 0) return MRS_OK;
  if ((rc = check_records(s, dev_records, (size_t)count, "dev_records"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  if (pick_tile())
    hipLaunchKernelGGL(k_save_tile, tiles_of(count), dim3(kBlock), 0, s->stream, s->view(), first, count, reinterpret_cast<ulonglong2*>(dev_records));
  else
    hipLaunchKernelGGL(k_save_lane, lanes_of(count), dim3(kBlock), 0, s->stream, s->view(), first, count,
                       reinterpret_cast<unsigned long long*>(dev_records));
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

int mrs_swarm_load_device(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_uav_snapshot_t* dev_records, int64_t n_records,
                          const int32_t* dev_index, uint8_t* dev_status, void* ext_stream) {
  MRS_ENTER(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_load_device: not on a sharded swarm");
  if (n_records < 0) return fail(MRS_ERR_ARG, "n_records < 0");
  if (!dev_index && n_records < count) return fail(MRS_ERR_ARG, "n_records < count without an index");
  if (count == 0) return MRS_OK;
  if ((rc = check_records(s, dev_records, (size_t)n_records, "dev_records"))) return rc;
  if (dev_index && (rc = check_device_ptr(s, dev_index, sizeof(int32_t) * (size_t)count, "dev_index"))) return rc;
  if (dev_status && (rc = check_device_ptr(s, dev_status, (size_t)count, "dev_status"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  if (pick_tile())
    hipLaunchKernelGGL(k_load_tile, tiles_of(count), dim3(kBlock), 0, s->stream, s->view(), first, count,
                       reinterpret_cast<const ulonglong2*>(dev_records), (long long)n_records, dev_index, dev_status);
  else
    hipLaunchKernelGGL(k_load_lane, lanes_of(count), dim3(kBlock), 0, s->stream, s->view(), first, count,
                       reinterpret_cast<const unsigned long long*>(dev_records), (long long)n_records, dev_index, dev_status);
  HIPCHK(hipGetLastError());
  // what mrs_swarm_copy_uavs notes: positions changed under the neighbour lists and the position records, and a loaded force must act
  s->nbr_dirty   = true;
  s->p_valid     = false;
  s->fext_active = true;
  return fence_out(s, ext);
}

}  // extern "C"
