// range_scan.hip -- range calibration: where update_range (dynamic_fixed_point.py:70-94) would settle on
// one tensor, found from one read of it instead of one controller step per unit of distance.
//
//   lbt_dfxp_range_scan   table[I + 30] += #{elements whose largest overflowing range is I}, I in [-30, 30]
//   lbt_dfxp_range_pick   c1(I) = sum of the entries from I up = #{x >= 2^I} + #{x < -2^I};
//                         I* = min{I in [bits - 31, bits - 1] : float(c1(I)) / nelem <= target} per job
//
// An element's largest overflowing I ("top") is a function of its bit pattern: biased exponent - 127, one
// less for a negative power of two (x < -2^I is strict), none for +-0, denormals and NaN, every I for
// +-inf. It overflows at exactly the I <= top. The scan histograms top over bins k = top + 31 (k in
// [1, 61], top clamped to 30; k = 0 collects what overflows nowhere in [-30, 30]).
//
// Real tensors put nearly all elements into 3 to 8 neighbouring bins, so a shared histogram would serialise
// on a handful of addresses. Here every LANE owns a private column of the workgroup's LDS histogram
// (sh[bin][thread]: a wave's 64 lanes hit 64 different banks whatever their bins), so an element costs one
// ds_add_u32 that conflicts with nothing and needs no return value -- no atomic ever meets another at one
// address -- and zero-heavy tensors (post-ReLU) cost the same as any other. At the end 248 threads fold the
// 62 x 256 counters (a rotated read order keeps the fold conflict-free) and the workgroup sends one 64-bit
// atomicAdd per non-empty bin -- a table's neighbouring entries share a cache line, so those are kept few: a
// workgroup takes at least 16 K elements, and at most 512 workgroups (two per CU: 62 KiB of LDS each) stride
// over the tensor with four 16-byte loads per lane in flight. Integer sums commute: the same tensor gives the same
// table in every run.
#include "dfxp_device.h"

using namespace lbt;

namespace {

constexpr int kT = 256;                // 4 waves
constexpr int kBins = LBT_RANGE_BINS;  // 61 table entries, I = -30 .. 30
constexpr int kRows = kBins + 1;       // + row 0: overflows nowhere in the table's span
constexpr int kUnroll = 4;             // float4 loads per lane and trip
constexpr int kMaxBlocks = 512;
constexpr int kMinTrips = 4;           // a workgroup's share before the grid grows: its flush costs ~8 atomics on
                                       // ONE cache line of the table, which the L2 serialises across workgroups
typedef float f4v __attribute__((ext_vector_type(4)));

// bin of one element: 0 = overflows at no I >= -30, else top + 31 with top clamped to 30. Subtracting the
// sign bit from the magnitude borrows into the exponent exactly when the mantissa is zero: a negative power
// of two lands one bin lower (-0 goes to -1: row 0 after the clamp; -inf stays far above the clamp).
LBT_DEV int bin_of(uint32_t u) {
  const int mag = (int)(u & 0x7fffffffu);
  int k = ((mag - (int)(u >> 31)) >> 23) - 96;  // (biased exponent - 127) + 31
  k = k < 0 ? 0 : (k > kBins ? kBins : k);      // below 2^-30 (and +-0, denormals) | top > 30 (and +-inf)
  return mag > 0x7f800000 ? 0 : k;              // NaN compares false at every I
}

LBT_DEV void count(uint32_t* col, uint32_t u) { atomicAdd(col + bin_of(u) * kT, 1u); }  // this lane's column
LBT_DEV void count4(uint32_t* col, f4v v) {
  count(col, __float_as_uint(v.x));
  count(col, __float_as_uint(v.y));
  count(col, __float_as_uint(v.z));
  count(col, __float_as_uint(v.w));
}

__global__ __launch_bounds__(kT) void range_scan_kernel(const float* __restrict__ x, int64_t n, int64_t head,
                                                        int64_t n4, unsigned long long* __restrict__ table) {
  __shared__ uint32_t sh[kRows * kT];
  const int t = threadIdx.x, lane = t & 63;
  uint32_t* col = sh + t;
#pragma unroll
  for (int r = 0; r < kRows; ++r) col[r * kT] = 0u;  // own column: nobody else touches it before the barrier
  const f4v* __restrict__ x4 = reinterpret_cast<const f4v*>(x + head);
  const int64_t stride = (int64_t)gridDim.x * (kUnroll * kT);
  for (int64_t base = (int64_t)blockIdx.x * (kUnroll * kT) + t; base < n4; base += stride) {
    f4v v[kUnroll];
#pragma unroll
    for (int c = 0; c < kUnroll; ++c)  // (a slot past the end re-reads the trip's first float4: in range)
      v[c] = __builtin_nontemporal_load(x4 + (base + c * kT < n4 ? base + c * kT : base));
#pragma unroll
    for (int c = 0; c < kUnroll; ++c)
      if (base + c * kT < n4) count4(col, v[c]);
  }
  if (blockIdx.x == 0) {
    // the up-to-3 elements in front of the first 16-byte boundary and the up-to-3 behind the last whole
    // float4 (summary.hip's param_block): threads 0..2
    if (t < head) count(col, __float_as_uint(x[t]));
    const int64_t tail = head + 4 * n4 + t;
    if (t < 3 && tail < n) count(col, __float_as_uint(x[tail]));
  }
  __syncthreads();
  // fold: thread (row r = t / 4, quarter q = t % 4) adds 64 columns of its row, starting at its own lane's
  // offset so that the 64 lanes of a wave read 64 different banks
  const int r = t >> 2, q = t & 3;
  uint32_t c = 0u;
  if (r < kRows) {
    const uint32_t* row = sh + r * kT + q * 64;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) c += row[(i + lane) & 63];
  }
  c += __shfl_xor(c, 1, 64);
  c += __shfl_xor(c, 2, 64);  // (a workgroup sees < 2^32 elements)
  if (q == 0 && r >= 1 && r < kRows && c != 0u) atomicAdd(table + (r - 1), (unsigned long long)c);
}

struct PickJobs { int32_t slot[LBT_RANGE_PICK_JOBS]; };

// One wave per job: lane L holds I = L - 30.
__global__ __launch_bounds__(kT) void range_pick_kernel(const unsigned long long* __restrict__ tables,
                                                        const PickJobs jobs, int njobs, int32_t* exps,
                                                        const int32_t* __restrict__ bits,
                                                        const float* __restrict__ target,
                                                        const float* __restrict__ nelem, int32_t* kept) {
  const int j = blockIdx.x * (kT / 64) + (int)(threadIdx.x >> 6);
  if (j >= njobs) return;
  const int lane = threadIdx.x & 63;
  const int s = jobs.slot[j];
  const int b = bits[s];
  if (b >= 32) return;  // the 32-bit bypass has no range (dynamic_fixed_point.py:22-23)
  const int hi = b - 1, lo = b - 1 - kEMax;
  const int I = lane - 30;
  const bool in = lane < kBins && I >= lo && I <= hi;
  unsigned long long c = lane < kBins ? tables[(int64_t)s * kBins + lane] : 0ull;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {  // c1(I): the entries from I up
    const uint32_t lo32 = __shfl_down((uint32_t)c, o, 64), hi32 = __shfl_down((uint32_t)(c >> 32), o, 64);
    c += lane + o < 64 ? (((unsigned long long)hi32 << 32) | lo32) : 0ull;
  }
  const float r = (float)c / nelem[s];  // range_apply's fp32 quotient
  const unsigned long long ok = __ballot(in && r <= target[s]);
  const bool empty = __ballot(in && I == lo && c == 0ull) != 0ull;  // nothing reaches even 2^lo: keep
  if (lane == 0) {
    kept[s] = empty ? 1 : 0;
    if (!empty) exps[s] = ok ? (int)__ffsll((long long)ok) - 1 - 30 : hi;
  }
}

}  // namespace

extern "C" int lbt_dfxp_range_scan(const float* x, int64_t n, uint64_t* table, void* stream) {
  if (n < 0 || n > ((int64_t)1 << 40)) return LBT_EINVAL;
  if (n == 0) return LBT_OK;
  if (!x || !table) return LBT_EINVAL;
  if (reinterpret_cast<uintptr_t>(x) & 3u) return LBT_EINVAL;
  int64_t head = (int64_t)((4u - (unsigned)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int64_t n4 = (n - head) >> 2;
  const int64_t share = (int64_t)kMinTrips * kUnroll * kT;
  int64_t blocks = (n4 + share - 1) / share;
  blocks = blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks);
  hipLaunchKernelGGL(range_scan_kernel, dim3((unsigned)blocks), dim3(kT), 0, (hipStream_t)stream, x, n, head, n4,
                     reinterpret_cast<unsigned long long*>(table));
  return (int)hipGetLastError();
}

extern "C" int lbt_dfxp_range_pick(const uint64_t* tables, const int32_t* slots, int32_t njobs, int32_t* exps,
                                   const int32_t* bits, const float* target, const float* nelem, int32_t nslots,
                                   int32_t* kept, void* stream) {
  if (njobs < 0 || nslots < 0) return LBT_EINVAL;
  if (njobs == 0) return LBT_OK;
  if (!tables || !slots || !exps || !bits || !target || !nelem || !kept) return LBT_EINVAL;
  for (int32_t j = 0; j < njobs; ++j)
    if (slots[j] < 0 || slots[j] >= nslots) return LBT_EINVAL;
  for (int32_t j0 = 0; j0 < njobs; j0 += LBT_RANGE_PICK_JOBS) {
    PickJobs jobs;
    const int nj = njobs - j0 < LBT_RANGE_PICK_JOBS ? njobs - j0 : LBT_RANGE_PICK_JOBS;
    for (int j = 0; j < LBT_RANGE_PICK_JOBS; ++j) jobs.slot[j] = j < nj ? slots[j0 + j] : 0;
    hipLaunchKernelGGL(range_pick_kernel, dim3((unsigned)((nj + kT / 64 - 1) / (kT / 64))), dim3(kT), 0,
                       (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(tables), jobs, nj, exps, bits,
                       target, nelem, kept);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return LBT_OK;
}
