// igemm.h -- what the translation units of the wide implicit GEMMs share: igemm.hip (64 / 128-row tiles,
// split-K, the parity classes of a strided dgrad, the forward / dgrad entry points), igemm_big.hip (256-row
// LDS-DMA tiles and their staged epilogues), igemm_persist.hip (the persistent quantising forward and
// dgrad + pass A) and igemm_wgrad.hip (the wide weight gradients). Only what more than one of them uses:
// a helper of one family stays in that family's file. The kernels themselves stay in each unit's
// anonymous namespace; the host functions at the end are the only calls that cross units.
#pragma once
#include "conv_epilogue.h"
#include "env.h"
#include "lds_tr.h"

namespace lbt {

struct IgArgs {
  const void* a;        // x codes (fwd) or g codes (dgrad), NHWC
  const int8_t* b;      // packed weight image [ncol][ks * 16]
  int ks;               // 16-byte slices per column
  int cred;             // channels of the gathered operand (multiple of 64)
  int a_u8off;          // A8 only: codes are q - 128
  lbt_conv_desc d;
  lbt_qdesc qa, qb;
  const int32_t* colsum;  // A8 u8off: sum_k W per column (the wcolsum of the fwd image)
  float* y;
  const float* add_src;
  int64_t M;
  int ncol;
  // split-K: blockIdx.z = split, each taking nk / ksplit consecutive k-blocks and STORING its exact
  // int32 partial sums (A8: one component; A16: hi and lo' + 128 sum W) into part[split][comp][M][ncol];
  // igemm_splitk_reduce_kernel adds the splits and runs the epilogue (ksplit == 1: none of this)
  int ksplit;
  int32_t* part;
  // fwd only, ksplit == 1: the epilogue is the consuming Normalization_q's input quantiser --
  // int8 codes yq, overflow counters of qout, exact per-channel sums chsum[NSHARD][2 * ncol]
  // (sum q, sum q^2); noise index = (row % hw) * ncol + col (noise over shape[1:]); y unused
  int8_t* yq;
  lbt_qdesc qout;
  int64_t* chsum;
  int hw;
  // taps of the k loop: dgrad kh = kh0 + SH * th (th < nkh), kw likewise (fwd and unit-stride dgrad:
  // every tap, kh = th). Strided dgrad runs one launch per parity class (cpy, cpx) of the dx pixels, whose rows are
  // (n, yc, xc) -> (n, yc * SH + cpy, xc * SW + cpx) over a ch x cw grid: only the taps with
  // (ih + PT - kh) % SH == 0 reach such a pixel, and for them the source row is yc + oy - th (no
  // zero rows, no division in the loop).
  int nkh, nkw, kh0, kw0, oy, ox, ch, cw, cpy, cpx;
  // dgrad, A16, 256-row kernel only (has_bna): the BN pass A this dx feeds (lbt_dgrad_bna), run in the
  // epilogue instead of storing dx (bna_epilogue)
  int has_bna;  // 1: bna (mask_r), 2: bn3 (g2 + y_bits, bn3.nbn BNs); sample-blocked row tiles (PERM)
  int npb;      // PERM: 16-pixel blocks per sample
  int perm;     // sample-blocked row tiles (the pass-A epilogues, the PERM quantising forward epilogue)
  lbt_dgrad_bna bna;
  lbt_dgrad_bn3 bn3;
  int dbg;  // igemm_big_kernel diagnostics (LBT_IGEMM_BIG_DBG; 1: no operand loads after the prologue)
};

}  // namespace lbt

namespace {

using namespace lbt;

constexpr int kT = 256, kBT = 512;  // threads of a 128-row / wgrad workgroup, of a 256-row one
constexpr int kBK = 64;             // channels of one k-block

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

static __device__ __attribute__((aligned(16))) uint32_t kFill80[4] = {0x80808080u, 0x80808080u, 0x80808080u,
                                                                      0x80808080u};
// The weight-gradient kernels name kFill80 inside a lambda, which the compiler takes for host-device code:
// it then exports the variable and every kernel of that unit reaches it through the GOT. That was the code
// of all the kernels while they shared one unit. A unit without such a use would address kFill80 directly
// (two instructions fewer per kernel, and not the code that was measured); this reference, never called,
// gives every unit the same addressing.
__host__ __device__ inline const uint32_t* fill80_exported() { return kFill80; }

template <int N>
LBT_DEV void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef __attribute__((address_space(3))) void* lds_vptr;

// Segment swizzles of the LDS images, conflict-free for ds_read_b128's lane groups
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32): a fragment read by lanes (r = lane & 15, q = lane >> 4)
// of rows base + r (base % 16 == 0) hits 16 distinct 4-bank quads in every group.
// 64-byte rows (4 segments; bank quad = (row & 3, segment)): f = {0, 2, 3, 1}[(row >> 2) & 3].
LBT_DEV int swz64(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
// 128-byte rows (8 segments; quad = (row & 1, segment)), segments 2q ^ f and 2q + 1 ^ f: f = (row >> 1) & 5.
LBT_DEV int swz128(int row) { return (row >> 1) & 5; }

// The conv-output quantiser in the GEMM epilogue (fwd, A8). Lane (r, q) holds column cw + 16 j + r
// of rows rtile + 16 i + e. Noise: one Philox4x32 call yields the 4 values of 4 consecutive channels
// of one pixel, so the 4 lanes r = 4g .. 4g+3 each draw the block of one of their 4 rows (e = r & 3)
// and pass values round in 4 shuffle steps -- one Philox call per 4 outputs, the same values as
// quantize_rows_kernel's qnoise4 of that block. Rows past M quantise 0 (no overflow, code 0).
template <int MI, int NJ>
LBT_DEV void quant_epilogue(const IgArgs& p, const v4i (&acc)[MI][NJ], const v4i (&accw)[NJ], int u8, float scale,
                            int64_t rtile, int rlim, bool full, int cw, int r, int q) {
  const QState qs = qstate(p.qout);
  const int ncol = p.ncol;
  const int jj = r & 3;  // this lane's slot in its 4-lane group
  int ov1w = 0, ov2w = 0;
  int cs1[NJ], cs2[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) { cs1[j] = 0; cs2[j] = 0; }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    // the pixel (within its image) of row e = jj of this i: this lane draws its noise block
    const int64_t myrow = rtile + i * 16 + jj;
    const uint32_t pix = (uint32_t)((myrow < p.M ? myrow : 0) % (uint32_t)p.hw);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = cw + j * 16 + r;
      if (cw + j * 16 >= ncol) continue;  // uniform
      const uint64_t blk = ((uint64_t)pix * (uint32_t)ncol + (uint32_t)(col & ~3)) >> 2;
      Noise4 mine = {{0.f, 0.f, 0.f, 0.f}};
      if (p.qout.stochastic) mine = qnoise4(p.qout, qs.step, blk);
      float u[4] = {0.f, 0.f, 0.f, 0.f};
      // step k: lane jj sends its block's value for column (jj - k) & 3 of the group and
      // receives, from lane (jj + k) & 3, the value of this lane's column for row (jj + k) & 3
      auto noise_step = [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const int sc = (jj - k) & 3;
        const float send = sc == 0 ? mine.u[0] : sc == 1 ? mine.u[1] : sc == 2 ? mine.u[2] : mine.u[3];
        const float got = quad_from<k>(send);
        const int re = (jj + k) & 3;
        u[0] = re == 0 ? got : u[0];
        u[1] = re == 1 ? got : u[1];
        u[2] = re == 2 ? got : u[2];
        u[3] = re == 3 ? got : u[3];
      };
      noise_step(std::integral_constant<int, 0>{});
      noise_step(std::integral_constant<int, 1>{});
      noise_step(std::integral_constant<int, 2>{});
      noise_step(std::integral_constant<int, 3>{});
      const int wsum = accw[j][0];
      int cc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = full || i * 16 + e < rlim;
        const float v = ok ? (float)(acc[i][j][e] + u8 * wsum) * scale : 0.f;
        const int c = quant_w<-1>(qs, p.qout.stochastic, v, u[e], ov1w, ov2w);
        cc[e] = c;
        cs1[j] += c;
        cs2[j] += c * c;
      }
      // the same 4-lane transpose on the codes: lane jj collects row jj's codes of the group's 4
      // columns and stores them as one dword
      const uint32_t packed = quad_pack_codes(cc, jj);
      if (full || i * 16 + jj < rlim)
        *reinterpret_cast<uint32_t*>(p.yq + (rtile + i * 16 + jj) * ncol + (col & ~3)) = packed;
    }
  }
  // per-column sums: the 4 q-lanes of a column meet by shuffles, then one int64 atomic per column
  // and sum into this workgroup's shard; overflow counters: wave totals, one atomic each
  const int shard = (int)((blockIdx.x + blockIdx.y * 7u) % LBT_NSHARD);
  int64_t* cs = p.chsum + (int64_t)shard * 2 * ncol;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    // row 0 ends with the column's code sum, row 1 with its sum of squares (rows_scatter2)
    const int t = rows_scatter2(cs1[j], cs2[j]);
    const int col = cw + j * 16 + r;
    if (q < 2 && cw + j * 16 < ncol && t) atomicAdd((unsigned long long*)&cs[q * ncol + col], (unsigned long long)(long long)t);
  }
  if ((threadIdx.x & 63) == 0 && p.qout.counts) {
    int32_t* ct = p.qout.counts + ((int64_t)p.qout.slot * LBT_NSHARD + shard) * LBT_CSTRIDE;
    if (ov1w) atomicAdd(ct, ov1w);
    if (ov2w) atomicAdd(ct + 1, ov2w);
  }
}

// Launch of a kernel whose dynamic LDS may pass the 64 KiB a kernel gets unasked: the limit is raised to
// shm once per kernel, before its first launch: one function-local static per Kernel, as long as each kernel
// is launched with one argument signature (each has one call site). shm is a constant of the kernel's
// geometry, worked out next to it by the caller.
template <auto Kernel, typename... Args>
void launch_dyn_lds(dim3 grid, dim3 block, size_t shm, hipStream_t st, const Args&... args) {
  static const bool attr_ = [shm] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)shm);
    return true;
  }();
  (void)attr_;
  hipLaunchKernelGGL(Kernel, grid, block, shm, st, args...);
}

}  // namespace

// The calls that cross units: each switches on its run-time arguments to the templates of its own unit.
// Hidden: the library exports nothing but the C ABI of include/lbt_dfxp.h.
#define LBT_HIDDEN __attribute__((visibility("hidden")))
namespace lbt {

// igemm_big.hip. launch_big<mode, a16>: false = the 256-row kernel does not take this GEMM
LBT_HIDDEN bool igemm_launch_big(int mode, bool a16, const IgArgs& p, hipStream_t st);
// the tuning's fwdq_perm (lbt_igemm_tuning; the struct has its one definition in igemm_big.hip)
LBT_HIDDEN int igemm_fwdq_perm();
// igemm_persist.hip. launch_fwdq_persist<bn> (bn 64 / 128) and launch_dgrada_persist: false = not taken
LBT_HIDDEN bool igemm_launch_fwdq_persist(int bn, const IgArgs& p, int tstages, hipStream_t st);
LBT_HIDDEN bool igemm_launch_dgrada_persist(const IgArgs& p, hipStream_t st);

}  // namespace lbt
