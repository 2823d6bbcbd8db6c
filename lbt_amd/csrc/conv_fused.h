// conv_fused.h -- the scaffold shared by the fused LDS-image 3x3 conv kernels: conv_bwd_kernel and
// conv_bwd2_kernel (conv_fused_bwd.hip), conv_fwd_fused_kernel and conv_fwd2_kernel (conv_fused_fwd.hip).
#pragma once
#include "chain_flags.h"
#include "conv_epilogue.h"
#include "lds_tr.h"
#include "pk2.h"

namespace {
using namespace lbt;

// Phase stamps of conv_bwd_kernel (scratch -DLBT_TRACE builds); -DLBT_P1STUDY moves them into its load
// phase: slots 1-3 = statistics loads issued / all loads issued / statistics finished, 4 / 5 = the ends of
// the load phase and of phase 1 (tools/trace_phases.py)
#ifdef LBT_P1STUDY
#define LBT_TSS(i) LBT_TS(i)
#define LBT_TSB(i) do { if ((i) == 1) LBT_TS(4); else if ((i) == 2) LBT_TS(5); } while (0)
#else
#define LBT_TSS(i) do { } while (0)
#define LBT_TSB(i) LBT_TS(i)
#endif
constexpr int kBNW = 8;    // waves per workgroup
constexpr int kBThreads = kBNW * 64;
// image rows per workgroup: 8 for the 16-channel stage (1024 4-row tiles would take two rounds of
// two 512-thread workgroups per CU), 4 otherwise (W * C == 512: a 4-row tile is 8 MFMA tiles)
__host__ __device__ constexpr int tile_rows(int CS) { return CS == 1 ? 8 : 4; }
// phase-1 (halo) channel-quad groups per thread: the TH + 2 halo rows' in-image pixels only (W * C / 4
// == 128 groups per row); the padding cells of the LDS halo image are filled by halo_pad_fill
__host__ __device__ constexpr int halo_iters(int TH) { return ((TH + 2) * 128 + kBThreads - 1) / kBThreads; }
// Tile geometry of a fused conv kernel on C = 16 CS channels and TH image rows per workgroup (W * C ==
// 512: host check). NQ channel quads per tile (TH x 512 bytes / 4), J of them per thread in phase 3;
// NPR (m, n) MFMA pairs per tile (2 TH: one per wave at TH = 4). Two-row tiles (TH = 2, the under-filled
// 32- / 64-channel launches) leave waves 4-7 without a pair and threads >= 256 without a phase-3 group.
template <int CS_, int TH_>
struct FusedTile {
  static constexpr int CS = CS_, TH = TH_, C = CS * 16, C4 = C / 4, W = 512 / C, Wp = W + 2, NT = CS;
  static constexpr int kMaxKS = (9 * CS + 3) / 4;  // k-steps of the stride-1 3x3 conv
  static constexpr int NQ = TH * 128, J = (NQ + kBThreads - 1) / kBThreads, NPR = 2 * TH;
  static constexpr int kBIt = halo_iters(TH);
  static_assert(TH % 4 == 0 || TH == 2, "whole groups of 4 rows, or 2-row tiles");
};
// Not shared, although copies: the block decode and thread indices, the in-image halo map, the statistics
// load, phase 2 of the stride-1 kernels, phase 3 of the backward kernels. As force-inlined helpers each
// changed the code of every kernel that used it, phase 2 / 3 also its VGPRs (profiles/conv_split/README.md).

// The conv's weight image shared through LDS by the fused conv kernels: [C columns][KS k-slices] of 16
// bytes (W4: 8-byte packed slices), loaded once per workgroup with coalesced 16-byte loads (in the
// launch's first load wave), written to LDS at the end of phase 1 (no extra wait: the loads have long
// landed) and read per fragment in phase 2. Each wave used to load its n-tile's fragments itself: 2
// (C = 64), 4 (32) or 8 (16) waves per n-tile, i.e. 72 KB of weight loads per stage-3 workgroup where the
// image is 36 KB -- through one CU's load path, in the load phase that dominates these launches. LDS
// column stride padded by 16 bytes: the 16 lanes r of a fragment read conflict-free.
template <int C, int KS, bool W4>
struct WImg {
  static constexpr int kBpf = W4 ? 8 : 16;       // bytes per (column, k-slice) fragment
  static constexpr int kColB = KS * kBpf;         // bytes per column in the global image
  static constexpr int kStride = kColB + 16;      // ... in LDS
  static constexpr int kBytes = C * kStride;
  static constexpr int kChunks = C * kColB / 16;  // 16-byte chunks of the global image
  static constexpr int kIt = (kChunks + kBThreads - 1) / kBThreads;
  static_assert(kColB % 16 == 0, "16-byte chunks within a column");
  LBT_DEV static void load(const int8_t* src, v4i (&v)[kIt]) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int i = (int)threadIdx.x + it * kBThreads;
      v[it] = *reinterpret_cast<const v4i*>(src + (int64_t)(i < kChunks ? i : 0) * 16);
    }
  }
  LBT_DEV static void store(int8_t* lds, const v4i (&v)[kIt]) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int i = (int)threadIdx.x + it * kBThreads;
      if (i < kChunks) {
        const int g = i * 16, col = g / kColB;
        *reinterpret_cast<v4i*>(lds + col * kStride + (g - col * kColB)) = v[it];
      }
    }
  }
  LBT_DEV static v4i frag(const int8_t* lds, int col, int slice) {
    if constexpr (W4)
      return unpack_i4x16(*reinterpret_cast<const v2i*>(lds + col * kStride + slice * 8));
    else
      return *reinterpret_cast<const v4i*>(lds + col * kStride + slice * 16);
  }
};

// Phase 1 of the fused conv kernels enumerates only the halo rows inside the image (rows ylo .. yhi =
// max(row0 - 1, 0) .. min(row0 + TH, H - 1), wave-uniform) and the columns 0 .. W - 1: no loads and no
// element chain on the conv's zero padding. The padding cells of the LDS halo image [(TH+2)][(W+2)][C]
// -- the left and right columns of every halo row, and the whole top / bottom row of a tile at the image
// edge -- take the padding code `word` (four codes) by plain stores, from the highest threads first:
// the waves the last phase-1 iteration leaves without a group. Before the barrier that ends phase 1.
template <int C, int TH>
LBT_DEV void halo_pad_fill(int8_t* img, int row0, int H, int word) {
  constexpr int C4 = C / 4, W = 512 / C, Wp = W + 2;
  constexpr int kSide = (TH + 2) * 2 * C4;  // (halo row, left | right, channel quad)
  static_assert(kSide <= kBThreads && W * C4 <= kBThreads, "one padding word per thread and kind");
  const int t = kBThreads - 1 - (int)threadIdx.x;
  if (t < kSide) {
    const int hy = t / (2 * C4), side = (t / C4) & 1, q = t % C4;
    *reinterpret_cast<int*>(img + (hy * Wp + side * (W + 1)) * C + q * 4) = word;
  }
  if (t < W * C4) {  // a row's cells of columns 0 .. W - 1 are consecutive
    if (row0 == 0) *reinterpret_cast<int*>(img + C + t * 4) = word;
    if (row0 + TH >= H) *reinterpret_cast<int*>(img + ((TH + 1) * Wp + 1) * C + t * 4) = word;
  }
}

// ---- overflow counts as wave totals on the scalar unit: the quantisers' asymmetric predicate x >= T or
// x < -T (T a power of two) is max(x, -x*(1-2^-24)) >= T -- for x < 0 the product rounds to >= T
// exactly when -x > T (the float after T, T(1+2^-23), gives T(1+2^-24-2^-47), which rounds down to T;
// -x = T gives T(1-2^-24), representable and < T). A NaN threshold (lanes that must not count: halo
// pixels, which the owning workgroup counts) compares false. Each compare leaves its 64-bit lane mask in
// an SGPR pair; a scalar population count and a scalar add fold it into the running total of its
// quantiser, c = c1 | c2 << 16 (a wave counts < 2^16 elements per quantiser: one SGPR per quantiser),
// so c holds wave totals (the same in every lane): one VALU instruction per compare, no per-lane
// counter registers and no wave reduction at the kernel end. The empty asm pins the total per element
// pair: without it the compiler sinks the population counts to the totals' use at the kernel end and
// keeps every element's mask live (v_writelane spills of SGPR pairs). Callers run it in wave-uniform
// control flow only, with loop exits and selects the compiler can see are scalar (v_readfirstlane of the
// wave index): a total merged at a divergent branch would be copied into a VGPR.
LBT_DEV int mask_count(bool p) { return __builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }
// max(a, b) as the bare instruction: fmaxf first canonicalises (v_max x, x, x) every operand the compiler
// cannot prove canonical. The result differs from fmaxf only in which NaN comes out, and it is only compared.
LBT_DEV float max_raw(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
LBT_DEV void ov_count2(pf2 xm, float T1, float T2, int& c) {
  const pf2 n = xm * pk(-0x1.fffffep-1f, -0x1.fffffep-1f);
  const float a0 = max_raw(xm.x, n.x), a1 = max_raw(xm.y, n.y);
  c += mask_count(a0 >= T1) + mask_count(a1 >= T1) + ((mask_count(a0 >= T2) + mask_count(a1 >= T2)) << 16);
  asm volatile("" : "+s"(c));
}
// the same for xm >= 0 (inputs after a ReLU): x < -T cannot hold
LBT_DEV void ov_count2_pos(pf2 xm, float T1, float T2, int& c) {
  c += mask_count(xm.x >= T1) + mask_count(xm.y >= T1) + ((mask_count(xm.x >= T2) + mask_count(xm.y >= T2)) << 16);
  asm volatile("" : "+s"(c));
}
// A wave's packed totals of quantiser i of nq into counts_stage_w's slots (lane 0 stores)
LBT_DEV void ov_stage_w(int i, int nq, int c, int* sh) {
  counts_stage_w(i, nq, c & 0xffff, (int)((unsigned)c >> 16), sh);
}
LBT_DEV float ov_thr(bool cnt, float T) { return cnt ? T : __builtin_nanf(""); }
// the same from a mask that is 0 where the lanes count and kOvNan where they must not: T > 0 with every
// exponent bit set is a NaN. One mask serves all thresholds of an element (one register, not one each).
constexpr int kOvNan = 0x7fc00000;
LBT_DEV float ov_thr(int nanmask, float T) { return __int_as_float(__float_as_int(T) | nanmask); }

// ---- the element chains run on pk2.h's packed fp32 pairs: the fused conv kernels are VALU-bound (SQ:
// VALU busy ~70 % of the kernel), so every multiply / add / fma of a channel quad is two packed ops;
// compares, clamps, floors and conversions stay scalar.
// floor(clip(xm + u, -L, L-1)) of a pair, as floats (the codes, exact)
LBT_DEV pf2 qfloor2(const QState& s, pf2 xm, pf2 u) {
  const pf2 v = xm + u;
  return pk(floorf(clip_q(s, v.x)), floorf(clip_q(s, v.y)));
}
LBT_DEV int pack4f(pf2 a, pf2 b) {
  const int c[4] = {(int)a.x, (int)a.y, (int)b.x, (int)b.y};
  return pack4_i8(c);
}

inline bool noise_ok(const lbt_qdesc& q) { return q.bits > 0 && q.stochastic && q.noise; }

}  // namespace
