// conv_fused_fwd.hip -- the fused conv forward entry points and the training-mode instantiations of
// conv_fused_fwd.h's kernels (the testing-mode ones: conv_fused_infer.hip).
#include "conv_fused_fwd.h"
#include "env.h"

using namespace lbt;

LBT_TRACE_SETTER(conv_fwd)

// Batch-adaptive tile rows of the fused conv kernels (lbt_conv_bwd_fused_i8 and lbt_conv_fwd_fused_i8 launch
// with it; host only, nothing is launched): the 16-channel stage takes 4-row tiles when its
// 8-row tiles leave the launch with fewer workgroups than CUs (N * H / 8 < 256: per-GPU batches below
// 64 -- the strong-scaling shards of configs[2]): twice the workgroups, each with two thirds of the halo
// rows of phase 1, half the phase-3 groups and MFMA pairs per wave. LBT_TILE_ROWS1=8|4 forces one.
// The 32- / 64-channel stages take 2-row tiles when 4-row tiles leave CUs without a workgroup
// (N * H / 4 < 256: per-GPU batches below 64 for the 64-channel stage, below 32 for the 32-channel
// one): B = 16 0.301 -> 0.291 ms per step, bit-identical. Not at one tile per CU: the 64-channel stage
// at B = 128 (256 tiles) measured 0.414 -> 0.433 ms with 2-row tiles (two co-resident workgroups per CU,
// each staging the whole 37 KB weight image and a halo of 2 rows per 2; profiles/round6/tile_rows23_ab.txt).
// LBT_TILE_ROWS23=4|2 forces one.
extern "C" int lbt_conv_fused_tile_rows(int32_t Cin, int64_t N, int32_t H) {
  if (Cin != 16 && Cin != 32 && Cin != 64) return -LBT_EINVAL;
  const int CS = Cin / 16;
  if (CS != 1) {
    static const int force23 = getenv_int("LBT_TILE_ROWS23", 0);
    if (force23 == 4 || H % 4) return 4;
    return (force23 == 2 || N * H / 4 < 256) ? 2 : 4;
  }
  static const int force = getenv_int("LBT_TILE_ROWS1", 0);
  if (force == 2 || force == 4 || force == 8) return H % force ? 8 : force;  // (16-row tiles at B=128: 0.447 vs 0.429 ms)
  if (N * H / 8 >= 256 || H % 4) return 8;
  return (N * H / 4 < 256 && H % 2 == 0) ? 2 : 4;  // (2-row tiles: B = 16, as the wide stages below)
}

// Testing mode (conv_fused_infer.hip) when every normalising branch of the chain is frozen: 1; none: 0
// (the training-mode checks below stay as they were); a mixed chain would be half a moments update: -1.
static int frozen_chain(const lbt_chain_fwd& a) {
  const bool f1 = a.b1.nrm.frozen != 0, f2 = a.has_b2 ? a.b2.nrm.frozen != 0 : f1;
  return f1 != f2 ? -1 : (f1 ? 1 : 0);
}

extern "C" int lbt_conv_fwd_fused_i8(const lbt_conv_fwd* q, void* stream) {
  if (!q) return LBT_EINVAL;
  if (const int fz = frozen_chain(q->c)) return fz < 0 ? LBT_EINVAL : conv_fwd_fused_infer(q, (hipStream_t)stream);
  const lbt_conv_desc& d = q->d;
  const int C = d.Cin;
  if (!desc_ok(d) || d.KH != 3 || d.KW != 3 || d.SH != 1 || d.SW != 1 || d.PT != 1 || d.PB != 1 || d.PL != 1 ||
      d.PR != 1 || d.Ho != d.H || d.Wo != d.W || d.Cout != C || (C != 16 && C != 32 && C != 64) ||
      d.H % tile_rows(C / 16) || d.W * C != 512 || (int64_t)d.N * d.H * 512 >= ((int64_t)1 << 29))
    return LBT_EINVAL;  // (st_out4's 32-bit byte offsets)
  const int CS = C / 16;
  const lbt_chain_fwd& a = q->c;
  const int64_t inner = (int64_t)d.H * d.W * C;
  if (a.C != C || a.rows != d.N || a.inner != inner || a.o2 || !a.o1 || a.o1_kind != LBT_OUT_U8OFF) return LBT_EINVAL;
  const int f = fwd_flags(a);
  constexpr int kNeed = kFQ | kFRout | kFRelu | kFO1 | kFStoch | kFU8;
  if ((f & kRt) || (f & kNeed) != kNeed || (f & (kFO2 | kFNoR))) return LBT_EINVAL;
  if (!noise_ok(a.qo1)) return LBT_EINVAL;
  for (int br = 0; br < (a.has_b2 ? 2 : 1); ++br) {
    const lbt_chain_branch& Bb = br ? a.b2 : a.b1;
    if (!noise_ok(Bb.qr) || !Bb.gb || !Bb.nrm.chsum || Bb.nrm.frozen) return LBT_EINVAL;
  }
  if (!q->yq || !noise_ok(q->qout) || !q->wcolsum || !q->wf) return LBT_EINVAL;
  if (q->ksf != 4 * ((9 * CS + 3) / 4)) return LBT_EINVAL;
  if (q->w4 && q->qw.bits > 4) return LBT_EINVAL;
  if (q->qout.bits > 8) return LBT_EINVAL;  // int8 codes; the int32 channel sums of q^2 assume |q| <= 2^7
  ConvFwdArgs p;
  p.c = a; p.wf = q->wf; p.wcolsum = q->wcolsum; p.qw = q->qw; p.H = d.H;
  p.yq = q->yq; p.qout = q->qout; p.ychsum = q->ychsum;
  const int th = lbt_conv_fused_tile_rows(C, d.N, d.H);
  const int64_t tiles = (int64_t)d.N * (d.H / th);
  if (tiles > 0x7fffffff) return LBT_EINVAL;
  const dim3 grid((unsigned)tiles);
  hipStream_t st = (hipStream_t)stream;
  const int nb = a.has_b2 ? 2 : 1;
  const int fl = f & ~kFU8 & ~kFStoch;  // variant key: Y / residual present
#define LBT_FW_TH(CS_, NB_, FL_, TH_)                                                                        \
  if (q->w4)                                                                                                 \
    hipLaunchKernelGGL((conv_fwd_fused_kernel<CS_, NB_, FL_, true, TH_>), grid, dim3(kBThreads), 0, st, p);    \
  else                                                                                                       \
    hipLaunchKernelGGL((conv_fwd_fused_kernel<CS_, NB_, FL_, false, TH_>), grid, dim3(kBThreads), 0, st, p);
#define LBT_FW(CS_, NB_, FL_)                                                                            \
  if (CS == CS_ && nb == NB_ && fl == ((FL_) & ~kFU8 & ~kFStoch)) {                                      \
    if (CS_ == 1 && th == 4) {                                                                           \
      LBT_FW_TH(CS_, NB_, FL_, (CS_ == 1 ? 4 : tile_rows(CS_)))                                          \
    } else if (th == 2) {                                                                                \
      LBT_FW_TH(CS_, NB_, FL_, 2)                                                                        \
    } else {                                                                                             \
      LBT_FW_TH(CS_, NB_, FL_, tile_rows(CS_))                                                           \
    }                                                                                                    \
    return (int)hipGetLastError();                                                                       \
  }
  // c2 (bn1 chain), c1 after an identity / projection block, block 0's c1 (the stem's chain)
#define LBT_FW_CS(CS_)                                  \
  LBT_FW(CS_, 1, kNeed)                                 \
  LBT_FW(CS_, 1, kNeed | kFRes | kFY)                   \
  LBT_FW(CS_, 2, kNeed | kFY)
  LBT_FW(1, 1, kNeed)
  LBT_FW(1, 1, kNeed | kFRes | kFY)
  LBT_FW(1, 1, kNeed | kFY)
  LBT_FW_CS(2)
  LBT_FW_CS(4)
#undef LBT_FW_CS
#undef LBT_FW
#undef LBT_FW_TH
  return LBT_EINVAL;
}

extern "C" int lbt_conv_fwd2_fused_i8(const lbt_conv_fwd2* q, void* stream) {
  if (!q) return LBT_EINVAL;
  if (const int fz = frozen_chain(q->c)) return fz < 0 ? LBT_EINVAL : conv_fwd2_fused_infer(q, (hipStream_t)stream);
  const lbt_conv_desc &d1 = q->d1, &ds = q->ds;
  const int C = d1.Cin, Cq = d1.Cout;
  if (!desc_ok(d1) || !desc_ok(ds) || d1.KH != 3 || d1.KW != 3 || d1.SH != 2 || d1.SW != 2 || d1.PT != 0 ||
      d1.PL != 0 || ds.KH != 1 || ds.KW != 1 || ds.SH != 2 || ds.SW != 2 || ds.PT != 0 || ds.PL != 0 ||
      (C != 16 && C != 32) || Cq != 2 * C || d1.W * C != 512 || d1.H % 2 || d1.W % 2 || d1.Ho * 2 != d1.H ||
      d1.Wo * 2 != d1.W || d1.Ho % kTH2 || ds.N != d1.N || ds.H != d1.H || ds.W != d1.W || ds.Cin != C ||
      ds.Cout != Cq || ds.Ho != d1.Ho || ds.Wo != d1.Wo || (int64_t)d1.N * d1.H * 512 >= ((int64_t)1 << 29))
    return LBT_EINVAL;
  const int CS = C / 16;
  const lbt_chain_fwd& a = q->c;
  if (a.C != C || a.rows != d1.N || a.inner != (int64_t)d1.H * d1.W * C || a.has_b2 || !a.o1 || !a.o2 ||
      a.o1_kind != LBT_OUT_U8OFF || a.o2_kind != LBT_OUT_U8OFF || !a.res || !a.y)
    return LBT_EINVAL;
  const int f = fwd_flags(a);
  constexpr int kNeed = kFQ | kFRout | kFRelu | kFO1 | kFO2 | kFStoch | kFU8 | kFRes | kFY;
  if (f != kNeed) return LBT_EINVAL;
  if (!noise_ok(a.qo1) || !noise_ok(a.qo2) || !noise_ok(a.b1.qr) || !a.b1.gb || !a.b1.nrm.chsum || a.b1.nrm.frozen)
    return LBT_EINVAL;
  if (!q->yq1 || !q->yqs || !noise_ok(q->qout1) || !noise_ok(q->qouts) || !q->wcolsum1 || !q->wcolsums || !q->wf1 ||
      !q->wfs)
    return LBT_EINVAL;
  if (q->ksf1 != 4 * ((9 * CS + 3) / 4) || q->ksfs != 4) return LBT_EINVAL;
  if (q->w4 && (q->qw1.bits > 4 || q->qws.bits > 4)) return LBT_EINVAL;
  if (q->qout1.bits > 8 || q->qouts.bits > 8) return LBT_EINVAL;  // int8 codes; int32 channel sums of q^2
  ConvFwd2Args p;
  p.c = a; p.wf1 = q->wf1; p.wfs = q->wfs; p.wcolsum1 = q->wcolsum1; p.wcolsums = q->wcolsums;
  p.qw1 = q->qw1; p.qws = q->qws; p.H = d1.H; p.yq1 = q->yq1; p.yqs = q->yqs; p.qout1 = q->qout1;
  p.qouts = q->qouts; p.ychsum1 = q->ychsum1; p.ychsums = q->ychsums;
  const int64_t tiles = (int64_t)d1.N * (d1.Ho / kTH2);
  if (tiles > 0x7fffffff || (int64_t)d1.N * d1.H * d1.W * C >= ((int64_t)1 << 31)) return LBT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define LBT_F2(CS_)                                                                                           \
  if (CS == CS_) {                                                                                            \
    if (q->w4)                                                                                                \
      hipLaunchKernelGGL((conv_fwd2_kernel<CS_, true>), dim3((unsigned)tiles), dim3(kBThreads), 0, st, p);    \
    else                                                                                                      \
      hipLaunchKernelGGL((conv_fwd2_kernel<CS_, false>), dim3((unsigned)tiles), dim3(kBThreads), 0, st, p);   \
    return (int)hipGetLastError();                                                                            \
  }
  LBT_F2(1)
  LBT_F2(2)
#undef LBT_F2
  return LBT_EINVAL;
}
