// conv_fused_infer.hip -- the testing-mode (INF) instantiations of conv_fused_fwd.h's kernels and their
// launchers: lbt_conv_fwd_fused_i8 / lbt_conv_fwd2_fused_i8 on a chain whose normalising branches are all
// frozen (Model.set_testing: the running averages normalise, nothing is updated). A forward-only launch:
// no channel sums, no overflow counters, and the R / X codes go to memory only where a pointer is given.
#include "conv_fused_fwd.h"

using namespace lbt;

LBT_TRACE_SETTER(conv_infer)

namespace {

// a frozen branch of an inference launch: codes in, running averages, a stochastic table-fed Rescale_q
// quantiser without counters
bool branch_ok(const lbt_chain_branch& b) {
  return b.nrm.frozen && b.nrm.q && b.nrm.run_mean && b.nrm.run_var && b.gb && noise_ok(b.qr) && !b.qr.counts;
}
// an output quantiser of an inference launch
bool qout_ok(const lbt_qdesc& q) { return noise_ok(q) && !q.counts; }

}  // namespace

int lbt::conv_fwd_fused_infer(const lbt_conv_fwd* q, hipStream_t st) {
  const lbt_conv_desc& d = q->d;
  const int C = d.Cin;
  if (!desc_ok(d) || d.KH != 3 || d.KW != 3 || d.SH != 1 || d.SW != 1 || d.PT != 1 || d.PB != 1 || d.PL != 1 ||
      d.PR != 1 || d.Ho != d.H || d.Wo != d.W || d.Cout != C || (C != 16 && C != 32 && C != 64) ||
      d.H % tile_rows(C / 16) || d.W * C != 512 || (int64_t)d.N * d.H * 512 >= ((int64_t)1 << 29))
    return LBT_EINVAL;  // (st_out4's 32-bit byte offsets)
  const int CS = C / 16;
  const lbt_chain_fwd& a = q->c;
  if (a.C != C || a.rows != d.N || a.inner != (int64_t)d.H * d.W * C || a.o2 || !a.relu) return LBT_EINVAL;
  if (a.o1 && a.o1_kind != LBT_OUT_U8OFF) return LBT_EINVAL;
  if (!branch_ok(a.b1) || (a.has_b2 && !branch_ok(a.b2)) || !qout_ok(a.qo1)) return LBT_EINVAL;
  if (!q->yq || !qout_ok(q->qout) || q->ychsum || !q->wcolsum || !q->wf) return LBT_EINVAL;
  if (q->ksf != 4 * ((9 * CS + 3) / 4)) return LBT_EINVAL;
  if (q->w4 && q->qw.bits > 4) return LBT_EINVAL;
  ConvFwdArgs p;
  p.c = a; p.wf = q->wf; p.wcolsum = q->wcolsum; p.qw = q->qw; p.H = d.H;
  p.yq = q->yq; p.qout = q->qout; p.ychsum = nullptr;
  const int th = lbt_conv_fused_tile_rows(C, d.N, d.H);
  const int64_t tiles = (int64_t)d.N * (d.H / th);
  if (tiles > 0x7fffffff) return LBT_EINVAL;
  const dim3 grid((unsigned)tiles);
  const int nb = a.has_b2 ? 2 : 1;
  const int fl = (a.res ? kFRes : 0) | (a.y ? kFY : 0);  // variant key: residual / Y present
#define LBT_FI_TH(CS_, NB_, FL_, TH_)                                                                              \
  if (q->w4)                                                                                                       \
    hipLaunchKernelGGL((conv_fwd_fused_kernel<CS_, NB_, FL_, true, TH_, true>), grid, dim3(kBThreads), 0, st, p);  \
  else                                                                                                             \
    hipLaunchKernelGGL((conv_fwd_fused_kernel<CS_, NB_, FL_, false, TH_, true>), grid, dim3(kBThreads), 0, st, p);
#define LBT_FI(CS_, NB_, FL_)                                  \
  if (CS == CS_ && nb == NB_ && fl == (FL_)) {                 \
    if (CS_ == 1 && th == 4) {                                 \
      LBT_FI_TH(CS_, NB_, FL_, (CS_ == 1 ? 4 : tile_rows(CS_))) \
    } else if (th == 2) {                                      \
      LBT_FI_TH(CS_, NB_, FL_, 2)                              \
    } else {                                                   \
      LBT_FI_TH(CS_, NB_, FL_, tile_rows(CS_))                 \
    }                                                          \
    return (int)hipGetLastError();                             \
  }
  // the chains of the training plan (c2's bn1 chain; c1 after an identity block, after a projection block,
  // after the stem), on every stage
#define LBT_FI_CS(CS_)            \
  LBT_FI(CS_, 1, 0)               \
  LBT_FI(CS_, 1, kFRes | kFY)     \
  LBT_FI(CS_, 1, kFY)             \
  LBT_FI(CS_, 2, kFY)
  LBT_FI_CS(1)
  LBT_FI_CS(2)
  LBT_FI_CS(4)
#undef LBT_FI_CS
#undef LBT_FI
#undef LBT_FI_TH
  return LBT_EINVAL;
}

int lbt::conv_fwd2_fused_infer(const lbt_conv_fwd2* q, hipStream_t st) {
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
  if (a.C != C || a.rows != d1.N || a.inner != (int64_t)d1.H * d1.W * C || a.has_b2 || !a.res || !a.y || !a.relu)
    return LBT_EINVAL;
  if ((a.o1 && a.o1_kind != LBT_OUT_U8OFF) || (a.o2 && a.o2_kind != LBT_OUT_U8OFF)) return LBT_EINVAL;
  if (!branch_ok(a.b1) || !qout_ok(a.qo1) || !qout_ok(a.qo2)) return LBT_EINVAL;
  if (!q->yq1 || !q->yqs || !qout_ok(q->qout1) || !qout_ok(q->qouts) || q->ychsum1 || q->ychsums || !q->wcolsum1 ||
      !q->wcolsums || !q->wf1 || !q->wfs)
    return LBT_EINVAL;
  if (q->ksf1 != 4 * ((9 * CS + 3) / 4) || q->ksfs != 4) return LBT_EINVAL;
  if (q->w4 && (q->qw1.bits > 4 || q->qws.bits > 4)) return LBT_EINVAL;
  ConvFwd2Args p;
  p.c = a; p.wf1 = q->wf1; p.wfs = q->wfs; p.wcolsum1 = q->wcolsum1; p.wcolsums = q->wcolsums;
  p.qw1 = q->qw1; p.qws = q->qws; p.H = d1.H; p.yq1 = q->yq1; p.yqs = q->yqs; p.qout1 = q->qout1;
  p.qouts = q->qouts; p.ychsum1 = nullptr; p.ychsums = nullptr;
  const int64_t tiles = (int64_t)d1.N * (d1.Ho / kTH2);
  if (tiles > 0x7fffffff || (int64_t)d1.N * d1.H * d1.W * C >= ((int64_t)1 << 31)) return LBT_EINVAL;
#define LBT_F2I(CS_)                                                                                               \
  if (CS == CS_) {                                                                                                 \
    if (q->w4)                                                                                                     \
      hipLaunchKernelGGL((conv_fwd2_kernel<CS_, true, true>), dim3((unsigned)tiles), dim3(kBThreads), 0, st, p);   \
    else                                                                                                           \
      hipLaunchKernelGGL((conv_fwd2_kernel<CS_, false, true>), dim3((unsigned)tiles), dim3(kBThreads), 0, st, p);  \
    return (int)hipGetLastError();                                                                                 \
  }
  LBT_F2I(1)
  LBT_F2I(2)
#undef LBT_F2I
  return LBT_EINVAL;
}
