// igemm_wgrad.hip -- the weight gradients of the wide layers (the implicit GEMMs of igemm.hip): the atomic /
// storing 64 x 64 kernel, the 3x3 stride-1 body and the 1x1 16-bit body.
//
// dW[tap][ci][co] = sum_p x[p shifted by tap][ci] * g[p][co] for the wide layers. x is offset int8
// (x' = x - 128, post-ReLU 9-bit codes 0..255); g is int8 or int16 (G16: g = 256 gh + gl' + 128).
// Per workgroup: one tap, 64 ci x 64 co, a pixel range; each wave walks 64-pixel chunks, stores
// [pixel][16 B] LDS images and multiplies ds_read_b64_tr_b8 fragments (as conv_wgrad_body.h's wgrad).
// Exact identity (over every processed lane, invalid ones carrying x' = -128, g = 0):
//   sum x g = 256 sum x' gh + sum x' gl' + 128 sum x' + 128 (256 sum gh + sum gl' + 128 npix)
// (G8: sum x g = sum x' g + 128 sum g); the row / column sums come from MFMAs against ones.
// The 4 waves meet in LDS (int64), then one int64 atomic per output into shard (split % nshard).
#include "igemm.h"

namespace {

// XCD-contiguous logical id of workgroup b of n: the hardware deals workgroups round-robin over the 8
// XCDs, so logical ids [start_x, start_x + count_x) all run on XCD x, in dispatch order (bijective)
LBT_DEV uint32_t xcd_logical(uint32_t b, uint32_t n) {
  const uint32_t x = b % 8, q = n / 8, r = n % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

constexpr int kWP = 64;

// STORE: the workgroup's partial is STORED into slab[split] (every element of slab[nsplit][K][Cout]
// has exactly one writer -- no zeroing, no atomics); else atomically added into shard split % nshard.
// Grid: 1-D over (split, tap x ci block, co block). xmap = 1 (default): XCD-aware order -- the
// workgroups of one pixel split (every ci / co block, which share that split's X and G chunks) are
// consecutive on ONE XCD, meant to serve the Cout/64-fold X and Cin/64-fold G re-reads of a 64 x 64 tile
// from that XCD's L2 (LBT_WGRAD_XMAP=1; measured 0.3 ms per ResNet-50 step SLOWER); xmap = 0 (default):
// split fastest (the former 3-D grid's order).
template <bool G16, bool STORE>
__global__ __launch_bounds__(kT, 1) void wgrad_wide_kernel(const int8_t* __restrict__ xq, const void* __restrict__ gq,
                                                        lbt_conv_desc d, long long* __restrict__ slab, int64_t P,
                                                        int nsplit, int nshard, int xmap) {
  constexpr int NG = G16 ? 2 : 1;  // G images: (gh, gl') or g
  constexpr int NBS = 4, COW = 16 * NBS;  // output-channel slices per workgroup
  // per wave: X [4 slices][64 px][16 B], G [NG][4 slices][64 px][16 B]; reused as the int64 tile
  __shared__ __attribute__((aligned(16))) int8_t lds[4][(4 + NBS * NG) * kWP * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int cib = d.Cin / 64, cob = d.Cout / 64;
  const uint32_t gy = (uint32_t)(d.KH * d.KW * cib), nblk = gy * (uint32_t)cob;
  uint32_t split, by, ob_;
  if (xmap) {
    const uint32_t nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, qq = nwg / 8, rr = nwg % 8;
    const uint32_t t = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + orig / 8;
    split = t / nblk;
    const uint32_t b = t - split * nblk;
    by = b / (uint32_t)cob;
    ob_ = b - by * (uint32_t)cob;
  } else {
    split = blockIdx.x % (uint32_t)nsplit;
    const uint32_t b = blockIdx.x / (uint32_t)nsplit;
    ob_ = b / gy;
    by = b - ob_ * gy;
  }
  const int tap = (int)by / cib, cb = (int)by - tap * cib, ob = (int)ob_;
  const int kh = tap / d.KW, kw = tap - kh * d.KW;
  int8_t* Xi = lds[wave];
  int8_t* Gi = lds[wave] + 4 * kWP * 16;
  const int64_t per = (P + nsplit - 1) / nsplit;
  const int64_t p0 = (int64_t)split * per;
  const int64_t p1 = p0 + per < P ? p0 + per : P;
  const uint32_t HWo = (uint32_t)d.Ho * d.Wo;
  v4i acc[NG][4][NBS], ax[4], ag[NG][NBS];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    ax[a] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < NBS; ++b)
#pragma unroll
      for (int h = 0; h < NG; ++h) acc[h][a][b] = v4i{0, 0, 0, 0};
  }
#pragma unroll
  for (int h = 0; h < NG; ++h)
#pragma unroll
    for (int b = 0; b < NBS; ++b) ag[h][b] = v4i{0, 0, 0, 0};
  const v4i ones = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
  long long nchunks = 0;
  // operand registers of one 64-pixel chunk; the next chunk's loads are issued right after this
  // chunk's registers are in LDS, so they fly during its MFMAs (no extra registers)
  v4i xs[4], gs[G16 ? 2 * NBS : NBS];
  bool xv = false, pv = false;
  auto issue = [&](int64_t c0) {
    const int64_t p = c0 + lane;
    pv = p < p1;
    const uint32_t pu = (uint32_t)(pv ? p : p0);
    const uint32_t n = pu / HWo, rem = pu - n * HWo;
    const int oh = (int)(rem / (uint32_t)d.Wo), ow = (int)(rem - (uint32_t)oh * (uint32_t)d.Wo);
    const int ih = oh * d.SH + kh - d.PT, iw = ow * d.SW + kw - d.PL;
    xv = pv && (unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W;
    const int8_t* xp = xq + (xv ? ((((int64_t)n * d.H + ih) * d.W + iw) * d.Cin + cb * 64) : 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) xs[s] = *reinterpret_cast<const v4i*>(xp + s * 16);
    if constexpr (G16) {
      const int16_t* gp = reinterpret_cast<const int16_t*>(gq) + (int64_t)pu * d.Cout + ob * COW;
#pragma unroll
      for (int s = 0; s < 2 * NBS; ++s) gs[s] = *reinterpret_cast<const v4i*>(gp + s * 8);
    } else {
      const int8_t* gp = reinterpret_cast<const int8_t*>(gq) + (int64_t)pu * d.Cout + ob * COW;
#pragma unroll
      for (int s = 0; s < NBS; ++s) gs[s] = *reinterpret_cast<const v4i*>(gp + s * 16);
    }
  };
  const int64_t cfirst = p0 + (int64_t)wave * kWP;
  issue(cfirst < p1 ? cfirst : p0);
  for (int64_t c0 = cfirst; c0 < p1; c0 += 4 * kWP) {
    ++nchunks;
    const int fx = (int)0x80808080u;  // x' = -128: x = 0 (padding, pixels past the range)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!xv) xs[s] = v4i{fx, fx, fx, fx};
      *reinterpret_cast<v4i*>(Xi + (s * kWP + lane) * 16) = xs[s];
    }
    if constexpr (G16) {
#pragma unroll
      for (int s = 0; s < NBS; ++s) {  // 16 codes -> 16 gh bytes, 16 gl' bytes; past the range g = 0
        int hi[4], lo[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t c01 = (uint32_t)gs[2 * s + (w >> 1)][(w & 1) * 2];
          const uint32_t c23 = (uint32_t)gs[2 * s + (w >> 1)][(w & 1) * 2 + 1];
          hi[w] = pv ? (int)__builtin_amdgcn_perm(c23, c01, 0x07050301u) : 0;
          lo[w] = pv ? (int)(__builtin_amdgcn_perm(c23, c01, 0x06040200u) ^ 0x80808080u) : (int)0x80808080u;
        }
        *reinterpret_cast<v4i*>(Gi + (s * kWP + lane) * 16) = v4i{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<v4i*>(Gi + ((NBS + s) * kWP + lane) * 16) = v4i{lo[0], lo[1], lo[2], lo[3]};
      }
    } else {
#pragma unroll
      for (int s = 0; s < NBS; ++s) {
        if (!pv) gs[s] = v4i{0, 0, 0, 0};
        *reinterpret_cast<v4i*>(Gi + (s * kWP + lane) * 16) = gs[s];
      }
    }
    const int64_t cn = c0 + 4 * kWP;
    issue(cn < p1 ? cn : c0);  // the next chunk (clamped: straight-line, a redundant last load)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    v4i gf[NG][NBS];
#pragma unroll
    for (int h = 0; h < NG; ++h)
#pragma unroll
      for (int b = 0; b < NBS; ++b) {
        gf[h][b] = tr_frag(Gi + (h * NBS + b) * kWP * 16, 16 * q, lane);
        ag[h][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, gf[h][b], ag[h][b], 0, 0, 0);
      }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const v4i xf = tr_frag(Xi + a * kWP * 16, 16 * q, lane);
      ax[a] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf, ones, ax[a], 0, 0, 0);
#pragma unroll
      for (int h = 0; h < NG; ++h)
#pragma unroll
        for (int b = 0; b < NBS; ++b) acc[h][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf, gf[h][b], acc[h][a][b], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  // ---- combine exactly; the 4 waves meet in LDS (int64 [64 ci][64 co]) one after another
  // (plain read-modify-write, each wave owning the tile between two barriers)
  __syncthreads();
  long long* tile = reinterpret_cast<long long*>(&lds[0][0]);
  const long long npix = nchunks * kWP;
  long long vv[4][NBS][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < NBS; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (G16) {
          const long long sg = 256ll * ag[0][b][i] + (long long)ag[1][b][i] + 128ll * npix;  // sum_p g[co]
          vv[a][b][i] = 256ll * acc[0][a][b][i] + (long long)acc[1][a][b][i] + 128ll * ax[a][i] + 128ll * sg;
        } else {
          vv[a][b][i] = (long long)acc[0][a][b][i] + 128ll * ag[0][b][i];
        }
      }
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NBS; ++b)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            long long* t = &tile[(a * 16 + q * 4 + i) * COW + b * 16 + r];
            *t = w == 0 ? vv[a][b][i] : *t + vv[a][b][i];
          }
    }
    __syncthreads();
  }
  const int64_t shard = STORE ? (int64_t)split : (int64_t)(split % (uint32_t)nshard);
  long long* dst = slab + (shard * (d.KH * d.KW) + tap) * d.Cin * d.Cout;
  for (int i = threadIdx.x; i < 64 * COW; i += kT) {
    const long long v = tile[i];
    const int ci = cb * 64 + i / COW, co = ob * COW + i % COW;
    if constexpr (STORE)
      dst[(int64_t)ci * d.Cout + co] = v;
    else if (v)
      atomicAdd((unsigned long long*)&dst[(int64_t)ci * d.Cout + co], (unsigned long long)v);
  }
}


// ----------------------------------------------------------------------------- 3x3 wgrad, all taps
// wgrad3_kernel: a stride-1 SAME 3x3 conv's weight gradient with ALL 9 taps in one workgroup tile, so
// X and G leave L2 once per (ci block, co block) instead of once per tap (wgrad_wide_kernel's 9x).
// Workgroup = (pixel split, 64 ci, 64 co) of 8 waves; a chunk is RB = 64 / W whole output rows of one
// image (RB * W <= 64 pixels = the MFMA k), staged once for all waves: the X halo window
// [4 ci slices][(RB + 2) x (W + 2) pixels][16 B] (fill code outside the image) and G's 64 pixels x
// 64 co ([hi | lo'][4 co slices][64 px][16 B]; past the rows / image: g = 0). Wave w owns ci slice
// w & 3 and co slices 2 (w >> 2) + {0, 1} for all 9 taps; its A fragments are transposed reads of
// the window at the tap's offset (pixels past the chunk read a duplicate of its last pixel: their
// g = 0 cancels them exactly, see the identity of wgrad_wide_kernel), its B fragments the G image.
// The next chunk's loads fly during the MFMAs. Every (split, tap, ci, co) has one writer: STORED
// into slab[split][9 * Cin][Cout] (int64), reduced by lbt_conv_wgrad_reduce64 over the splits.
constexpr int kW3Win = 192;  // window pixels per ci slice: (64 / W + 2) * (W + 2) <= 192 (host check)

// ds_read_b64_tr_b8 as inline asm: the compiler's waitcnt pass makes every ds_read_tr intrinsic wait
// for ALL outstanding LDS-DMA (vmcnt(0): it cannot tell the ring's stages apart), which serialises the
// DMA ring. The asm form is invisible to that pass, so its results are fenced by hand: tr_wait()
// (s_waitcnt lgkmcnt(0)) takes the fragments as in/out operands, so no use can move above it.
LBT_DEV v2i tr8_asm(uint32_t addr) {
  v2i r;
  asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
LBT_DEV v4i tr_frag_asm(uint32_t a, uint32_t b) {
  const v2i lo = tr8_asm(a), hi = tr8_asm(b);
  return v4i{lo.x, lo.y, hi.x, hi.y};
}
LBT_DEV void tr_wait(v4i& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)::"memory"); }

LBT_DEV v4i tr_frag2(const int8_t* img, int oa, int ob) {
  typedef __attribute__((address_space(3))) v2i lds_v2i;
  const v2i lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i*)(img + oa));
  const v2i hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i*)(img + ob));
  return v4i{lo.x, lo.y, hi.x, hi.y};
}

// Operands reach LDS by LDS-DMA (global_load_lds_dwordx4, no staging registers) through an S-stage
// ring of raw chunks -- the X window in its final [slice][pixel][16 B] layout, G as raw codes
// [pixel][64 co] -- with one barrier per chunk: step c waits for chunk c + 1's DMA, splits its raw G
// into the hi / lo' planes of plane buffer (c + 1) & 1, issues chunk c + S - 1's DMA into the stage
// chunk c - 1 left, and runs chunk c's MFMAs. NXW = X DMA instructions per wave per chunk (each wave
// issues exactly NXW + 1 per chunk -- idle slots write a dummy KiB -- so the vmcnt waits are constants).
template <bool G16, int NXW, int S>
__global__ __launch_bounds__(512, 2) void wgrad3_kernel(const int8_t* __restrict__ xq, const void* __restrict__ gq,
                                                      lbt_conv_desc d, long long* __restrict__ slab, int nsplit,
                                                      int dbg) {
  constexpr int NP = G16 ? 2 : 1;                    // G planes: (gh, gl') or g
  constexpr int XB = 4 * kW3Win * 16;                // X window image (12 KiB)
  constexpr int GB = 64 * 64 * (G16 ? 2 : 1);        // raw G codes of a chunk (8 / 4 KiB)
  constexpr int STG = XB + GB;
  constexpr int PB = NP * 4 * 64 * 16;               // one plane buffer
  extern __shared__ __attribute__((aligned(16))) int8_t lds[];
  int8_t* const planes = lds + S * STG;              // [2][PB]
  int8_t* const dummy = planes + 2 * PB;             // 1 KiB sink of the idle DMA slots
  __shared__ int sax[9 * 64];  // sum_p x' per (tap, ci): waves 0-3 -> all
  __shared__ int sag[NP * 64];  // sum_p g (planes) per co: waves with ci slice 0 -> all
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int H = d.H, W = d.W, Cin = d.Cin, Cout = d.Cout;
  const int RB = 64 / W, NPX = RB * W, Wp = W + 2, WIN = (RB + 2) * Wp;
  const int CPI = (H + RB - 1) / RB;
  const int64_t TC = (int64_t)d.N * CPI;
  const int nblk = (Cin / 64) * (Cout / 64);
  // dbg bit 1: XCD-aware order (a pixel split's channel blocks, which read the same X / G chunks, on one
  // XCD's L2)
  const uint32_t bid = (dbg & 2) ? xcd_logical(blockIdx.x, gridDim.x) : blockIdx.x;
  const int blk = (int)(bid % (uint32_t)nblk), split = (int)(bid / (uint32_t)nblk);
  const int cb = blk / (Cout / 64), ob = blk - cb * (Cout / 64);
  const int64_t c0 = TC * split / nsplit, c1 = TC * (split + 1) / nsplit;
  const int nc = (int)(c1 - c0);
  typedef __attribute__((address_space(3))) int8_t lds_i8;
  const uint32_t lbase = (uint32_t)(uintptr_t)(lds_i8*)lds;  // LDS byte address of the ring
  const int ws = wave & 3, wh = wave >> 2;
  const bool do_ax = G16 && wh == 0, do_ag = ws == 0;
  // transposed-read offsets (X: clamped to the chunk). Lane group q supplies k = pixels 8q .. 8q+7 (first
  // read) and 32+8q .. 32+8q+7 (second) -- any k order serves, A and B use the same -- so lanes 0-31 of
  // each ds_read_b64_tr_b8 cover 16 consecutive 16-byte rows (all 64 banks once; pixels 16q + j/2 put
  // lane groups 0 and 1 on the same 32 banks: 2-way conflicts)
  const int pa = 8 * q + (j >> 1), pb = pa + 32;
  const int xa = pa < NPX ? pa : NPX - 1, xb = pb < NPX ? pb : NPX - 1;
  const int oxa = ((xa / W) * Wp + xa % W) * 16 + 8 * (j & 1);
  const int oxb = ((xb / W) * Wp + xb % W) * 16 + 8 * (j & 1);
  const int oga = pa * 16 + 8 * (j & 1), ogb = pb * 16 + 8 * (j & 1);
  const int ngx = (WIN + 63) >> 6;  // 64-pixel groups of the window per slice

  // DMA of chunk k (clamped to the split's last) into stage st. Everything but the chunk's (image,
  // first row) is loop-invariant per lane, and issue() is called with k = 0, 1, 2, ... (clamped), so
  // (n, row0) advance incrementally -- no divisions in the loop.
  int xhy[NXW], xrel[NXW], xdst[NXW];
  bool xreal[NXW];
#pragma unroll
  for (int u = 0; u < NXW; ++u) {
    const int ins = wave + 8 * u;  // (slice, pixel group) = (ins % 4, ins / 4)
    const int sl = ins & 3, gp = ins >> 2;
    const int pix = gp * 64 + lane;
    const int hy = pix / Wp, hx = pix - hy * Wp;
    xreal[u] = gp < ngx;
    // window pixels past WIN and columns outside the image read the fill (hy = -1 marks them)
    xhy[u] = (pix < WIN && hx >= 1 && hx <= W) ? hy : -1000000;
    xrel[u] = (hy - 1) * W + (hx - 1);
    xdst[u] = xreal[u] ? (sl * kW3Win + gp * 64) * 16 : -1;
  }
  const int gitem = wave * 64 + lane;
  const int gpl = G16 ? gitem >> 3 : gitem >> 2, gseg = G16 ? gitem & 7 : gitem & 3;
  const bool greal = G16 || wave < 4;
  const int grow = gpl < NPX ? gpl / W : 1000000;  // output row of the pixel within the chunk
  int in_n = (int)(c0 / CPI), in_row0 = (int)(c0 - (int64_t)in_n * CPI) * RB, in_k = 0;
  auto issue = [&](int k, int st) {
    if (k < nc && k != in_k) {  // advance to chunk k (= in_k + 1)
      in_row0 += RB;
      if (in_row0 >= H) { in_row0 = 0; ++in_n; }
      in_k = k;
    }
    const int n = in_n, row0 = in_row0;
    int8_t* sb = lds + st * STG;
    const int8_t* xim = xq + ((int64_t)n * H * W + (int64_t)row0 * W) * Cin + cb * 64;
#pragma unroll
    for (int u = 0; u < NXW; ++u) {
      const int sl = (wave + 8 * u) & 3;
      const bool in = (unsigned)(row0 - 1 + xhy[u]) < (unsigned)H;
      const int8_t* src = in ? xim + (int64_t)xrel[u] * Cin + sl * 16 : reinterpret_cast<const int8_t*>(kFill80);
      int8_t* dst = xreal[u] ? sb + xdst[u] : dummy;
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)dst, 16, 0, 0);
    }
    {  // G: wave w moves items 64 w .. 64 w + 63 of the chunk's raw codes (G8: waves 4-7 idle)
      const bool in = greal && row0 + grow < H;
      const int8_t* src = in ? reinterpret_cast<const int8_t*>(gq) +
                                   (((int64_t)n * H * W + (int64_t)row0 * W + gpl) * Cout + ob * 64) * (G16 ? 2 : 1) +
                                   gseg * 16
                             : reinterpret_cast<const int8_t*>(zi());
      int8_t* dst = greal ? sb + XB + wave * 1024 : dummy;
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)dst, 16, 0, 0);
    }
  };
  // raw G of the chunk in stage st -> plane buffer pbuf (one 16-byte item per thread)
  auto split_g = [&](int st, int pbuf) {
    const int8_t* raw = lds + st * STG + XB;
    int8_t* pl8 = planes + pbuf * PB;
    if constexpr (G16) {
      const int pl = tid >> 3, seg = tid & 7;
      const v4i gr = *reinterpret_cast<const v4i*>(raw + tid * 16);
      int hi[2], lo[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const uint32_t c01 = (uint32_t)gr[2 * w], c23 = (uint32_t)gr[2 * w + 1];
        hi[w] = (int)__builtin_amdgcn_perm(c23, c01, 0x07050301u);
        lo[w] = (int)(__builtin_amdgcn_perm(c23, c01, 0x06040200u) ^ 0x80808080u);
      }
      const int o = ((seg >> 1) * 64 + pl) * 16 + (seg & 1) * 8;
      *reinterpret_cast<v2i*>(pl8 + o) = v2i{hi[0], hi[1]};
      *reinterpret_cast<v2i*>(pl8 + 4 * 64 * 16 + o) = v2i{lo[0], lo[1]};
    } else if (tid < 256) {
      *reinterpret_cast<v4i*>(pl8 + ((tid & 3) * 64 + (tid >> 2)) * 16) = *reinterpret_cast<const v4i*>(raw + tid * 16);
    }
  };

  v4i acc[9][2][NP], ax[9], ag[2][NP];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    ax[t] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int h = 0; h < NP; ++h) acc[t][c][h] = v4i{0, 0, 0, 0};
  }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int h = 0; h < NP; ++h) ag[c][h] = v4i{0, 0, 0, 0};
  const v4i ones = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
  constexpr int G1 = NXW + 1;  // DMA instructions per wave per chunk

  // chunk k's MFMAs; the A fragment of tap t + 1 is read while tap t's MFMAs run
  auto mma = [&](int k) {
    const uint32_t xs = lbase + (uint32_t)((k % S) * STG + ws * kW3Win * 16);
    const uint32_t gp = lbase + (uint32_t)(S * STG + (k & 1) * PB);
    v4i bf[2][NP];
#pragma unroll
    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        const uint32_t b = gp + (uint32_t)(((h * 4 + 2 * wh + cs) * 64) * 16);
        bf[cs][h] = tr_frag_asm(b + oga, b + ogb);
      }
    v4i af = tr_frag_asm(xs + oxa, xs + oxb);
#pragma unroll
    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
      for (int h = 0; h < NP; ++h) tr_wait(bf[cs][h]);
    tr_wait(af);
    if (do_ag) {
#pragma unroll
      for (int cs = 0; cs < 2; ++cs)
#pragma unroll
        for (int h = 0; h < NP; ++h) ag[cs][h] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bf[cs][h], ag[cs][h], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      v4i an = af;
      if (t < 8) {
        const uint32_t toff = (uint32_t)((((t + 1) / 3) * Wp + (t + 1) % 3) * 16);
        an = tr_frag_asm(xs + oxa + toff, xs + oxb + toff);
      }
      if (do_ax) ax[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, ones, ax[t], 0, 0, 0);
#pragma unroll
      for (int cs = 0; cs < 2; ++cs)
#pragma unroll
        for (int h = 0; h < NP; ++h) acc[t][cs][h] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[cs][h], acc[t][cs][h], 0, 0, 0);
      if (t < 8) {
        tr_wait(an);
        af = an;
      }
    }
  };

  if (nc > 0) {
#pragma unroll
    for (int k = 0; k < S - 1; ++k) issue(k, k);
    vm_wait<(S - 2) * G1>();  // chunk 0 landed
    __builtin_amdgcn_s_barrier();
    split_g(0, 0);
    for (int k = 0; k < nc; ++k) {
      vm_wait<(S - 3) * G1>();  // chunk k + 1 landed (this wave's part)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's plane writes of chunk k
      __builtin_amdgcn_s_barrier();  // every wave's DMA of k + 1 and planes of k; chunk k - 1's readers done
      if (!(dbg & 1)) issue(k + S - 1, (k + S - 1) % S);
      mma(k);
      split_g((k + 1) % S, (k + 1) & 1);  // in the MFMAs' shadow; past the last chunk: a harmless stale split
    }
    vm_wait<0>();  // no DMA may still write LDS when the workgroup ends
  }
  // ---- the row / column sums to every wave, then one exact int64 per output
  if (do_ax && j == 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) sax[t * 64 + ws * 16 + 4 * q + i] = ax[t][i];
  }
  if (do_ag && q == 0) {
#pragma unroll
    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
      for (int h = 0; h < NP; ++h) sag[h * 64 + (2 * wh + cs) * 16 + j] = ag[cs][h][0];
  }
  __syncthreads();
  const long long npix = (long long)nc * 64;
  long long* dst = slab + (int64_t)split * 9 * Cin * Cout;
#pragma unroll
  for (int cs = 0; cs < 2; ++cs) {
    const int col = (2 * wh + cs) * 16 + j;
    const long long sgc = G16 ? 256ll * sag[col] + (long long)sag[64 + col] + 128ll * npix : (long long)sag[col];
    const int co = ob * 64 + col;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cl = ws * 16 + 4 * q + i;
        long long v;
        if constexpr (G16)
          v = 256ll * acc[t][cs][0][i] + (long long)acc[t][cs][NP - 1][i] + 128ll * sax[t * 64 + cl] + 128ll * sgc;
        else
          v = (long long)acc[t][cs][0][i] + 128ll * sgc;
        dst[((int64_t)t * Cin + cb * 64 + cl) * Cout + co] = v;
      }
  }
}

template <bool G16, int NXW>
void wgrad3_launch(const int8_t* xq, const void* gq, const lbt_conv_desc& d, long long* slab, int nsplit, dim3 grid,
                   int dbg, hipStream_t st) {
  constexpr int S = 4;
  constexpr int PB = (G16 ? 2 : 1) * 4 * 64 * 16;
  constexpr size_t shm = (size_t)S * (4 * kW3Win * 16 + 64 * 64 * (G16 ? 2 : 1)) + 2 * PB + 1024;
  // LBT_WGRAD_XCD bit 1: the XCD-aware order for the 3x3 body (dbg bit 1)
  static const int xmap = getenv_int("LBT_WGRAD_XCD", 1) & 2;
  launch_dyn_lds<&wgrad3_kernel<G16, NXW, S>>(grid, dim3(512), shm, st, xq, gq, d, slab, nsplit, dbg | xmap);
}

bool wgrad3_ok(const lbt_conv_desc& d) {
  if (d.KH != 3 || d.KW != 3 || d.SH != 1 || d.SW != 1 || d.PT != 1 || d.PB != 1 || d.PL != 1 || d.PR != 1 ||
      d.Ho != d.H || d.Wo != d.W || d.W > 64 || d.Cin % 64 || d.Cout % 64)
    return false;
  const int RB = 64 / d.W;
  return (RB + 2) * (d.W + 2) <= kW3Win;
}

// ----------------------------------------------------------------------------- 1x1 wgrad, 16-bit G
// wgrad1_kernel: a 1x1 conv's weight gradient (pad 0, any stride) with 16-bit gradient codes on a
// workgroup tile of (64 WCI) ci x (32 WCO) co, WCI x WCO = 8 waves of 64 ci x 32 co (wgrad_wide_kernel's
// 64 x 64 tile re-read X Cout/64 times and G Cin/64 times: ~616 MB of operand loads per ResNet-50 1x1
// conv against 100-460 MB of data). A chunk = 64 pixels (the MFMA k); every operand image is
// [64 px][16 B] -- an X slice of 16 ci, or a RAW G group of 8 co as (lo, hi) byte pairs -- moved by
// LDS-DMA through an S-stage ring with one barrier per chunk. The raw G image needs no split pass:
// a transposed read gives lane i byte i of each pixel's 16 bytes, i.e. column i = (co i / 2, byte
// i & 1), so the MFMA runs on 16 "columns" of 8 co x (lo, hi); the lo lanes XOR their bytes with
// 0x80 (lo' = lo - 128, signed), and the epilogue joins lane pairs:
//   sum x g = 256 sum x' gh + sum x' gl' + 128 sum x' + 128 (256 sum gh + sum gl' + 128 npix)
// (x' = x - 128; every processed pixel counts, padding ones carry x' = -128, g = 0, which the
// identity cancels). Every (split, ci, co) has one writer: STORED into slab[split][Cin][Cout].
template <int WCI, int S>
__global__ __launch_bounds__(512, 1) void wgrad1_kernel(const int8_t* __restrict__ xq, const int16_t* __restrict__ gq,
                                                      lbt_conv_desc d, long long* __restrict__ slab, int nsplit,
                                                      int xmap) {
  constexpr int WCO = 8 / WCI;
  constexpr int TCI = 64 * WCI, TCO = 32 * WCO;     // workgroup tile
  constexpr int NXS = TCI / 16, NGG = TCO / 8;       // X slices, G groups (1 KiB images each)
  constexpr int NXW = (NXS + 7) / 8, NGW = NGG / 8;  // DMA instructions per wave per chunk
  constexpr int G1 = NXW + NGW;
  constexpr int STG = (NXS + NGG) * 1024;
  static_assert(NGG % 8 == 0, "geometry");
  extern __shared__ __attribute__((aligned(16))) int8_t lds[];
  int8_t* const dummy = lds + S * STG;  // 1 KiB sink of idle X slots
  __shared__ int sax[TCI];              // sum_p x' per ci
  __shared__ int sag[2 * TCO];          // sum_p of each raw-G column (co, byte)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int wci = wave / WCO, wco = wave - wci * WCO;
  const int Cin = d.Cin, Cout = d.Cout;
  const int64_t P = (int64_t)d.N * d.Ho * d.Wo;
  const int64_t TC = (P + 63) / 64;
  const int cbn = Cin / TCI, obn = Cout / TCO, nblk = cbn * obn;
  // xmap: XCD-aware order (a pixel split's channel tiles, which read the same X / G chunks, on one XCD)
  const uint32_t bid = xmap ? xcd_logical(blockIdx.x, gridDim.x) : blockIdx.x;
  const int blk = (int)(bid % (uint32_t)nblk), split = (int)(bid / (uint32_t)nblk);
  const int cb = blk / obn, ob = blk - cb * obn;
  const int64_t c0 = TC * split / nsplit, c1 = TC * (split + 1) / nsplit;
  const int nc = (int)(c1 - c0);
  typedef __attribute__((address_space(3))) int8_t lds_i8;
  const uint32_t lbase = (uint32_t)(uintptr_t)(lds_i8*)lds;
  const bool do_ax = wco == 0, do_ag = wci == 0;
  // transposed-read offsets: lane group q supplies k = pixels 8q .. 8q+7 (first read), 32 + 8q .. (second)
  const int pa = 8 * q + (j >> 1);
  const int oa = pa * 16 + 8 * (j & 1), ob2 = oa + 32 * 16;
  const uint32_t hwo = (uint32_t)d.Ho * d.Wo;
  const bool unit = d.SH == 1 && d.SW == 1 && d.Ho == d.H && d.Wo == d.W;

  auto issue = [&](int k, int st) {
    const int64_t p = (c0 + k) * 64 + lane;
    const bool pv = p < P;
    const uint32_t pu = (uint32_t)(pv ? p : 0);
    uint32_t xp = pu;
    if (!unit) {
      const uint32_t n = pu / hwo, rem = pu - n * hwo, oh = rem / (uint32_t)d.Wo, ow = rem - oh * (uint32_t)d.Wo;
      xp = (n * (uint32_t)d.H + oh * (uint32_t)d.SH) * (uint32_t)d.W + ow * (uint32_t)d.SW;
    }
    int8_t* sb = lds + st * STG;
    const int8_t* xs = xq + (int64_t)xp * Cin + cb * TCI;
#pragma unroll
    for (int u = 0; u < NXW; ++u) {
      const int sl = wave + 8 * u;
      const bool real = sl < NXS;
      const int8_t* src = (pv && real) ? xs + sl * 16 : reinterpret_cast<const int8_t*>(kFill80);
      int8_t* dst = real ? sb + sl * 1024 : dummy;
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)dst, 16, 0, 0);
    }
    const int8_t* gs = reinterpret_cast<const int8_t*>(gq + (int64_t)pu * Cout + ob * TCO);
#pragma unroll
    for (int u = 0; u < NGW; ++u) {
      const int g = wave + 8 * u;
      const int8_t* src = pv ? gs + g * 16 : reinterpret_cast<const int8_t*>(zi());
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)(sb + (NXS + g) * 1024), 16, 0, 0);
    }
  };

  v4i acc[4][4], ax[4], ag[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    ax[a] = v4i{0, 0, 0, 0};
    ag[a] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = v4i{0, 0, 0, 0};
  }
  const v4i ones = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const int lox = (j & 1) ? 0 : (int)0x80808080u;  // lo-byte columns: lo' = lo ^ 0x80

  auto mma = [&](int k) {
    const uint32_t sb = lbase + (uint32_t)((k % S) * STG);
    v4i af[4], bf[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t g = sb + (uint32_t)((NXS + wco * 4 + b) * 1024);
      bf[b] = tr_frag_asm(g + oa, g + ob2);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const uint32_t x = sb + (uint32_t)((wci * 4 + a) * 1024);
      af[a] = tr_frag_asm(x + oa, x + ob2);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      tr_wait(bf[b]);
      bf[b] = bf[b] ^ v4i{lox, lox, lox, lox};
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) tr_wait(af[a]);
    if (do_ag) {
#pragma unroll
      for (int b = 0; b < 4; ++b) ag[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bf[b], ag[b], 0, 0, 0);
    }
    if (do_ax) {
#pragma unroll
      for (int a = 0; a < 4; ++a) ax[a] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[a], ones, ax[a], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[a], bf[b], acc[a][b], 0, 0, 0);
  };

  if (nc > 0) {
#pragma unroll
    for (int k = 0; k < S - 1; ++k) issue(k < nc ? k : nc - 1, k);
    for (int k = 0; k < nc; ++k) {
      vm_wait<(S - 2) * G1>();       // chunk k landed (this wave's part)
      __builtin_amdgcn_s_barrier();  // every wave's part of chunk k; chunk k - 1's readers done
      const int nx = k + S - 1;
      issue(nx < nc ? nx : nc - 1, nx % S);
      mma(k);
    }
    vm_wait<0>();  // no DMA may still write LDS when the workgroup ends
  }
  // ---- sums to every wave; lo lanes (even columns) join their hi partner and store
  if (do_ax && j == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) sax[(wci * 4 + a) * 16 + 4 * q + i] = ax[a][i];
  }
  if (do_ag && q == 0) {
#pragma unroll
    for (int b = 0; b < 4; ++b) sag[(wco * 4 + b) * 16 + j] = ag[b][0];
  }
  __syncthreads();
  const long long npix = (long long)nc * 64;
  long long* dst = slab + (int64_t)split * Cin * Cout;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int colg = (wco * 4 + b) * 16 + (j & ~1);  // this pair's lo column in the tile
    const long long sgc = 256ll * sag[colg + 1] + (long long)sag[colg] + 128ll * npix;  // sum_p g[co]
    const int co = ob * TCO + (wco * 4 + b) * 8 + (j >> 1);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int hi = __shfl_xor(acc[a][b][i], 1, 64);
        const int cl = (wci * 4 + a) * 16 + 4 * q + i;
        const long long v = 256ll * hi + (long long)acc[a][b][i] + 128ll * sax[cl] + 128ll * sgc;
        if (!(j & 1)) dst[(int64_t)(cb * TCI + cl) * Cout + co] = v;
      }
  }
}

// the 1x1 body's tile: 0 = not taken, else WCI (waves along ci; 8 / WCI along co)
int wgrad1_wci(const lbt_conv_desc& d) {
  if (d.KH != 1 || d.KW != 1 || d.PT || d.PL || d.PB < 0 || d.PR < 0 || (d.Ho - 1) * d.SH >= d.H ||
      (d.Wo - 1) * d.SW >= d.W)
    return 0;
  if (d.Cin % 128 == 0 && d.Cout % 128 == 0) return 2;
  if (d.Cin % 64 == 0 && d.Cout % 256 == 0) return 1;
  if (d.Cin % 256 == 0 && d.Cout % 64 == 0) return 4;
  return 0;
}

template <int WCI>
void wgrad1_launch(const int8_t* xq, const int16_t* gq, const lbt_conv_desc& d, long long* slab, int nsplit,
                   hipStream_t st) {
  constexpr int S = 3, WCO = 8 / WCI;
  constexpr size_t shm = (size_t)S * (4 * WCI + 4 * WCO) * 1024 + 1024;
  const int64_t nblk = (int64_t)(d.Cin / (64 * WCI)) * (d.Cout / (32 * WCO));
  // LBT_WGRAD_XCD (default 1): bit 0 the XCD-aware order for this 1x1 body -- its pixel split's channel
  // tiles share one XCD's L2 for their X / G chunks (ResNet-50 weight gradients 5.33 -> 5.19 ms per step;
  // bit 1, the same for the 3x3 body, measured no change: profiles/round5/wgrad_xcd_ab.txt)
  static const int xmap = getenv_int("LBT_WGRAD_XCD", 1) & 1;
  launch_dyn_lds<&wgrad1_kernel<WCI, S>>(dim3((unsigned)(nblk * nsplit)), dim3(512), shm, st, xq, gq, d, slab, nsplit,
                                         xmap);
}

}  // namespace

// wide wgrad: x offset int8 codes (q - 128), g int8 (g_i16 = 0) or int16 codes; adds into a
// ZEROED int64 slab [nshard][KH*KW*Cin][Cout] (reduce with lbt_conv_wgrad_reduce64 over nshard).
extern "C" int lbt_conv_wgrad_igemm(const int8_t* xq, const void* gq, int32_t g_i16, lbt_conv_desc d, int64_t* slab,
                                    int32_t nsplit, int32_t nshard, void* stream) {
  if (!desc_ok(d) || d.Cin % 64 || d.Cout % 64 || nsplit <= 0 || nshard <= 0 || nshard > nsplit) return LBT_EINVAL;
  const int64_t P = (int64_t)d.N * d.Ho * d.Wo;
  if (P >= ((int64_t)1 << 31)) return LBT_EINVAL;
  const int64_t nwg = (int64_t)d.KH * d.KW * (d.Cin / 64) * (d.Cout / 64) * nsplit;
  if (nwg > 0x7fffffff) return LBT_EINVAL;
  const dim3 grid((unsigned)nwg);
  static const int xmap = getenv_int("LBT_WGRAD_XMAP", 0);
  hipStream_t st = (hipStream_t)stream;
  if (g_i16)
    hipLaunchKernelGGL((wgrad_wide_kernel<true, false>), grid, dim3(kT), 0, st, xq, gq, d, (long long*)slab, P, nsplit,
                       nshard, xmap);
  else
    hipLaunchKernelGGL((wgrad_wide_kernel<false, false>), grid, dim3(kT), 0, st, xq, gq, d, (long long*)slab, P, nsplit,
                       nshard, xmap);
  return (int)hipGetLastError();
}

// ... storing: slab [nsplit][KH*KW*Cin][Cout] is fully WRITTEN (one partial per pixel split; no
// zeroing, no atomics); reduce with lbt_conv_wgrad_reduce64 over nsplit.
extern "C" int lbt_conv_wgrad_igemm_store(const int8_t* xq, const void* gq, int32_t g_i16, lbt_conv_desc d,
                                          int64_t* slab, int32_t nsplit, void* stream) {
  if (!desc_ok(d) || d.Cin % 64 || d.Cout % 64 || nsplit <= 0) return LBT_EINVAL;
  const int64_t P = (int64_t)d.N * d.Ho * d.Wo;
  if (P >= ((int64_t)1 << 31)) return LBT_EINVAL;
  if ((P + nsplit - 1) / nsplit > 4 * 131072) return LBT_EINVAL;  // int32 MFMA sums of a wave stay exact
  hipStream_t st = (hipStream_t)stream;
  static const int w3 = getenv_int("LBT_WGRAD3", 1);
  if (w3 && wgrad3_ok(d)) {  // 3x3 / stride 1: all taps per workgroup; splits over whole-row chunks
    const int RB = 64 / d.W;
    const int64_t chunks = (int64_t)d.N * ((d.H + RB - 1) / RB);
    const int64_t nblk = (int64_t)(d.Cin / 64) * (d.Cout / 64);
    // <= 1024 chunks a split: every int32 MFMA sum stays below 2^31 (64 products of |x' g| <= 2^14 a chunk)
    if (nsplit > chunks || (chunks + nsplit - 1) / nsplit > 1024 || nblk * nsplit > 0x7fffffff) return LBT_EINVAL;
    const dim3 grid((unsigned)(nblk * nsplit));
    static const int dbg = getenv_int("LBT_WGRAD3_DBG", 0);  // diagnostics: 1 = no DMA after the prologue
    const int win = (RB + 2) * (d.W + 2);
    const bool two = 4 * ((win + 63) / 64) > 8;  // X DMA instructions per wave per chunk: 1 or 2
    long long* sl = (long long*)slab;
    if (g_i16) {
      if (two) wgrad3_launch<true, 2>(xq, gq, d, sl, nsplit, grid, dbg, st);
      else wgrad3_launch<true, 1>(xq, gq, d, sl, nsplit, grid, dbg, st);
    } else {
      if (two) wgrad3_launch<false, 2>(xq, gq, d, sl, nsplit, grid, dbg, st);
      else wgrad3_launch<false, 1>(xq, gq, d, sl, nsplit, grid, dbg, st);
    }
    return (int)hipGetLastError();
  }
  static const int w1 = getenv_int("LBT_WGRAD1", 1);
  if (w1 && g_i16 && wgrad1_wci(d)) {  // 1x1, 16-bit G: (64 WCI) ci x (32 WCO) co workgroup tiles
    const int wci = wgrad1_wci(d);
    const int64_t chunks = (P + 63) / 64;
    const int64_t nblk = (int64_t)(d.Cin / (64 * wci)) * (d.Cout / (256 / wci));
    // <= 2047 chunks a split: every int32 MFMA sum stays below 2^31 (|x' g| <= 2^14 a pixel; 2048
    // chunks of saturated codes, x' = -128 and both G bytes -128, would reach 2^31 exactly)
    if (nsplit > chunks || (chunks + nsplit - 1) / nsplit > 2047 || nblk * nsplit > 0x7fffffff) return LBT_EINVAL;
    const int16_t* g16 = reinterpret_cast<const int16_t*>(gq);
    long long* sl = (long long*)slab;
    if (wci == 2) wgrad1_launch<2>(xq, g16, d, sl, nsplit, st);
    else if (wci == 1) wgrad1_launch<1>(xq, g16, d, sl, nsplit, st);
    else wgrad1_launch<4>(xq, g16, d, sl, nsplit, st);
    return (int)hipGetLastError();
  }
  const int64_t nwg = (int64_t)d.KH * d.KW * (d.Cin / 64) * (d.Cout / 64) * nsplit;
  if (nwg > 0x7fffffff) return LBT_EINVAL;
  const dim3 grid((unsigned)nwg);
  static const int xmap = getenv_int("LBT_WGRAD_XMAP", 0);
  if (g_i16)
    hipLaunchKernelGGL((wgrad_wide_kernel<true, true>), grid, dim3(kT), 0, st, xq, gq, d, (long long*)slab, P, nsplit,
                       nsplit, xmap);
  else
    hipLaunchKernelGGL((wgrad_wide_kernel<false, true>), grid, dim3(kT), 0, st, xq, gq, d, (long long*)slab, P, nsplit,
                       nsplit, xmap);
  return (int)hipGetLastError();
}
