// decoder_plan.hpp -- a pass of the decoder as a plan: every launch of a forward or a VJP is decided and sized first
// (Planner::forward, Planner::backward: an ordered list of steps), then launched as it stands (launch_plan).  Each
// decision is written once, here; sdfr_decoder_launch_plan answers from the same planners.  Included by decoder.hip
// behind its kernels (same translation unit): the only HIP calls of the planners are the two queries of kernel_caps.
#pragma once

namespace {
constexpr int kFcSamples = 8;                 // samples per workgroup of fc_stack_batch_kernel
constexpr size_t kFusedLdsMax = 150 * 1024;   // few latents: layer pairs as one launch each (decoder_fused.hpp)
constexpr int kPlanSteps = 96;                // a pass of 16 layers: at most 5 launches per layer + 8 around them

// conv3d_mfma_kernel's split-K form: for launches with so few tiles that a wave's K loop is the critical path
int use_split_k(bool zgrp, int n_tiles, int co_tiles, int N, int kpad) {
  // (the choice does not depend on N up to 16 samples: small batches decode bit-identically to single latents)
  return (!zgrp && (long long)n_tiles * co_tiles <= SDFR_SPLITK_MAX_TILES && N <= SDFR_SPLITK_MAX_LATENTS && kpad >= 128) ? 1 : 0;
}

// What the runtime says about a kernel, asked once per kernel: its dynamic-LDS limit (MaxDynamicSharedMemorySize) raised
// to `lds_bytes` -- above 64 KiB it must be; `lds_bytes` + the kernel's static LDS <= 160 KiB; false: the runtime
// refused, and the planner takes the other form -- and, where asked for, the waves per SIMD its registers allow (0:
// unknown).  Keyed by the kernel alone: the first answer holds for every device of the process.  (Per-device keying is
// a change to this key -- the pair (device, fn) -- and to nothing else.)
struct KernelCaps { bool lds_raised; int waves; };
KernelCaps kernel_caps(const void* fn, size_t lds_bytes, bool want_waves = false) {
  static std::map<const void*, KernelCaps> known;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find(fn);
  if (it == known.end()) {
    const bool ok = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
    if (!ok) (void)hipGetLastError();   // (not an error of the call that asked: it takes the other form)
    it = known.emplace(fn, KernelCaps{ok, -1}).first;
  }
  KernelCaps& c = it->second;
  if (want_waves && c.waves < 0) {
    hipFuncAttributes fa;
    c.waves = 0;
    if (c.lds_raised && hipFuncGetAttributes(&fa, fn) == hipSuccess)
      c.waves = std::max(1, std::min(8, 512 / ((std::max(fa.numRegs, 1) + 7) / 8 * 8)));
  }
  return c;
}

// The instantiation a step's selectors name, for the planner (kernel_caps) and the launcher alike
using ResizeTFn = decltype(&resize3_backward_tiled_kernel<0, 6>);
ResizeTFn resize_t_fn(int mix, int taps) {   // mix: channels of the 1x1x1 layer (0: none); taps: 6, 8 or 12
  ResizeTFn fn = nullptr;
  dispatch_int_else_last<0, 1, 2, 3, 4>(mix, [&](auto co) { dispatch_int_else_last<6, 8, 12>(taps, [&](auto t) {
    fn = &resize3_backward_tiled_kernel<decltype(co)::value, decltype(t)::value>;
  }); });
  return fn;
}
using StageFn = decltype(&vjp_stage_kernel<0, 6, 0, true>);
StageFn vjp_stage_fn(int mix, int taps, int mode, int zin) {
  StageFn fn = nullptr;
  // (only the stage without a channel mix has a form that starts behind its producer's z pass)
  dispatch_int_else_last<0, 1, 2, 3, 4>(mix, [&](auto co) { dispatch_int_else_last<6, 12>(taps, [&](auto t) {
    dispatch_int_else_last<0, 4, 1>(mode, [&](auto md) {
      constexpr int CO = decltype(co)::value, T = decltype(t)::value, M = decltype(md)::value;
      fn = &vjp_stage_kernel<CO, T, M, true>;
      if constexpr (CO == 0) { if (!zin) fn = &vjp_stage_kernel<CO, T, M, false>; }
    });
  }); });
  return fn;
}
using MfmaUpFn = decltype(&conv3d_mfma_up_kernel<4>);
MfmaUpFn mfma_up_fn(int wpt) { return wpt == 4 ? &conv3d_mfma_up_kernel<4> : &conv3d_mfma_up_kernel<1>; }

// the source ranges of the resize n_in -> n_out: kept per decoder at creation; any other pair is computed into `local`
const ResizeSources* find_resize_sources(const sdfr_decoder* d, int n_in, int n_out) {
  for (const ResizeSources& r : d->rs_src)
    if (r.n_in == n_in && r.n_out == n_out) return &r;
  return nullptr;
}
const ResizeSources& resize_sources_of(const sdfr_decoder* d, int n_in, int n_out, ResizeSources& local) {
  if (const ResizeSources* r = find_resize_sources(d, n_in, n_out)) return *r;
  local = host_resize_sources(n_in, n_out);
  return local;
}

// The direct convolution is for batches (enough tiles to fill the chip).  Does a layer / batch qualify for it, and with
// which tile?  (n: input size, m: output size)  Asked once per layer and pass (Planner::direct).
struct DirectTile { bool ok = false; int TX = 0, TY = 0, ZC = 0, tiles = 0; };   // columns per workgroup, threads per column, tiles
DirectTile direct_tile(size_t w_off, int n, int m, int N) {
  DirectTile t;
  if (w_off == 0 || n > 64 || m < 4) return t;
  const int ZC = (m + 3) / 4;                       // z chunks of 4 outputs per column
  int zc_pow = 1;
  while (zc_pow < ZC) zc_pow <<= 1;                 // threads per column (power of two <= 16)
  if (zc_pow > 16) return t;
  const int cols = 256 / zc_pow;                    // columns per workgroup, at most
  // TX x TY <= cols columns per workgroup: the fewest tiles, then the smallest staged patch (30^3 outputs: 5 x 6
  // columns cover them exactly in 30 tiles of 7 x 8 patch columns; the power-of-two 4 x 8 takes 32 tiles of 6 x 10)
  int TX = 1, TY = cols;
  long long best = -1;
  for (int a = 1; a <= std::min(cols, m); ++a) {
    const int b = std::min(cols / a, m);
    const long long tiles = (long long)((m + a - 1) / a) * ((m + b - 1) / b);
    const long long cost = tiles * 4096 + (a + 2) * (b + 2);
    if (best < 0 || cost < best) { best = cost; TX = a; TY = b; }
  }
  const int tiles = ((m + TX - 1) / TX) * ((m + TY - 1) / TY);
  // enough workgroups to fill the chip -- or, for the handful of latents of a multi-object frame (8 ... 31: K objects
  // side by side), a layer of at least 15 tiles from 240 workgroups on: decoder N = 16 forward 162 -> 97 us, the 8- and
  // 16-object loops +8 % / +24 % objects per second; single latents, small layers and big batches keep their forms
  // (measured with the plain 240 threshold: N = 1 VJP 123 -> 160 us, N = 256 403 -> 453 us)
  const long long wgs = (long long)tiles * N;
  if (wgs < SDFR_DIRECT_MIN_TILES && !(N >= SDFR_DIRECT_MIN_LATENTS_FEW && tiles >= 15 && wgs >= SDFR_DIRECT_MIN_TILES_FEW)) return t;
  t.ok = true; t.TX = TX; t.TY = TY; t.ZC = zc_pow; t.tiles = tiles;
  return t;
}

// Where a step reads or writes: a tensor of the caller's, a slot of the tape, one of the two workspace buffers
struct Slot {
  enum Kind { kNone, kOut, kGrad, kTapeFc, kTapeConv, kBuf } kind = kNone;
  int i = 0;   // kTapeConv: the layer; kBuf: buffer 0 / 1
  bool operator==(const Slot& o) const { return kind == o.kind && i == o.i; }
};
// One launch.  The fields a form does not use stay 0.
struct Step {
  int form, layer;          // SDFR_DECODER_STEP_*; the convolution layer it serves (-1: the Linear stack, the volume)
  Slot src, dst, aux;       // aux: the mask or activation read besides src, or the second tensor written
  unsigned grid[3]; int threads; size_t lds;
  int sel[2];               // template selectors besides the channel counts (per form: see launch_plan)
  int C, CO, mix;           // channels in, out; those of the 1x1x1 layer applied with it (0: none)
  int ni, n, m, pz, pad, relu, clamp;   // sizes: coarse (in front of a resize), input, output; z-row pitch, zero padding written
  int TX, TY, ZC, CK, FX;   // tile (ZC: threads per column, or z tiles), channels per round, widest source range
  int kpad, zg, split, tw;  // the MFMA forms
  int items, per, slots, span, tc;   // the tiled resizes
  int taps, mode, zin, e_nin, scaled;   // the VJP stage (VjpStage)
  size_t outer, inner;      // the single-axis transposed resizes
};
struct Plan {
  int n = 0;
  const char* error = nullptr;   // why the pass cannot run (nothing is launched then)
  Slot t_mid;                    // VJP: where the gradient w.r.t. the wide Linear layer's input lies
  FcDesc fd;
  Step s[kPlanSteps];
};
// the facts a plan depends on besides the handle and N
struct Facts {
  bool tape = false, clamp = false;   // forward: a taped one; enforce_tsdf with a truncation value
  int stages = 3;                     // forward: 1 the Linear stack, 2 the convolutional part, 3 both
  bool deferred = false;              // VJP: the last launch is left to the caller
  int views = 0;                      // VJP: the scaled form's view count (0: not the scaled form)
  unsigned out_mod = 0, tape_mod = 0, grad_mod = 0;   // the caller's pointers modulo 16 bytes
};

struct Planner {
  const sdfr_decoder* const d; const int N; const Facts f; const bool vjp;
  const int opt_resize, opt_tiled, opt_single;   // every option is read once, here (opt_fc_one_wave: one_wave)
  bool one_wave;
  DirectTile direct[16];   // per layer: this pass's direct convolution
  Plan plan;
  int cur = 0;             // forward: the buffer that holds the activation; VJP: the free one

  Planner(const sdfr_decoder* dec, int n, const Facts& facts, bool is_vjp)
      : d(dec), N(n), f(facts), vjp(is_vjp), opt_resize(dec->opt_fused_resize.load(std::memory_order_relaxed)),
        opt_tiled(dec->opt_tiled_vjp.load(std::memory_order_relaxed)),
        opt_single(dec->opt_fused_single.load(std::memory_order_relaxed)) {
    decoder_fc_desc(d, &plan.fd, nullptr, nullptr);
    one_wave = decoder_fc_one_wave(d, plan.fd);
    for (int l = 0; l < d->n_conv; ++l) {
      const int k = d->conv_k[l], nin = d->conv_in_size[l], m = nin - k + 1;
      direct[l] = vjp ? direct_tile(d->bwd_direct_off[l], m + 2 * (k - 1), nin, N) : direct_tile(d->fwd_direct_off[l], nin, m, N);
    }
  }
  int out_n(int l) const { return d->conv_in_size[l] - d->conv_k[l] + 1; }   // size of the tensor layer l produces
  Slot tape_conv(int l) const { return Slot{Slot::kTapeConv, l}; }
  Slot scratch() const { return Slot{Slot::kBuf, vjp ? cur : cur ^ 1}; }     // the buffer a step may write
  // a slot's address modulo 16 bytes: the workspace is 256-byte aligned by construction, the rest follows from N
  unsigned mod16(Slot s) const {
    const size_t per = s.kind == Slot::kTapeFc ? d->tape_fc_off : s.kind == Slot::kTapeConv ? d->tape_conv_off[s.i]
                       : s.kind == Slot::kBuf ? s.i * (vjp ? d->max_bwd : d->max_act) : 0;
    const unsigned base = s.kind == Slot::kOut ? f.out_mod : s.kind == Slot::kGrad ? f.grad_mod
                          : (s.kind == Slot::kTapeFc || s.kind == Slot::kTapeConv) ? f.tape_mod : 0;
    return (unsigned)((base + (size_t)N * per * sizeof(float)) & 15);
  }
  Step& add(int form, int layer, Slot src, Slot dst, unsigned gx, unsigned gy, unsigned gz, int threads, size_t lds = 0) {
    if (plan.n == kPlanSteps) { plan.error = "more launches than a plan holds (internal)"; --plan.n; }
    Step& s = plan.s[plan.n++] = Step{};
    s.form = form; s.layer = layer; s.src = src; s.dst = dst;
    s.grid[0] = gx; s.grid[1] = gy; s.grid[2] = gz; s.threads = threads; s.lds = lds;
    if (dst == scratch()) cur ^= 1;
    return s;
  }

  // ---- the launches both passes share -------------------------------------------------------------------------------
  // conv3d_mfma_kernel in the form the layer / batch takes (plain, z-grouped, split-K, input resident in LDS)
  void mfma(int l, Slot src, Slot dst, int cin, int cout, int n, int m, int relu) {
    const sdfr_decoder::ZPlan& zp = vjp ? d->bwd_z[l] : d->fwd_z[l];
    const int kpad = vjp ? d->bwd_kpad[l] : d->conv_kpad[l];
    // (a single decode is latency-bound: there the finer grid of the ungrouped form wins)
    // (up to 16 samples the split-K form decides, so that small batches equal single decodes bit for bit)
    const int split = use_split_k(false, (m * m * m + 15) / 16, (cout + 15) / 16, N, kpad);
    const bool zgrp = !split && zp.zg > 1 && !d->conv_swap[l] && (long long)m * m * (m / zp.zg) * N >= kZGroupMinRows;
    const int kp = zgrp ? zp.kpad : kpad, zg = zgrp ? zp.zg : 1, nt = (m * m * (m / zg) + 15) / 16;
    const int co_tiles = zgrp ? 1 : (cout + 15) / 16, tw = nt >= 32768 ? 4 : 1;
    const size_t in_floats = (size_t)cin * n * n * n, lds_res = ((size_t)kp * 17 + in_floats) * sizeof(float);
    // (resident: the whole grid is then N * co_tiles workgroups -- only where that still fills the chip)
    const bool resident = !split && zg == 1 && N * co_tiles >= 128 && nt >= 8 && nt <= 64 && lds_res <= 120 * 1024 &&
                          (in_floats & 3) == 0 && mod16(src) == 0 &&
                          kernel_caps(reinterpret_cast<const void*>(&conv3d_mfma_kernel<true>), 120 * 1024).lds_raised;
    const int form = zgrp ? SDFR_DECODER_STEP_MFMA_Z_GROUPED : split ? SDFR_DECODER_STEP_MFMA_SPLIT_K : SDFR_DECODER_STEP_MFMA;
    Step& s = resident ? add(SDFR_DECODER_STEP_MFMA_RESIDENT, l, src, dst, 1, co_tiles, N, 256, lds_res)
                       : add(form, l, src, dst, split ? nt : (nt + 4 * tw - 1) / (4 * tw), co_tiles, N, 256,
                             (size_t)kp * 17 * sizeof(float) + (split ? 4096 : 0));
    s.C = cin; s.CO = cout; s.n = n; s.m = m; s.kpad = kp; s.relu = relu;
    s.tw = resident ? 1 : tw; s.zg = resident ? 1 : zg; s.split = split;
  }
  // conv3d_direct_kernel: false where the layer / batch does not qualify.  pz: floats between the z-rows of src (n, or
  // more: the padded tensors of the VJP); mix_out: the 1x1x1 layer l + 1 is applied in the epilogue and written there
  bool direct_conv(int l, Slot src, Slot dst, int cin, int cout, int n, int pz, int m, int relu, Slot mix_out = Slot{}) {
    const DirectTile& t = direct[l];
    if (!t.ok) return false;
    // channels per LDS chunk: patch of CK channels <= 24 KB
    const int per_ch = (t.TX + 2) * (t.TY + 2) * ((pz + 3) & ~3);   // (LDS rows are padded to 16 bytes)
    const int CK = std::max(1, std::min(cin, (24 * 1024 / 4) / per_ch));
    // 16-byte loads: runs start and end on 16-byte boundaries, offsets and channel fit the packed word of the prefetch
    const bool vec4 = (pz & 3) == 0 && mod16(src) == 0 && (size_t)CK * n * n * pz < 0xffffff && CK < 127;
    if (!vec4 && pz != n) return false;   // (the scalar-load form takes dense rows only; rows are padded only to 16 bytes)
    const size_t lds = ((size_t)CK * per_ch + 8) * sizeof(float);   // (+ the over-read of the last z-run)
    Step& s = add(SDFR_DECODER_STEP_DIRECT, l, src, dst, t.tiles, 1, N, 256, lds);
    s.aux = mix_out; s.mix = mix_out.kind != Slot::kNone ? d->conv_cout[l + 1] : 0;
    if (s.mix) cur ^= 1;   // (mix_out is the free buffer)
    s.sel[0] = vec4; s.C = cin; s.CO = cout; s.n = n; s.pz = pz; s.m = m; s.relu = relu;
    s.TX = t.TX; s.TY = t.TY; s.ZC = t.ZC; s.CK = CK;
    return true;
  }
  // layer l's convolution as it lies (forward), or its transposed one (VJP: the channels swap roles)
  void conv(int l, Slot src, Slot dst, int cin, int cout, int n, int pz, int m, int relu) {
    if (d->conv_k[l] == 1 && cout <= 4) {
      // element-wise (the MFMA form of the transposed layer: 207 us per 256 latents, this: ~35)
      const int voxn = n * n * n;
      const bool v4 = !vjp && N >= 32 && (voxn & 3) == 0 && ((mod16(src) | mod16(dst)) & 15) == 0;
      Step& s = add(v4 ? SDFR_DECODER_STEP_CONV1X1_VEC4 : SDFR_DECODER_STEP_CONV1X1, l, src, dst,
                    ((v4 ? voxn / 4 : voxn) + 255) / 256, N, 1, 256);
      s.C = cin; s.CO = cout; s.n = n; s.relu = relu;
    } else if (!d->conv_swap[l] && direct_conv(l, src, dst, cin, cout, n, pz, m, relu)) {
      // (batched: direct VALU convolution)
    } else if (pz != n) {
      plan.error = "padded rows without the direct convolution (internal)";
    } else {
      mfma(l, src, dst, cin, cout, n, m, relu);
    }
  }

  // ---- forward ----------------------------------------------------------------------------------------------------------
  void resize(int l, Slot src, int C, int ni, int no, int relu, bool clamp, Slot dst) {
    // input columns under an 8 x 8 output patch, worst tile
    const int max_r = host_resize_span(ni, no, no, kResizeTile, kResizeTile);
    const size_t lds = ((size_t)max_r * max_r * (ni + no) + 3) * sizeof(float);   // (+3: the second array starts 16-byte aligned)
    const int tiles = (no + kResizeTile - 1) / kResizeTile;
    const bool pow2 = no >= 16 && no <= 128 && (no & (no - 1)) == 0;
    // (a single decode has too few tiles to fill the chip: the gather kernel is faster there)
    const long long tile_items = (long long)tiles * tiles * C * N;
    if (pow2 && ni <= no && lds <= 48 * 1024 && (long long)C * N < (1ll << 30) && tile_items >= SDFR_RESIZE_TILED_MIN_ITEMS) {
      // volumes per workgroup: as many as still leave ~8 workgroups per CU
      const int items = C * N;
      // (256 mug latents, us: 14 -> 32 x 8 channels 68.6 / 52.9 / 55.4 / 53.3 at 1 / 2 / 4 / 8 volumes per workgroup,
      // 30 -> 64 x 1 channel 68.5 / 60.3 / 55.8 / 63.6 -- profiles/r04_decoder_resize_ipw.txt; before this form 70.8 / 66.7)
      const int ipw = std::max((int)std::max<long long>(1, std::min<long long>(4, tile_items / 2048)), (items + 65534) / 65535);
      Step& s = add(SDFR_DECODER_STEP_RESIZE_TILED, l, src, dst, tiles * tiles, (items + ipw - 1) / ipw, 1, 256, lds);
      s.sel[0] = 4;   // log2 of no (16, 32, 64 or 128)
      while ((1 << s.sel[0]) < no) ++s.sel[0];
      s.sel[1] = mod16(dst) == 0;
      s.items = items; s.per = ipw; s.span = max_r * max_r;
      s.ni = ni; s.m = no; s.relu = relu; s.clamp = clamp;
      return;
    }
    Step& s = add(SDFR_DECODER_STEP_RESIZE, l, src, dst, (unsigned)(((size_t)C * no * no * no + 255) / 256), N, 1, 256);
    s.C = C; s.ni = ni; s.m = no; s.relu = relu; s.clamp = clamp;
  }
  // resize ni -> in_size folded into layer l's direct convolution (conv3d_direct_up_kernel): same tiling as
  // direct_conv; the chunk is also bounded by the coarse columns a thread prefetches
  bool direct_up(int l, Slot src, Slot dst, int cin, int ni) {
    const int n = d->conv_in_size[l], m = n - 2, cout = d->conv_cout[l];
    if (!opt_resize || n < 16 || n > 64 || (n & (n - 1)) != 0 || ni > n || ni < 2) return false;
    // Measured on 256 mug latents (profiles/r04_decoder_fused_resize.txt): 6 -> 16 in front of the 16 -> 8 layer,
    // 112 us folded against 96 + 26 as two launches; 14 -> 32 in front of the 8 -> 4 layer, 268 us folded against
    // 170 + 77 -- there the patch's 1.87x overlap makes every workgroup interpolate what its neighbours interpolate
    // too, in a kernel that is VALU-bound already.  So: folded up to a fine size of 16 (mode 2, the tests': always).
    if (opt_resize == 1 && n > 16) return false;
    const DirectTile& t = direct[l];
    const int IX = t.TX + 2, IY = t.TY + 2;
    if (!t.ok || IX > 34 || IY > 34 || (cout != 4 && cout != 8 && cout != 16)) return false;
    // coarse columns under a patch, worst tile (the kernel's float arithmetic)
    const int max_cols = host_resize_span(ni, n, m, t.TX, IX) * host_resize_span(ni, n, m, t.TY, IY);
    const int per_ch = IX * IY * n;
    int CK = std::max(1, std::min(cin, (24 * 1024 / 4) / per_ch));
    CK = std::min(CK, 2048 / (max_cols * ni));      // <= 8 prefetched values per thread
    if (CK < 1 || CK >= 127 || (size_t)CK * ni * ni * ni >= 0xffffff) return false;
    const size_t lds = ((size_t)CK * per_ch + 8 + (size_t)CK * max_cols * ni) * sizeof(float);
    if (lds > 60 * 1024) return false;
    Step& s = add(SDFR_DECODER_STEP_DIRECT_UP, l, src, dst, t.tiles, 1, N, 256, lds);
    while ((1 << s.sel[0]) < n) ++s.sel[0];   // log2 of n
    s.C = cin; s.CO = cout; s.ni = ni; s.n = n; s.m = m; s.relu = d->conv_relu[l];
    s.TX = t.TX; s.TY = t.TY; s.ZC = t.ZC; s.CK = CK; s.span = max_cols;
    return true;
  }
  // few latents: resize ni -> in_size + layer l's 3x3x3 convolution in one launch (conv3d_mfma_up_kernel), only where
  // the unfused convolution takes its split-K form (the arithmetic this kernel reproduces).  mix_out: the swapped
  // 1x1x1 layer l + 1 in the epilogue as well (at most 16 channels into it: one column tile).
  bool mfma_up(int l, Slot src, Slot dst, int cin, int ni, Slot mix_out) {
    const int n = d->conv_in_size[l], m = n - 2, cout = d->conv_cout[l], kpad = d->conv_kpad[l];
    if (!(opt_single & 1) || ni > n || ni < 1 || m < 1 || direct[l].ok) return false;
    const int co_tiles = (cout + 15) / 16, ZT = (m + 15) / 16;
    if (ZT > 4 || !use_split_k(false, (m * m * m + 15) / 16, co_tiles, N, kpad)) return false;
    int TX, TY;   // columns per workgroup
    few_latent_tile(m, ZT, (long long)co_tiles * N, TX, TY);
    const int tiles = TX * TY * ZT, wpt = 4 * tiles <= 16 ? 4 : 1;
    const int threads = std::max(256, 64 * wpt * tiles);
    const int IX = TX + 2, IY = TY + 2;
    const int CX = std::max({1, host_resize_span(ni, n, m, TX, IX), host_resize_span(ni, n, m, TY, IY)});
    const int PZ = 16 * ZT + 2, patch_n = cin * IX * IY * PZ;
    const size_t zc_n = (size_t)cin * CX * CX * PZ;
    if (zc_n >= 65536 || patch_n >= 65536 || threads / PZ < 1 || threads / (IX * IY) < 1) return false;   // (reciprocal divisions)
    const size_t lds = ((size_t)kpad * 17 + (wpt == 4 ? 4 * threads : 0) + ((patch_n + 3) & ~3) + zc_n) * sizeof(float);
    const void* fn = reinterpret_cast<const void*>(mfma_up_fn(wpt));
    if (lds > kFusedLdsMax || (lds > 64 * 1024 && !kernel_caps(fn, kFusedLdsMax).lds_raised)) return false;
    Step& s = add(SDFR_DECODER_STEP_MFMA_UP, l, src, dst, ((m + TX - 1) / TX) * ((m + TY - 1) / TY), co_tiles, N, threads, lds);
    s.aux = mix_out; s.mix = mix_out.kind != Slot::kNone ? d->conv_cout[l + 1] : 0;
    if (s.mix) cur ^= 1;   // (mix_out is the free buffer)
    s.sel[0] = wpt; s.C = cin; s.CO = cout; s.ni = ni; s.n = n; s.m = m; s.kpad = kpad; s.relu = d->conv_relu[l];
    s.span = CX; s.ZC = ZT; s.TX = TX; s.TY = TY;
    return true;
  }
  // few latents: the Linear stack and the first convolution as one launch (fc_conv_kernel) -- a 3x3x3 layer that is not
  // the last, with a layer behind it that is not a 1x1x1 one swapped with its resize
  bool fc_conv() {
    if (!(opt_single & 2) || f.stages != 3 || d->n_conv < 2 || d->conv_swap[0] || d->conv_k[0] != 3 || d->conv_swap[1] || N >= 32)
      return false;
    const int n = d->conv_in_size[0], m = n - 2, cin = d->conv_cin[0], cout = d->conv_cout[0], kpad = d->conv_kpad[0];
    if (m < 1 || m == d->volume || !one_wave || direct[0].ok) return false;
    const int co_tiles = (cout + 15) / 16, ZT = (m + 15) / 16;
    if (ZT > 4 || !use_split_k(false, (m * m * m + 15) / 16, co_tiles, N, kpad)) return false;
    const int PZ = 16 * ZT + 2, patch_n = cin * 9 * PZ, items = cin * 9 * n;
    if (patch_n >= 65536 || plan.fd.width[plan.fd.n_fc - 1] > kFcWaveWidth) return false;
    // a row of the wide layer per thread where the workgroup size allows
    int threads = 256 * ZT;
    while (threads < 1024 && threads < items) threads *= 2;
    const size_t lds = ((size_t)kpad * 17 + 4 * threads + patch_n) * sizeof(float);
    const void* fn = reinterpret_cast<const void*>(&fc_conv_kernel);
    if (lds > 100 * 1024 || (lds > 38 * 1024 && !kernel_caps(fn, 100 * 1024).lds_raised)) return false;   // (+ 25 KB static)
    Step& s = add(SDFR_DECODER_STEP_FC_CONV, 0, Slot{}, f.tape ? tape_conv(0) : scratch(), m * m, co_tiles, N, threads, lds);
    if (f.tape) s.aux = Slot{Slot::kTapeFc};
    s.C = cin; s.CO = cout; s.n = n; s.m = m; s.kpad = kpad; s.relu = d->conv_relu[0]; s.ZC = ZT;
    return true;
  }
  void fc_stack(Slot dst) {
    const int last = d->fc_out[d->n_fc - 1];
    int hid = d->latent;   // widest input of a layer
    for (int l = 0; l + 1 < d->n_fc; ++l) hid = std::max(hid, d->fc_out[l]);
    const size_t fc_lds = 2 * (size_t)hid * kFcSamples * sizeof(float);
    // batches (small ones keep the form of a single decode)
    const bool batch = N >= 4 * kFcSamples && fc_lds <= 48 * 1024, narrow = one_wave && (!batch || fc_lds <= 32 * 1024);
    const unsigned gx = (last + kFcBlock - 1) / kFcBlock;
    if (batch) add(narrow ? SDFR_DECODER_STEP_FC_STACK_BATCH_NARROW : SDFR_DECODER_STEP_FC_STACK_BATCH, -1, Slot{}, dst, gx,
                   (N + kFcSamples - 1) / kFcSamples, 1, kFcBlock, fc_lds).ni = hid;
    else add(narrow ? SDFR_DECODER_STEP_FC_STACK_NARROW : SDFR_DECODER_STEP_FC_STACK, -1, Slot{}, dst, gx, N, 1, kFcBlock);
  }
  // a swapped 1x1x1 layer takes the one-launch form of single latents: its channel mix inside its resize (resize3_mix_kernel)
  bool few_mix(int l) const {
    const size_t mo = d->conv_in_size[l];
    return d->conv_cout[l] <= 4 && (size_t)N * d->conv_cout[l] * mo * mo * mo <= kFewElementsMix;
  }
  void forward() {
    const int nc = d->n_conv;
    const Slot out{Slot::kOut}, tape_fc{Slot::kTapeFc};
    Slot act = tape_fc;   // (stages == 2: left there by stage 1 -- or by the loop's tail, sdfr_loop_tail_fused)
    int l = 0;
    // with a tape, every ReLU'd layer output goes to its own slot (and is read from there)
    if (f.stages != 2) {
      if (fc_conv()) l = 1;
      else fc_stack(f.tape ? tape_fc : Slot{Slot::kBuf, cur});
      act = plan.s[plan.n - 1].dst;
    }
    if (f.stages == 1) return;
    int c = l ? d->conv_cout[0] : d->conv_cin[0], n = l ? out_n(0) : d->conv_in_size[0];
    // where layer l's output goes: straight to `out` (a last layer of the volume's size with no clamp left to apply),
    // to its tape slot, or to the other buffer
    // (a ReLU'd last layer of a taped forward goes to its tape slot first -- the VJP reads its mask there -- and is
    // copied out: until round 6 it went straight to `out` and the VJP masked with whatever the slot held)
    auto layer_dst = [&](int l, bool no_clamp) {
      const bool to_out = l == nc - 1 && out_n(l) == d->volume && no_clamp && !(f.tape && d->conv_relu[l]);
      return to_out ? out : f.tape ? tape_conv(l) : scratch();
    };
    // a swapped layer's resize behind its convolution: with the layer's ReLU, and the final clamp when this is it
    auto swapped_resize = [&](int l, Slot src, int ni) {
      const Slot dst = layer_dst(l, true);
      resize(l, src, d->conv_cout[l], ni, d->conv_in_size[l], d->conv_relu[l], dst == out && f.clamp, dst);
      return dst;
    };
    for (; l < nc; ++l) {
      const int k = d->conv_k[l], co_n = d->conv_cout[l], nf = d->conv_in_size[l], mf = nf - k + 1;
      if (d->conv_swap[l]) {   // (k == 1: the convolution keeps the incoming size, the resize follows)
        if (few_mix(l)) {
          const Slot dst = layer_dst(l, true);
          Step& s = add(SDFR_DECODER_STEP_RESIZE_MIX, l, act, dst, (unsigned)(((size_t)nf * nf * nf + 255) / 256), N, 1, 256);
          s.C = c; s.CO = co_n; s.ni = n; s.m = nf; s.relu = d->conv_relu[l]; s.clamp = dst == out && f.clamp;
          act = dst;
        } else {
          conv(l, act, scratch(), c, co_n, n, n, n, 0);
          act = swapped_resize(l, plan.s[plan.n - 1].dst, n);
        }
        c = co_n; n = nf;
        continue;
      }
      // a swapped 1x1x1 layer behind this one (the mug decoder's last: 4 -> 1 channels behind the resize to the volume)
      // can be applied in this layer's epilogue: the resize behind it gathers one channel, not four
      const bool mixable = k == 3 && l + 1 < nc && d->conv_swap[l + 1] && d->conv_cout[l + 1] <= 4;
      const Slot dst = layer_dst(l, !f.clamp), taped = f.tape ? tape_conv(l) : Slot{};
      bool mixed = false;
      if (n != nf && k == 3 && direct_up(l, act, dst, c, n)) {
        // (batches: the resize in the patch load, the up-sampled tensor is never written)
      } else if (n != nf && k == 3 && mixable && co_n <= 16 && mfma_up(l, act, taped, c, n, scratch())) {
        mixed = true;   // (resize3_kernel behind it instead of resize3_mix_kernel: bit for bit the same corner values)
      } else if (n != nf && k == 3 && mfma_up(l, act, dst, c, n, Slot{})) {
        // (few latents: the resize inside the split-K MFMA convolution's operand fetch)
      } else {
        if (n != nf) {
          const Slot coarse = act;
          resize(l, coarse, c, n, nf, 0, false, act = scratch());
        }
        // batches: the swapped layer in the direct convolution's epilogue, unless it takes its one-launch form
        const Slot cdst = layer_dst(l, !f.clamp);
        mixed = mixable && !few_mix(l + 1) && direct_conv(l, act, taped, c, co_n, nf, nf, mf, d->conv_relu[l], scratch());
        if (!mixed) conv(l, act, cdst, c, co_n, nf, nf, mf, d->conv_relu[l]);
      }
      const Step& s = plan.s[plan.n - 1];
      act = mixed ? s.aux : s.dst;
      c = co_n; n = mf;
      if (mixed) {   // layer l + 1 is applied but for its resize
        act = swapped_resize(++l, act, n);
        c = d->conv_cout[l]; n = d->conv_in_size[l];
      }
    }
    // behind the last layer: what is not in `out` yet gets there, resized to the volume or copied, and clamped
    if (act == out) return;
    const size_t words = (size_t)N * d->volume * d->volume * d->volume;
    if (n != d->volume) return resize(-1, act, 1, n, d->volume, 0, f.clamp, out);
    add(SDFR_DECODER_STEP_COPY, -1, act, out, (unsigned)((words + 255) / 256), 1, 1, 256).outer = words;
    if (f.clamp) add(SDFR_DECODER_STEP_CLAMP, -1, out, out, (unsigned)((words + 255) / 256), 1, 1, 256).outer = words;
  }

  // ---- VJP ----------------------------------------------------------------------------------------------------------------
  // transpose of a trilinear resize of [N*C] volumes n_out^3 -> n_in^3: z, then y, then x
  // pad >= 0: the last pass also applies the ReLU mask `act` (may be none) and the zero padding of the
  // transposed convolution that follows (resize_x_backward_pad_kernel)
  // Single latents (the captured loop) are bound by the launch count: there the z and y passes share a launch.
  // mix_l >= 0: the x pass also applies the transposed 1x1 layer mix_l, C -> mix_cout channels
  // (resize_x_backward_mix_pad_kernel; needs pad >= 0).
  // pz: floats between the z-rows of the padded tensor written (pad >= 0), >= n_in + 2 pad
  void resize_t(int l, Slot g, int C, int n_in, int n_out, int pad = -1, Slot act = Slot{}, int mix_l = -1, int mix_cout = 0,
                int pz = 0) {
    if (pz == 0) pz = n_in + 2 * std::max(pad, 0);
    const size_t nc = (size_t)N * C;
    ResizeSources local;
    const ResizeSources& rs = resize_sources_of(d, n_in, n_out, local);
    // (n_in <= n_out: the z pass writes a row's n_in results over the row's own n_out sources)
    // (single latents too: one launch of ~9 us instead of two of 6 + 5 in the captured loop, C5 0.144 -> 0.1375 ms)
    // the three passes in one launch on an LDS-staged block (resize3_backward_tiled_kernel): 16-byte loads of g
    if (opt_tiled && (mix_l < 0 || (C == 1 && pad >= 0)) && n_in <= 64 && n_in <= n_out && n_out <= 1024 && nc < (1u << 24) &&
        (n_out & 3) == 0 && mod16(g) == 0 && rs.max_taps <= kBtTaps && rs.max_span <= 16) {
      const int padv = pad >= 0 ? pad : 0;
      // the instantiation: the channels of the 1x1 layer (0: none), the taps that hold the longest exact source range
      const int mix = mix_l < 0 ? 0 : (mix_cout >= 1 && mix_cout <= 3) ? mix_cout : 4;
      const int taps = rs.max_taps <= 6 ? 6 : rs.max_taps <= 8 ? 8 : 12;
      // (a block above 64 KiB of dynamic LDS needs the kernel's limit raised; 0 waves: the runtime refused)
      const int waves_simd = kernel_caps(reinterpret_cast<const void*>(resize_t_fn(mix, taps)), 150 * 1024, true).waves;
      // tile edge and workgroup size: the pair that stages the fewest fine rows over the launch, among those whose
      // block fits the registers of the prefetch (kBtLoads vectors per thread) and leaves two workgroups on a CU
      struct Pick { int tc = 0, threads = 0, max_f = 0, wgs = 0; size_t lds = 0; double cost = 0; } best;
      for (int tc = 2; tc <= std::min(kBtMaxTile, n_in); ++tc) {
        if (SDFR_BT_TILE > 0 && tc != std::min(SDFR_BT_TILE, n_in)) continue;
        int max_f = 1;
        for (int c0 = 0; c0 < n_in; c0 += tc) max_f = std::max(max_f, rs.hi[std::min(c0 + tc, n_in) - 1] - rs.lo[c0] + 1);
        const int tiles = (n_in + tc - 1) / tc;
        const size_t lds = ((size_t)max_f * max_f * n_out + (size_t)max_f * tc * n_in) * sizeof(float);
        if (lds > 150 * 1024) continue;
        for (int threads = 256; threads <= kBtMaxThreads; threads *= 2) {
          if (SDFR_BT_THREADS > 0 && threads != SDFR_BT_THREADS) continue;
          if ((size_t)max_f * max_f * (n_out >> 2) > (size_t)kBtLoads * threads) continue;
          const size_t oc = tiles == 1 ? n_in + 2 * padv : tc + padv;   // columns of the padded tensor a tile writes, per axis
          if (oc * oc * pz > (size_t)kBtOut * threads) continue;
          // workgroups a CU holds (LDS, registers), and the cost: rows staged over the launch, with a charge for a
          // thin CU (few waves to hide the chain of a workgroup behind)
          const int wgs = (int)std::min<size_t>((160 * 1024) / (lds + 6 * 1024), (size_t)(4 * waves_simd) / (threads / 64));
          if (wgs < 1) continue;
          const double waves = (double)wgs * threads / 64;
          const double cost = (double)tiles * tiles * max_f * max_f * (1.0 + 4.0 / waves);
          if (!best.tc || cost < best.cost) { best.tc = tc; best.threads = threads; best.max_f = max_f; best.lds = lds; best.wgs = wgs; best.cost = cost; }
        }
      }
      if (best.tc) {
        const int tiles = (n_in + best.tc - 1) / best.tc, tt = tiles * tiles;
        // channel slots: each workgroup walks over `per` channels (tables and addresses once, the next channel's
        // rows prefetched); `per` so that the workgroups come in whole rounds of what the chip holds
        const long long cap = 256LL * best.wgs;
        int slots = 8;
        double best_t = 0;
        for (int per = 1; per <= 32; ++per) {
          const int sl = (int)(((nc + per - 1) / per + 7) / 8 * 8);
          const long long rounds = ((long long)tt * sl + cap - 1) / cap;
          const double t = (double)rounds * (per + 0.7);   // (+ the set-up of a workgroup, in channels)
          if (per == 1 || t < best_t) { best_t = t; slots = sl; }
        }
        Step& s = add(SDFR_DECODER_STEP_RESIZE_T_TILED, l, g, scratch(), (unsigned)(tt * slots), 1, 1, best.threads, best.lds);
        s.aux = pad >= 0 ? act : Slot{}; s.sel[0] = mix; s.sel[1] = taps; s.mix = mix_l < 0 ? 0 : mix_cout;
        s.ni = n_in; s.m = n_out; s.pad = pad; s.pz = pz; s.tc = best.tc; s.span = best.max_f; s.items = (int)nc; s.slots = slots;
        return;
      }
    }
    // (the z + y launch takes candidate ranges, as resize_sources gives them, up to kZyTaps long)
    const bool few = nc * n_out * n_out * n_out <= kFewElements && rs.max_span <= kZyTaps;
    if (few) {
      Step& s = add(SDFR_DECODER_STEP_RESIZE_T_ZY, l, g, scratch(), (unsigned)((nc * n_out * n_in * n_in + 255) / 256), 1, 1, 256);
      s.outer = nc * n_out; s.ni = n_in; s.m = n_out;
      g = s.dst;
    }
    for (int a = few ? 2 : 0; a < 3; ++a) {
      // z: [nc][no][no][no] -> [nc][no][no][ni], y: -> [nc][no][ni][ni], x: -> [nc][ni][ni][ni]
      const size_t outer = a == 0 ? nc * n_out * n_out : a == 1 ? nc * n_out : nc, inner = a == 0 ? 1 : a == 1 ? n_in : n_in * n_in;
      const int form = a < 2 ? SDFR_DECODER_STEP_RESIZE_T_AXIS : mix_l >= 0 ? SDFR_DECODER_STEP_RESIZE_T_X_MIX_PAD
                       : pad >= 0 ? SDFR_DECODER_STEP_RESIZE_T_X_PAD : SDFR_DECODER_STEP_RESIZE_T_AXIS;
      const bool mixes = form == SDFR_DECODER_STEP_RESIZE_T_X_MIX_PAD;   // (one workgroup row per sample: grid (.., N))
      const size_t np = (size_t)n_in + 2 * std::max(pad, 0);
      const size_t cnt = mixes ? np * np * pz : form == SDFR_DECODER_STEP_RESIZE_T_X_PAD ? nc * np * np * pz : outer * n_in * inner;
      Step& s = add(form, l, g, scratch(), (unsigned)((cnt + 255) / 256), mixes ? N : 1, 1, 256);
      s.C = C; s.mix = mixes ? mix_cout : 0; s.outer = outer; s.inner = inner;
      s.ni = n_in; s.m = n_out; s.aux = act; s.pad = a == 2 ? pad : -1; s.pz = pz;
      g = s.dst;
    }
  }
  // One stage of the VJP for few latents in one launch (vjp_stage_kernel): the transposed resize n_out -> n_in of C
  // channels (+ ReLU mask, + the swapped 1x1x1 layer mix_l, C = 1 -> mix_cout channels, + zero padding) and the transposed
  // convolution of layer lc that reads it; false where the pair keeps its launches.  zin: the stage runs the z pass
  // itself (g is the fine gradient); 0: its producer's epilogue has (g is coarse along z already).
  bool vjp_stage(int lc, Slot g, int C, int n_in, int n_out, int mix_l, int mix_cout, int zin, bool first) {
    // bit 4: the FIRST stage of the VJP (the one that reads the decoder's incoming gradient); bit 8: the stages behind a
    // fused one as well, chained through the z-pass epilogue (measured: no faster than their two launches each)
    if (!(opt_single & (first ? 4 : 8))) return false;
    const int k = d->conv_k[lc], ci_n = d->conv_cin[lc], co_n = d->conv_cout[lc];
    const int CP = mix_cout > 0 ? mix_cout : C;
    if (k != 3 || d->conv_swap[lc] || CP != co_n || (mix_cout > 0 && (C != 1 || mix_cout > 4 || !zin))) return false;
    if (n_in != out_n(lc) || n_in > n_out || n_in > 64) return false;
    if (zin && ((n_out & 3) || mod16(g))) return false;
    // (the tables of this resize: built at creation for the resize in front of layer lc + 1)
    if (lc + 1 >= d->n_conv || d->rs_tab_off[lc + 1] == 0 || d->conv_prev[lc + 1] != n_in || d->conv_in_size[lc + 1] != n_out) return false;
    const int pad = k - 1, np = n_in + 2 * pad, nc = np - 2, kpad = d->bwd_kpad[lc], ci_tiles = (ci_n + 15) / 16;
    // the form the unfused transposed convolution takes: plain or split-K only (not the direct, not the z-grouped one)
    if (N > SDFR_SPLITK_MAX_LATENTS || direct[lc].ok) return false;
    const int split = use_split_k(false, (nc * nc * nc + 15) / 16, ci_tiles, N, kpad);
    const sdfr_decoder::ZPlan& zp = d->bwd_z[lc];
    if (!split && zp.zg > 1 && (long long)nc * nc * (nc / zp.zg) * N >= kZGroupMinRows) return false;
    const int ZT = (nc + 15) / 16;
    if (ZT > 4) return false;
    ResizeSources local;
    const ResizeSources& rs = resize_sources_of(d, n_in, n_out, local);
    if (rs.empty || rs.max_span > 16 || rs.max_taps > kBtTaps) return false;
    const int taps = rs.max_taps <= 6 ? 6 : 12;
    int TX, TY, FX = 0, CK = 0, threads = 0;   // columns per workgroup, widest source range, channels per round
    few_latent_tile(nc, ZT, (long long)ci_tiles * N, TX, TY);
#ifdef SDFR_VJP_TUNE   // timing experiments: tile shape and workgroup size from the environment
    if (const char* e = getenv("SDFR_VJP_TX")) TX = atoi(e);
    if (const char* e = getenv("SDFR_VJP_TY")) TY = atoi(e);
#endif
    const int tiles = TX * TY * ZT, max_thr = zin ? 512 : 1024;   // (vjp_stage_kernel's launch bounds)
    if (64 * tiles > max_thr) return false;
    const int mode = !split ? 0 : (256 * tiles <= max_thr ? 4 : 1);
    const int IX = TX + 2, IY = TY + 2;
    for (int pass = 0; pass < 2; ++pass) {
      const int T = pass ? TY : TX, I = pass ? IY : IX;
      for (int t0 = 0; t0 < nc; t0 += T)
        FX = std::max(FX, rs.hi[std::min(t0 - pad + I - 1, n_in - 1)] - rs.lo[std::max(t0 - pad, 0)] + 1);
    }
    // channels per round and workgroup size: the whole tensor in one round where the LDS allows
    const int PZ = 16 * ZT + 2, patch_n = CP * IX * IY * PZ, RL = zin ? n_out : n_in;
    const int min_thr = std::max(256, mode == 4 ? 256 * tiles : 64 * tiles);
    const size_t epi = (size_t)TX * TY * 16 * nc;   // (the epilogue's rows reuse F)
    size_t lds = 0;
    for (int ck = C; ck >= 1 && !CK; --ck) {
      const size_t f_n = std::max((size_t)ck * FX * FX * RL, epi);
      const size_t units = (size_t)ck * FX * FX * (zin ? RL / 4 : RL);
      threads = min_thr;
      while (threads < max_thr && (size_t)threads * 8 < units) threads *= 2;
#ifdef SDFR_VJP_TUNE
      if (const char* e = getenv("SDFR_VJP_THREADS")) threads = std::max(min_thr, std::min(max_thr, atoi(e)));
#endif
      const size_t fixed = (size_t)kpad * 17 + (mode == 4 ? 4 * threads : 0) + ((patch_n + 3) & ~3);
      lds = (fixed + (((size_t)ck * FX * IY * n_in + 3) & ~(size_t)3) + f_n) * sizeof(float);
      if (lds > kFusedLdsMax - 8 * 1024 || units >= 65536 || (size_t)ck * IX * IY * n_in >= 65536) continue;   // (8 KB static)
      CK = ck;
    }
    if (!CK || patch_n >= 65536) return false;
    // (a refusal of the runtime leaves the pair its launches, like every other reason above)
    const void* fn = reinterpret_cast<const void*>(vjp_stage_fn(mix_cout, taps, mode, zin));
    if (lds > 56 * 1024 && !kernel_caps(fn, kFusedLdsMax - 8 * 1024).lds_raised) return false;
    Step& s = add(SDFR_DECODER_STEP_VJP_STAGE, lc, g, scratch(), ((nc + TX - 1) / TX) * ((nc + TY - 1) / TY), ci_tiles, N, threads, lds);
    s.aux = d->conv_relu[lc] ? tape_conv(lc) : Slot{};
    s.C = C; s.mix = mix_cout; s.sel[0] = mix_l; s.ni = n_in; s.m = n_out; s.pad = pad; s.kpad = kpad;
    s.CK = CK; s.FX = FX; s.ZC = ZT; s.TX = TX; s.TY = TY; s.taps = taps; s.mode = mode; s.zin = zin;
    // the scaled form: the stage that reads grad_out adds the two volumes on load
    s.scaled = f.views == 1 && g.kind == Slot::kGrad;
    return true;
  }
  void backward() {
    const int nc = d->n_conv, last = nc - 1;
    // gradient w.r.t. the current tensor, [N][c][n^3]: what the last step wrote
    auto g = [&] { return plan.n ? plan.s[plan.n - 1].dst : Slot{Slot::kGrad}; };
    // the ReLU mask of layer l's output, where it has one
    auto mask = [&](int l) { return d->conv_relu[l] ? tape_conv(l) : Slot{}; };
    // z-row pitch of the padded tensor layer l's transposed convolution reads: rows 16 bytes apart when the direct
    // convolution takes it (its 16-byte loads and register prefetch then apply whatever the size; 34 -> 36 floats)
    auto pitch = [&](int l) {
      const int k = d->conv_k[l], np = out_n(l) + 2 * (k - 1);
      return !d->conv_swap[l] && !(k == 1 && d->conv_cin[l] <= 4) && direct[l].ok ? (np + 3) & ~3 : np;
    };
    if (out_n(last) != d->volume) resize_t(-1, g(), 1, out_n(last), d->volume);   // final resize
    for (int l = last; l >= 0; --l) {
      const int k = d->conv_k[l], ci_n = d->conv_cin[l], co_n = d->conv_cout[l];
      const int nin = d->conv_in_size[l], m = out_n(l), prev = d->conv_prev[l];
      const bool swap = d->conv_swap[l] != 0;
      const int np = swap ? prev : m + 2 * (k - 1);   // size of the tensor the transposed conv reads
      const int nconv = swap ? prev : nin;            // ... and of the one it produces
      const int pz = swap ? np : pitch(l);            // ... and the floats between its z-rows
      // the layer below produced the tensor in front of this layer's resize, and no swapped resize of its own sits
      // between: the pair can share launches (the resize's last pass writes the padded, masked input of the transposed
      // convolution below -- or the whole pair is one fused stage)
      const bool pair = prev != nin && l > 0 && !d->conv_swap[l - 1];
      // what the step that wrote g has done of this layer already: its steps 1 and 2 (a fused stage), its step 1 (g is
      // the padded, masked output gradient)
      Step* in = plan.n ? &plan.s[plan.n - 1] : nullptr;
      const bool staged = in && in->form == SDFR_DECODER_STEP_VJP_STAGE && in->layer == l;
      const bool padded = in && in->layer == l + 1 && in->pad >= 0 &&
                          (in->form == SDFR_DECODER_STEP_RESIZE_T_TILED || in->form == SDFR_DECODER_STEP_RESIZE_T_X_PAD ||
                           in->form == SDFR_DECODER_STEP_RESIZE_T_X_MIX_PAD);
      // 1. ReLU' and zero padding of the output gradient
      if (!staged && !padded && (!swap || d->conv_relu[l])) {
        const size_t cntp = (size_t)co_n * (swap ? m : np) * (swap ? m : np) * (swap ? m : pz);
        Step& s = add(SDFR_DECODER_STEP_PAD_MASK, l, g(), scratch(), (unsigned)((cntp + 255) / 256), N, 1, 256);
        s.aux = mask(l); s.C = co_n; s.m = m; s.pad = swap ? 0 : k - 1; s.pz = swap ? m : pz;
      }
      if (swap) {
        // (swapped 1x1 layer: forward was conv -> resize, so the resize is transposed first)
        // single latents: its last pass also runs the transposed 1x1 layer and writes the padded, masked input of
        // the transposed convolution below (conv1x1 + pad_mask launches saved) -- or the fused stage does all of it
        if (pair && !d->conv_relu[l] && ci_n <= 4 && ((size_t)N * co_n * nin * nin * nin <= kFewElements || co_n == 1)) {
          if (!vjp_stage(l - 1, g(), co_n, prev, nin, l, ci_n, 1, g().kind == Slot::kGrad))
            resize_t(l, g(), co_n, prev, nin, d->conv_k[l - 1] - 1, mask(l - 1), l, ci_n, pitch(l - 1));
          continue;
        }
        resize_t(l, g(), co_n, prev, nin);
      }
      // 2. data gradient = valid conv (kernel k) of the padded tensor with the flipped weights
      if (!staged) conv(l, g(), scratch(), co_n, ci_n, np, pz, nconv, 0);
      // 3. the resize in front of this layer, if any
      if (swap || prev == nin) continue;
      // few latents: with the layer below as one stage -- behind a fused stage chained to it (that stage's epilogue runs
      // this resize's z pass on its output rows), else reading the fine gradient itself
      if (pair && staged && vjp_stage(l - 1, g(), ci_n, prev, nin, -1, 0, 0, false)) in->e_nin = prev;
      else if (pair && vjp_stage(l - 1, g(), ci_n, prev, nin, -1, 0, 1, g().kind == Slot::kGrad)) {}
      else if (pair) resize_t(l, g(), ci_n, prev, nin, d->conv_k[l - 1] - 1, mask(l - 1), -1, 0, pitch(l - 1));
      else resize_t(l, g(), ci_n, prev, nin);
    }
    // the scaled form: unless a fused stage adds the two volumes on load, a launch of its own sums them first
    if (f.views) {
      bool in_stage = false;
      for (int i = 0; i < plan.n; ++i) in_stage = in_stage || plan.s[i].scaled;
      if (!in_stage) {
        const size_t vox = (size_t)d->volume * d->volume * d->volume;
        add(SDFR_DECODER_STEP_SCALED_COMBINE, -1, Slot{Slot::kGrad}, Slot{Slot::kGrad}, (unsigned)((vox + 255) / 256), 1, 1, 256);
        std::rotate(plan.s, plan.s + plan.n - 1, plan.s + plan.n);
      }
    }
    // g is now the gradient w.r.t. the (ReLU'd) output of the Linear stack, in the buffer that is not scratch(): the
    // transposed wide layer must write the FREE buffer -- other workgroups still read g while this one stores.
    const int win = plan.fd.width[d->n_fc - 1], wout = plan.fd.width[d->n_fc], kIb = 5, kSb = 4;
    const bool batch = N >= 32 && (wout & 3) == 0 &&
                       (((size_t)plan.fd.w_off[d->n_fc - 1] * sizeof(float) | mod16(g()) | mod16(Slot{Slot::kTapeFc})) & 15) == 0;
    plan.t_mid = scratch();
    if (batch) add(SDFR_DECODER_STEP_FC_LAST_T_BATCH, -1, g(), plan.t_mid, (win + kIb - 1) / kIb, (N + kSb - 1) / kSb, 1, kFcBlock);
    else add(SDFR_DECODER_STEP_FC_LAST_T, -1, g(), plan.t_mid, win, N, 1, kFcBlock);
    const int tail = one_wave ? SDFR_DECODER_STEP_FC_STACK_T_WAVE : SDFR_DECODER_STEP_FC_STACK_T;
    if (!f.deferred) add(tail, -1, plan.t_mid, Slot{}, N, 1, 1, one_wave ? 64 : kFcBlock);
  }
};

Plan make_plan(const sdfr_decoder* d, int N, const Facts& f, bool vjp) {
  Planner p(d, N, f, vjp);
  vjp ? p.backward() : p.forward();
  return p.plan;
}

// ---- launching a plan: nothing is decided here -------------------------------------------------------------------------
struct ScaledGrad {   // sdfr_decoder_backward_latent_deferred_scaled: g2 [n][volume], cnt [n]
  float* g2; const float* cnt; float weight; int n;
};
struct Tensors {   // what the slots of a plan stand for in one call
  const float* z; float *out, *tape, *buf[2], *grad, *g_z; const ScaledGrad* sg;
};
void launch_plan(const sdfr_decoder* d, const Plan& plan, bool vjp, const Tensors& t, int N, hipStream_t st) {
  const float* P = d->d_params;
  const float* zb = P + d->zero_bias_off;
  const size_t vox = (size_t)d->volume * d->volume * d->volume;
  auto at = [&](Slot s) -> float* {
    return s.kind == Slot::kOut ? t.out : s.kind == Slot::kGrad ? t.grad : s.kind == Slot::kBuf ? t.buf[s.i]
           : s.kind == Slot::kNone ? nullptr : t.tape + (size_t)N * (s.kind == Slot::kTapeFc ? d->tape_fc_off : d->tape_conv_off[s.i]);
  };
  for (int i = 0; i < plan.n; ++i) {
    const Step& s = plan.s[i];
    const int l = s.layer;
    const dim3 grid(s.grid[0], s.grid[1], s.grid[2]), block(s.threads);
    const float* src = at(s.src);
    float *dst = at(s.dst), *aux = at(s.aux);
    const float clamp = s.clamp ? d->tsdf : 0.0f;
    // layer l's weights and bias as this pass's convolution reads them; the 1x1x1 layer applied with it
    const float* w = l < 0 ? nullptr : P + (vjp ? d->bwd_w_off[l] : d->conv_w_off[l]);
    const float* bias = l < 0 || vjp ? zb : P + d->conv_b_off[l];
    const float* mix_w = s.mix && !vjp ? P + d->conv_w_off[l + 1] : nullptr;
    const float* mix_b = s.mix && !vjp ? P + d->conv_b_off[l + 1] : nullptr;
    const float* tape_fc = t.tape ? at(Slot{Slot::kTapeFc}) : nullptr;
    const int voxn = s.n * s.n * s.n, F = s.form;
#define SDFR_LAUNCH(kernel, ...) hipLaunchKernelGGL(kernel, grid, block, s.lds, st, __VA_ARGS__)   // (lds: 0 where unused)
    switch (F) {
      case SDFR_DECODER_STEP_FC_STACK: case SDFR_DECODER_STEP_FC_STACK_NARROW:
        SDFR_LAUNCH(F == SDFR_DECODER_STEP_FC_STACK ? fc_stack_kernel<false> : fc_stack_kernel<true>, P, plan.fd, t.z, dst);
        break;
      case SDFR_DECODER_STEP_FC_STACK_BATCH: case SDFR_DECODER_STEP_FC_STACK_BATCH_NARROW:
        SDFR_LAUNCH((F == SDFR_DECODER_STEP_FC_STACK_BATCH ? fc_stack_batch_kernel<kFcSamples, false>
                                                           : fc_stack_batch_kernel<kFcSamples, true>), P, plan.fd, t.z, N, s.ni, dst);
        break;
      case SDFR_DECODER_STEP_FC_CONV:
        SDFR_LAUNCH(fc_conv_kernel, P, plan.fd, t.z, aux, w, bias, dst, s.C, s.CO, s.n, s.m, s.kpad, s.relu, s.ZC);
        break;
      case SDFR_DECODER_STEP_RESIZE: SDFR_LAUNCH(resize3_kernel, src, s.C, s.ni, s.m, s.relu, clamp, dst); break;
      case SDFR_DECODER_STEP_RESIZE_TILED:
        dispatch_int_else_last<4, 5, 6, 7>(s.sel[0], [&](auto log) {
          constexpr int LOG = decltype(log)::value;
          SDFR_LAUNCH((s.sel[1] ? resize3_tiled_kernel<LOG, true> : resize3_tiled_kernel<LOG, false>), src, s.items, s.per, s.ni,
                      s.relu, clamp, s.span, dst);
        });
        break;
      case SDFR_DECODER_STEP_RESIZE_MIX:
        dispatch_int_else_last<1, 2, 3, 4>(s.CO, [&](auto co) {
          SDFR_LAUNCH(resize3_mix_kernel<decltype(co)::value>, src, w, bias, s.C, s.ni, s.m, s.relu, clamp, dst);
        });
        break;
      case SDFR_DECODER_STEP_CONV1X1: case SDFR_DECODER_STEP_CONV1X1_VEC4:
        dispatch_int_else_last<1, 2, 3, 4>(s.CO, [&](auto co) {
          constexpr int CO = decltype(co)::value;
          SDFR_LAUNCH(F == SDFR_DECODER_STEP_CONV1X1 ? conv1x1_kernel<CO> : conv1x1_vec4_kernel<CO>, src, w, bias, s.C, voxn, s.relu,
                      dst);
        });
        break;
      case SDFR_DECODER_STEP_DIRECT:
        dispatch_int_else_last<4, 8, 16>(s.CO, [&](auto co) {
          constexpr int CO = decltype(co)::value;
          SDFR_LAUNCH((s.sel[0] ? conv3d_direct_kernel<CO, true> : conv3d_direct_kernel<CO, false>), src,
                      P + (vjp ? d->bwd_direct_off[l] : d->fwd_direct_off[l]), bias, dst, s.C, s.n, s.pz, s.m, s.relu, s.TX, s.TY, s.ZC,
                      s.CK, mix_w, mix_b, s.mix, aux);
        });
        break;
      case SDFR_DECODER_STEP_DIRECT_UP:
        dispatch_int<4, 8, 16>(s.CO, [&](auto co) {
          SDFR_LAUNCH(conv3d_direct_up_kernel<decltype(co)::value>, src, s.ni, P + d->fwd_direct_off[l], bias, dst, s.C, s.n, s.sel[0],
                      s.m, s.relu, s.TX, s.TY, s.ZC, s.CK, s.span);
        });
        break;
      case SDFR_DECODER_STEP_MFMA: case SDFR_DECODER_STEP_MFMA_SPLIT_K:
      case SDFR_DECODER_STEP_MFMA_Z_GROUPED: case SDFR_DECODER_STEP_MFMA_RESIDENT: {
        const sdfr_decoder::ZPlan& zp = vjp ? d->bwd_z[l] : d->fwd_z[l];
        const bool zgrp = F == SDFR_DECODER_STEP_MFMA_Z_GROUPED;
        const int* tab = reinterpret_cast<const int*>(P + (zgrp ? zp.tab_off : vjp ? d->bwd_tab_off[l] : d->conv_tab_off[l]));
        SDFR_LAUNCH(F == SDFR_DECODER_STEP_MFMA_RESIDENT ? conv3d_mfma_kernel<true> : conv3d_mfma_kernel<false>, src,
                    zgrp ? P + zp.w_off : w, tab, bias, dst, s.C, s.CO, s.n, s.m, s.kpad, s.relu, s.tw, s.zg, s.split);
        break;
      }
      case SDFR_DECODER_STEP_MFMA_UP:
        SDFR_LAUNCH(mfma_up_fn(s.sel[0]), src, s.ni, w, bias, dst, s.C, s.CO, s.n, s.m, s.kpad, s.relu, s.span, s.ZC, s.TX, s.TY,
                    mix_w, mix_b, s.mix, aux);
        break;
      case SDFR_DECODER_STEP_COPY: copy_words_async(dst, src, s.outer, st); break;
      case SDFR_DECODER_STEP_CLAMP: SDFR_LAUNCH(clamp_kernel, dst, s.outer, d->tsdf); break;
      case SDFR_DECODER_STEP_SCALED_COMBINE:
        SDFR_LAUNCH(scaled_combine_kernel, t.grad, t.sg->g2, t.sg->n, t.sg->cnt, t.sg->weight, vox);
        break;
      case SDFR_DECODER_STEP_PAD_MASK: SDFR_LAUNCH(pad_mask_kernel, src, aux, s.C, s.m, s.pad, s.pz, dst); break;
      case SDFR_DECODER_STEP_RESIZE_T_TILED:
        SDFR_LAUNCH(resize_t_fn(s.sel[0], s.sel[1]), src, s.ni, s.m, aux, std::max(s.pad, 0), s.pz, s.tc, s.span, s.items, s.slots,
                    s.mix ? w : nullptr, zb, dst);
        break;
      case SDFR_DECODER_STEP_RESIZE_T_ZY: SDFR_LAUNCH(resize_zy_backward_kernel, src, s.outer, s.ni, s.m, dst); break;
      case SDFR_DECODER_STEP_RESIZE_T_AXIS: SDFR_LAUNCH(resize_axis_backward_kernel, src, s.outer, s.ni, s.m, s.inner, dst); break;
      case SDFR_DECODER_STEP_RESIZE_T_X_PAD:
        SDFR_LAUNCH(resize_x_backward_pad_kernel, src, s.outer, s.ni, s.m, aux, s.pad, s.pz, dst);
        break;
      case SDFR_DECODER_STEP_RESIZE_T_X_MIX_PAD:
        dispatch_int_else_last<1, 2, 3, 4>(s.mix, [&](auto co) {
          SDFR_LAUNCH(resize_x_backward_mix_pad_kernel<decltype(co)::value>, src, s.C, s.ni, s.m, w, zb, aux, s.pad, s.pz, dst);
        });
        break;
      case SDFR_DECODER_STEP_VJP_STAGE: {
        VjpStage v;
        v.g = src; v.act = aux; v.mix_w = s.mix ? P + d->bwd_w_off[s.sel[0]] : nullptr; v.mix_b = zb;
        v.wmat = w; v.bias = zb; v.out = dst;
        v.tab = P + d->rs_tab_off[l + 1]; v.e_tab = s.e_nin > 0 ? P + d->rs_tab_off[l] : nullptr;
        v.C = s.C; v.n_in = s.ni; v.n_out = s.m; v.pad = s.pad; v.Cc = d->conv_cin[l]; v.kpad = s.kpad;
        v.CK = s.CK; v.FX = s.FX; v.ZT = s.ZC; v.TX = s.TX; v.TY = s.TY; v.zin = s.zin; v.e_nin = s.e_nin;
        if (s.scaled) { v.g2 = t.sg->g2; v.cnt = t.sg->cnt; v.weight = t.sg->weight; }
        SDFR_LAUNCH(vjp_stage_fn(s.mix, s.taps, s.mode, s.zin), v);
        break;
      }
      case SDFR_DECODER_STEP_FC_LAST_T_BATCH:
        SDFR_LAUNCH((fc_last_backward_batch_kernel<5, 4>), P, plan.fd, src, tape_fc, N, dst);
        break;
      case SDFR_DECODER_STEP_FC_LAST_T:   // (the scaled form: both volumes are zero-filled once they have been read)
        SDFR_LAUNCH(fc_last_backward_kernel, P, plan.fd, src, tape_fc, dst, t.sg ? t.grad : (float*)nullptr,
                    t.sg ? t.sg->g2 : (float*)nullptr, (int)(vox / 4), t.sg ? t.sg->n : 0);
        break;
      case SDFR_DECODER_STEP_FC_STACK_T: case SDFR_DECODER_STEP_FC_STACK_T_WAVE:
        SDFR_LAUNCH(F == SDFR_DECODER_STEP_FC_STACK_T ? fc_stack_backward_kernel : fc_stack_backward_wave_kernel, P, plan.fd, t.z, src,
                    t.g_z);
        break;
    }
#undef SDFR_LAUNCH
  }
}
}  // namespace
