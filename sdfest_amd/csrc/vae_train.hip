// vae_train.hip -- one training iteration of the SDF VAE (sdfest/vae/scripts/train.py:195-287), gfx950: the forward with
// a tape, the loss and its gradient, the gradient of every parameter, and Adam over a flat buffer.
//
// The network is a list of ops over activations in torch's order ((C, S, S, S) per sample, then flat):
//   encoder  conv / pool / linear / relu as encoder.hip has them, then the two heads and z = eps exp(0.5 log_var) + means
//   decoder  Linear + ReLU for every fc layer; per conv layer a trilinear resize (align_corners = False) where the size
//            differs, Conv3d (stride 1, no padding), ReLU; a last resize to the volume size
// The parameters are read where the caller keeps them: one flat buffer in state_dict order and torch's layouts
// ([cout][cin][k][k][k], [out][in]).  Nothing is re-laid-out: a training step changes every weight, and the inference
// handles' derived layouts (decoder.hip: about eight per layer) are built once, from the trained state.
//
// Who owns what, so that every result has one owner, a fixed order of summation and no atomics:
//   forward        conv: a thread per (sample, 4 output channels, position), fmaf over ci, a, b, c; linear and heads: a
//                  wave per (sample, row), lane l sums the features l, l + 64, ..., then a fixed butterfly; pool / resize / relu:
//                  a thread per output element
//   data gradient  in GATHER form, a thread per INPUT element: conv sums over (co, taps) the outputs that read it,
//                  resize over the outputs whose two source indices per axis name it, pool over the windows whose first
//                  maximum it is (recomputed from the tape).  The ReLU of the layer that produced the input is applied
//                  by the thread that writes the gradient (out > 0 ? g : 0), so every gradient tensor is stored masked.
//   conv weight /  two stages.  Stage 1: a workgroup owns kWgCo output channels x kWgRows rows of (ci, tap) and a range
//   bias gradient  of kWgChunks x kWgT positions of one sample; per chunk it stages the masked output gradient
//                  [co][t] and the im2col rows [(ci, tap)][t] in LDS (row pitch kWgT + 1: the 32 rows a wave reads lie
//                  in 32 banks) and every thread accumulates its 4 (co, row) partials in registers over t = 0, 1, ...
//                  Stage 2: a thread group per element sums the partial records in ascending order, in fp64.
//   linear weight  a thread per (out, in): the sum over the samples in ascending order (an outer-product sum over N)
//   loss           stage 1: a thread takes kLossItems voxels, a workgroup reduces its four sums (butterfly, then the
//                  waves in order); stage 2: one workgroup sums the records and the KLD in fp64, fixed tree
//   pc term        a thread per depth pixel; loss_pc in the same two stages; the scatter into g_recon as 64-bit
//                  fixed-point integer adds (associative: any order gives the same bits), converted once
// Measured figures and what binds each kernel: DESIGN.md section 3.14.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "philox.hpp"

namespace {
constexpr int kOpConv = SDFR_ENC_CONV, kOpPool = SDFR_ENC_MAXPOOL, kOpLinear = SDFR_ENC_LINEAR, kOpRelu = SDFR_ENC_RELU;
constexpr int kOpResize = 5;              // decoder only, never in an op list of the ABI
constexpr int kMaxOps = 32, kMaxLatent = 512, kMaxHidden = 2048;   // the inference handles' limits
constexpr int kThreads = 256;
constexpr int kCT = 4;                    // conv: output (forward) / input (data gradient) channels per thread
constexpr int kWgT = 128;                 // weight gradient: positions per staged chunk
constexpr int kWgChunks = 4;              // ... chunks per workgroup (one partial record per kWgT * kWgChunks positions)
constexpr int kWgCo = 32, kWgRows = 32;   // ... output channels x (ci, tap) rows per workgroup: 4 accumulators a thread
constexpr int kCombineSlices = 16;        // combine: threads per element, each a contiguous slice of the records
constexpr int kLossItems = 8;             // loss: voxels per thread
constexpr int kSrcX = -1, kSrcZ = -2;     // an op's input: the volume, the latent, or the output of op `src`
constexpr unsigned kMaxBlocks = 1u << 20;
constexpr int kPcGroups = 128;            // point cloud term: workgroups (= records) per sample
constexpr int kPcTileW = 32, kPcTileH = 8;   // ... pixels per workgroup and round
static_assert(kPcTileW * kPcTileH == kThreads, "a thread per pixel of a tile");
constexpr unsigned kPcStream = 0x56415043u;  // counter word 3 of the term's orientations ("VAPC", include/sdfr.h)
}  // namespace

struct TrainOp {
  int type, cin, cout;        // linear: in / out features; pool, relu, resize: cin = cout = channels
  int n, m, k, s, p, relu;    // input side, output side, kernel, stride, padding; relu: applied to the output
  int src, src_relu;          // src_relu: the input is a ReLU's output (the data gradient is masked with it)
  int to_recon;               // the output goes to the caller's recon, not to the tape
  long long w_off, b_off;     // floats into the flat parameter buffer
  long long in_f, out_f;      // floats per sample
  long long tape_off;         // floats per sample of the tape in front of this op's output
};

struct sdfr_vae_trainer {
  int device = 0, volume = 0, latent = 0, F = 0;
  float tsdf = 0.0f;
  std::vector<TrainOp> ops;   // encoder ops [0, n_enc), decoder ops [n_enc, size)
  int n_enc = 0;
  int first_param_op = 0;     // the encoder's first op with parameters: no data gradient at or in front of it
  long long hm_w = 0, hm_b = 0, hl_w = 0, hl_b = 0;   // the heads in the parameter buffer
  size_t n_params = 0, n_enc_params = 0;
  long long tape_f = 0;       // floats per sample
  long long max_act = 0;      // floats per sample of the largest activation (the gradient buffers' size)
};

namespace sdfr {
namespace {

inline unsigned blocks_for(long long items) {
  return (unsigned)std::min<long long>((items + kThreads - 1) / kThreads, kMaxBlocks);
}

// ---- forward --------------------------------------------------------------------------------------------------------
// grid-stride over N x ceil(cout / 4) x m^3 items
__global__ __launch_bounds__(kThreads) void train_conv_forward_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                      TrainOp op, const float* __restrict__ prm, int N) {
  const int n = op.n, m = op.m, k = op.k, s = op.s, p = op.p, k3 = k * k * k;
  const long long mv = (long long)m * m * m, nv = (long long)n * n * n;
  const int chunks = (op.cout + kCT - 1) / kCT;
  const long long total = (long long)N * chunks * mv;
  const float* __restrict__ w = prm + op.w_off;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < total; it += (long long)gridDim.x * kThreads) {
    const long long nb = it / (chunks * mv), r = it - nb * chunks * mv;
    const int ch = (int)(r / mv), pos = (int)(r - ch * mv);
    const int x = pos / (m * m), yz = pos - x * m * m, y = yz / m, z = yz - y * m;
    const float* wc[kCT];
    float acc[kCT];
#pragma unroll
    for (int t = 0; t < kCT; ++t) {
      acc[t] = 0.0f;
      wc[t] = w + (size_t)min(ch * kCT + t, op.cout - 1) * op.cin * k3;   // past cout: computed, never stored
    }
    const float* src = in + (size_t)nb * op.in_f;
    for (int ci = 0; ci < op.cin; ++ci) {
      const float* sc = src + (size_t)ci * nv;
      for (int a = 0; a < k; ++a) {
        const int ix = x * s - p + a;
        if ((unsigned)ix >= (unsigned)n) continue;
        for (int b = 0; b < k; ++b) {
          const int iy = y * s - p + b;
          if ((unsigned)iy >= (unsigned)n) continue;
          const float* row = sc + ((size_t)ix * n + iy) * n;
          const int tap0 = ci * k3 + (a * k + b) * k;
          for (int c = 0; c < k; ++c) {
            const int iz = z * s - p + c;
            if ((unsigned)iz >= (unsigned)n) continue;
            const float v = row[iz];
#pragma unroll
            for (int t = 0; t < kCT; ++t) acc[t] = fmaf(v, wc[t][tap0 + c], acc[t]);
          }
        }
      }
    }
    float* dst = out + (size_t)nb * op.out_f;
#pragma unroll
    for (int t = 0; t < kCT; ++t) {
      const int co = ch * kCT + t;
      if (co < op.cout) {
        float v = acc[t] + prm[op.b_off + co];
        if (op.relu) v = fmaxf(v, 0.0f);
        dst[(size_t)co * mv + pos] = v;
      }
    }
  }
}

// a wave per (sample, output row), grid-stride
__global__ __launch_bounds__(kThreads) void train_linear_forward_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                        TrainOp op, const float* __restrict__ prm, int N) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (kThreads / 64), total = (long long)N * op.cout;
  for (long long it = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); it < total; it += waves) {
    const long long nb = it / op.cout;
    const int o = (int)(it - nb * op.cout);
    float r = wave_dot(in + (size_t)nb * op.cin, prm + op.w_off + (size_t)o * op.cin, op.cin, lane) +
              prm[op.b_off + o];
    if (op.relu) r = fmaxf(r, 0.0f);
    if (lane == 0) out[(size_t)nb * op.cout + o] = r;
  }
}

__global__ __launch_bounds__(kThreads) void train_pool_forward_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                      TrainOp op, int N) {
  const int n = op.n, m = op.m, k = op.k, s = op.s;
  const long long mv = (long long)m * m * m, nv = (long long)n * n * n, total = (long long)N * op.cout * mv;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < total; it += (long long)gridDim.x * kThreads) {
    const long long nc = it / mv;
    const int pos = (int)(it - nc * mv);
    const int x = pos / (m * m), yz = pos - x * m * m, y = yz / m, z = yz - y * m;
    const float* sc = in + (size_t)nc * nv + ((size_t)(x * s) * n + y * s) * n + z * s;
    float r = -INFINITY;
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b)
        for (int c = 0; c < k; ++c) r = fmaxf(r, sc[((size_t)a * n + b) * n + c]);
    if (op.relu) r = fmaxf(r, 0.0f);
    out[it] = r;
  }
}

__global__ __launch_bounds__(kThreads) void train_relu_forward_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                      long long total) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads)
    out[i] = fmaxf(in[i], 0.0f);
}

// torch's source index of output index o (upsample_trilinear3d, align_corners = False): i0, i1 = i0 + (i0 < n - 1), the
// weight l1 of i1 (1 - l1 of i0); scale = (float)n_in / n_out
__device__ __forceinline__ void resize_source(int o, float scale, int n_in, int& i0, int& i1, float& l1) {
  const float src = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.0f);
  i0 = min((int)src, n_in - 1);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
}

// a thread per output element
__global__ __launch_bounds__(kThreads) void train_resize_forward_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                        TrainOp op, int N) {
  const int n = op.n, m = op.m;
  const float scale = (float)n / (float)m;
  const long long mv = (long long)m * m * m, nv = (long long)n * n * n, total = (long long)N * op.cout * mv;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < total; it += (long long)gridDim.x * kThreads) {
    const long long nc = it / mv;
    const int pos = (int)(it - nc * mv);
    const int x = pos / (m * m), yz = pos - x * m * m, y = yz / m, z = yz - y * m;
    int x0, x1, y0, y1, z0, z1;
    float lx, ly, lz;
    resize_source(x, scale, n, x0, x1, lx);
    resize_source(y, scale, n, y0, y1, ly);
    resize_source(z, scale, n, z0, z1, lz);
    const float* sc = in + (size_t)nc * nv;
    auto at = [&](int a, int b, int c) { return sc[((size_t)a * n + b) * n + c]; };
    const float hx = 1.0f - lx, hy = 1.0f - ly, hz = 1.0f - lz;
    out[it] = hx * (hy * (hz * at(x0, y0, z0) + lz * at(x0, y0, z1)) + ly * (hz * at(x0, y1, z0) + lz * at(x0, y1, z1))) +
              lx * (hy * (hz * at(x1, y0, z0) + lz * at(x1, y0, z1)) + ly * (hz * at(x1, y1, z0) + lz * at(x1, y1, z1)));
  }
}

// the heads and z: a wave per (sample, latent component) -- its means row, its log_var row, then z
__global__ __launch_bounds__(kThreads) void train_heads_forward_kernel(const float* __restrict__ h, int F, int L, int N,
                                                                       const float* __restrict__ prm, long long hm_w,
                                                                       long long hm_b, long long hl_w, long long hl_b,
                                                                       float* __restrict__ means,
                                                                       float* __restrict__ log_var,
                                                                       float* __restrict__ z, unsigned long long seed) {
// z = eps * sd + means as two roundings, like encoder.hip and the reference's torch expression
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (kThreads / 64), total = (long long)N * L;
  for (long long it = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); it < total; it += waves) {
    const int nb = (int)(it / L), j = (int)(it - (long long)nb * L);
    const float* hin = h + (size_t)nb * F;
    const float mu = wave_dot(hin, prm + hm_w + (size_t)j * F, F, lane) + prm[hm_b + j];
    const float lv = wave_dot(hin, prm + hl_w + (size_t)j * F, F, lane) + prm[hl_b + j];
    if (lane == 0) {
      means[it] = mu;
      log_var[it] = lv;
      const float sd = expf(0.5f * lv);
      z[it] = normal_eps(seed, (unsigned)nb, (unsigned)j) * sd + mu;
    }
  }
}

// ---- loss -------------------------------------------------------------------------------------------------------------
struct LossArgs {
  float w2s, w2l, w1s, w1l, wk, tsdf;   // tsdf: 0 = no clamp (warm-up, or a model without truncation)
};

// stage 1: record b = {l2_small, l2_large, l1_small, l1_large} of the voxels [b * 256 * kLossItems, ...)
__global__ __launch_bounds__(kThreads) void train_loss_kernel(const float* __restrict__ recon, const float* __restrict__ x,
                                                              long long total, LossArgs a, float* __restrict__ g_recon,
                                                              float* __restrict__ records) {
  __shared__ float part[kThreads / 64][4];
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const long long base = (long long)blockIdx.x * kThreads * kLossItems + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kLossItems; ++i) {
    const long long e = base + (long long)i * kThreads;
    if (e >= total) break;
    const float xv = x[e];
    float r = recon[e], pass = 1.0f;
    if (a.tsdf > 0.0f && fabsf(xv) >= a.tsdf && fabsf(r) >= a.tsdf) {   // train.py:208-218; clamp's gradient: 1 inside
      pass = (r < -a.tsdf || r > a.tsdf) ? 0.0f : 1.0f;
      r = fminf(fmaxf(r, -a.tsdf), a.tsdf);
    }
    const float d = r - xv, e1 = fabsf(d), e2 = e1 * e1;
    const bool small = fabsf(xv) < 0.1f;
    s[small ? 0 : 1] += e2;
    s[small ? 2 : 3] += e1;
    const float sign = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    g_recon[e] = pass * ((small ? a.w2s : a.w2l) * 2.0f * d + (small ? a.w1s : a.w1l) * sign);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[q] += __shfl_xor(s[q], d, 64);
    if (lane == 0) part[wave][q] = s[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float t = part[0][threadIdx.x];
    for (int wv = 1; wv < kThreads / 64; ++wv) t += part[wv][threadIdx.x];
    records[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// stage 2, one workgroup: thread t sums the records t, t + 256, ... (fp64), a fixed tree over the threads; the KLD and
// its gradient; the total
__global__ __launch_bounds__(kThreads) void train_loss_finish_kernel(const float* __restrict__ records, long long n_records,
                                                                     const float* __restrict__ means,
                                                                     const float* __restrict__ log_var, long long NL,
                                                                     LossArgs a, float* __restrict__ terms,
                                                                     float* __restrict__ g_means,
                                                                     float* __restrict__ g_log_var) {
  __shared__ double red[5][kThreads];
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long r = threadIdx.x; r < n_records; r += kThreads)
    for (int q = 0; q < 4; ++q) s[q] += (double)records[r * 4 + q];
  for (long long i = threadIdx.x; i < NL; i += kThreads) {
    const float mu = means[i], lv = log_var[i], ev = expf(lv);
    s[4] += (double)(1.0f + lv - mu * mu - ev);
    g_means[i] = a.wk * mu;
    g_log_var[i] = a.wk * 0.5f * (ev - 1.0f);
  }
  for (int q = 0; q < 5; ++q) red[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int half = kThreads / 2; half >= 1; half >>= 1) {
    if (threadIdx.x < half)
      for (int q = 0; q < 5; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double kld = -0.5 * red[4][0];
    for (int q = 0; q < 4; ++q) terms[q] = (float)red[q][0];
    terms[4] = (float)kld;
    terms[5] = (float)((double)a.w2s * red[0][0] + (double)a.w2l * red[1][0] + (double)a.w1s * red[2][0] +
                       (double)a.w1l * red[3][0] + (double)a.wk * kld);
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float masked(float g, const float* __restrict__ act, size_t i) {
  return (act == nullptr || act[i] > 0.0f) ? g : 0.0f;
}

// out = g where act > 0 (a ReLU nothing else applies: the last layer's, a stand-alone relu op's)
__global__ __launch_bounds__(kThreads) void train_mask_kernel(const float* __restrict__ g, const float* __restrict__ act,
                                                              float* __restrict__ out, long long total) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads)
    out[i] = act[i] > 0.0f ? g[i] : 0.0f;
}

// conv data gradient: a thread per (sample, 4 input channels, input position); mask: the input activation or NULL
__global__ __launch_bounds__(kThreads) void train_conv_dgrad_kernel(const float* __restrict__ gout, float* __restrict__ gin,
                                                                    const float* __restrict__ mask, TrainOp op,
                                                                    const float* __restrict__ prm, int N) {
  const int n = op.n, m = op.m, k = op.k, s = op.s, p = op.p, k3 = k * k * k;
  const long long mv = (long long)m * m * m, nv = (long long)n * n * n;
  const int chunks = (op.cin + kCT - 1) / kCT;
  const long long total = (long long)N * chunks * nv;
  const float* __restrict__ w = prm + op.w_off;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < total; it += (long long)gridDim.x * kThreads) {
    const long long nb = it / (chunks * nv), r = it - nb * chunks * nv;
    const int ch = (int)(r / nv), pos = (int)(r - ch * nv);
    const int x = pos / (n * n), yz = pos - x * n * n, y = yz / n, z = yz - y * n;
    int cis[kCT];
    float acc[kCT];
#pragma unroll
    for (int t = 0; t < kCT; ++t) {
      acc[t] = 0.0f;
      cis[t] = min(ch * kCT + t, op.cin - 1);
    }
    const float* g = gout + (size_t)nb * op.out_f;
    for (int co = 0; co < op.cout; ++co) {
      const float* gc = g + (size_t)co * mv;
      const float* wco = w + (size_t)co * op.cin * k3;
      for (int a = 0; a < k; ++a) {
        const int tx = x + p - a, ox = tx / s;
        if (tx < 0 || ox * s != tx || ox >= m) continue;
        for (int b = 0; b < k; ++b) {
          const int ty = y + p - b, oy = ty / s;
          if (ty < 0 || oy * s != ty || oy >= m) continue;
          for (int c = 0; c < k; ++c) {
            const int tz = z + p - c, oz = tz / s;
            if (tz < 0 || oz * s != tz || oz >= m) continue;
            const float v = gc[((size_t)ox * m + oy) * m + oz];
            const int tap = (a * k + b) * k + c;
#pragma unroll
            for (int t = 0; t < kCT; ++t) acc[t] = fmaf(v, wco[(size_t)cis[t] * k3 + tap], acc[t]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kCT; ++t) {
      const int ci = ch * kCT + t;
      if (ci < op.cin) {
        const size_t i = (size_t)nb * op.in_f + (size_t)ci * nv + pos;
        gin[i] = masked(acc[t], mask, i);
      }
    }
  }
}

// conv weight / bias gradient, stage 1 (see the file comment).  grid: (N * ranges, co groups * row groups);
// record g = blockIdx.x: [cout][cin k^3] weights, then [cout] bias
__global__ __launch_bounds__(kThreads) void train_conv_wgrad_kernel(const float* __restrict__ gout, const float* __restrict__ in,
                                                                    TrainOp op, int ranges, float* __restrict__ records) {
  __shared__ float dy[kWgCo][kWgT + 1];
  __shared__ float col[kWgRows][kWgT + 1];
  const int n = op.n, m = op.m, k = op.k, s = op.s, p = op.p, k3 = k * k * k, R = op.cin * k3;
  const int mv = m * m * m;
  const size_t nv = (size_t)n * n * n;
  const int row_groups = (R + kWgRows - 1) / kWgRows;
  const int nb = blockIdx.x / ranges, range = blockIdx.x - nb * ranges;
  const int cog = (blockIdx.y / row_groups) * kWgCo, rg = (blockIdx.y % row_groups) * kWgRows;
  const int r_l = threadIdx.x & (kWgRows - 1), co_l = threadIdx.x / kWgRows;   // 32 rows x 8 channel lanes
  constexpr int kCoLanes = kThreads / kWgRows, kAcc = kWgCo / kCoLanes;
  float acc[kAcc], bias = 0.0f;
#pragma unroll
  for (int j = 0; j < kAcc; ++j) acc[j] = 0.0f;
  const float* g = gout + (size_t)nb * op.out_f;
  const float* src = in + (size_t)nb * op.in_f;
  for (int chunk = 0; chunk < kWgChunks; ++chunk) {
    const int c0 = (range * kWgChunks + chunk) * kWgT;
    if (c0 >= mv) break;   // uniform over the workgroup
    for (int i = threadIdx.x; i < kWgCo * kWgT; i += kThreads) {
      const int cl = i / kWgT, t = i - cl * kWgT, co = cog + cl;
      dy[cl][t] = (co < op.cout && c0 + t < mv) ? g[(size_t)co * mv + c0 + t] : 0.0f;
    }
    for (int i = threadIdx.x; i < kWgRows * kWgT; i += kThreads) {
      const int rl = i / kWgT, t = i - rl * kWgT, r = rg + rl, pos = c0 + t;
      float v = 0.0f;
      if (r < R && pos < mv) {
        const int ci = r / k3, tap = r - ci * k3, a = tap / (k * k), bc = tap - a * k * k, b = bc / k, c = bc - b * k;
        const int x = pos / (m * m), yz = pos - x * m * m, y = yz / m, z = yz - y * m;
        const int ix = x * s - p + a, iy = y * s - p + b, iz = z * s - p + c;
        if ((unsigned)ix < (unsigned)n && (unsigned)iy < (unsigned)n && (unsigned)iz < (unsigned)n)
          v = src[(size_t)ci * nv + ((size_t)ix * n + iy) * n + iz];
      }
      col[rl][t] = v;
    }
    __syncthreads();
    for (int t = 0; t < kWgT; ++t) {
      const float cv = col[r_l][t];
#pragma unroll
      for (int j = 0; j < kAcc; ++j) acc[j] = fmaf(dy[co_l + kCoLanes * j][t], cv, acc[j]);
    }
    if (rg == 0 && threadIdx.x < kWgCo)
      for (int t = 0; t < kWgT; ++t) bias += dy[threadIdx.x][t];
    __syncthreads();
  }
  float* rec = records + (size_t)blockIdx.x * ((size_t)op.cout * R + op.cout);
  if (rg + r_l < R) {
#pragma unroll
    for (int j = 0; j < kAcc; ++j) {
      const int co = cog + co_l + kCoLanes * j;
      if (co < op.cout) rec[(size_t)co * R + rg + r_l] = acc[j];
    }
  }
  if (rg == 0 && threadIdx.x < kWgCo && cog + threadIdx.x < op.cout) rec[(size_t)op.cout * R + cog + threadIdx.x] = bias;
}

// stage 2: element e of a record (weights, then bias) = the sum over the n_records records.  16 threads an element, each
// a contiguous slice in ascending order (fp64), then the slices in order.  grid: ceil(elements / 16)
__global__ __launch_bounds__(kThreads) void train_conv_wgrad_combine_kernel(const float* __restrict__ records, int n_records,
                                                                            long long n_w, long long n_b,
                                                                            float* __restrict__ gw, float* __restrict__ gb) {
  __shared__ double part[kCombineSlices][kThreads / kCombineSlices];
  const int e_l = threadIdx.x % (kThreads / kCombineSlices), sl = threadIdx.x / (kThreads / kCombineSlices);
  const long long e = (long long)blockIdx.x * (kThreads / kCombineSlices) + e_l, stride = n_w + n_b;
  const int per = (n_records + kCombineSlices - 1) / kCombineSlices;
  const int r0 = sl * per, r1 = min(n_records, r0 + per);
  double s = 0.0;
  if (e < stride)
    for (int r = r0; r < r1; ++r) s += (double)records[(size_t)r * stride + e];
  part[sl][e_l] = s;
  __syncthreads();
  if (sl == 0 && e < stride) {
    for (int q = 1; q < kCombineSlices; ++q) s += part[q][e_l];
    if (e < n_w) gw[e] = (float)s;
    else gb[e - n_w] = (float)s;
  }
}

// linear weight / bias gradient: a thread per (out, in) element, then per out; the samples in ascending order
__global__ __launch_bounds__(kThreads) void train_linear_wgrad_kernel(const float* __restrict__ gout, const float* __restrict__ in,
                                                                      int fin, int fout, int N, float* __restrict__ gw,
                                                                      float* __restrict__ gb) {
  const long long n_w = (long long)fin * fout, total = n_w + fout;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    float acc = 0.0f;
    if (e < n_w) {
      const int o = (int)(e / fin), i = (int)(e - (long long)o * fin);
      for (int nb = 0; nb < N; ++nb) acc = fmaf(gout[(size_t)nb * fout + o], in[(size_t)nb * fin + i], acc);
      gw[e] = acc;
    } else {
      const int o = (int)(e - n_w);
      for (int nb = 0; nb < N; ++nb) acc += gout[(size_t)nb * fout + o];
      gb[o] = acc;
    }
  }
}

// linear data gradient, few outputs: a thread per (sample, in); the heads pass both weight blocks (g2 / w2 else NULL)
__global__ __launch_bounds__(kThreads) void train_linear_dgrad_kernel(const float* __restrict__ g1, const float* __restrict__ w1,
                                                                      const float* __restrict__ g2, const float* __restrict__ w2,
                                                                      int fin, int fout, int N, const float* __restrict__ mask,
                                                                      float* __restrict__ gin) {
  const long long total = (long long)N * fin;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    const long long nb = e / fin;
    const int i = (int)(e - nb * fin);
    float acc = 0.0f;
    for (int o = 0; o < fout; ++o) acc = fmaf(g1[(size_t)nb * fout + o], w1[(size_t)o * fin + i], acc);
    if (g2)
      for (int o = 0; o < fout; ++o) acc = fmaf(g2[(size_t)nb * fout + o], w2[(size_t)o * fin + i], acc);
    gin[e] = masked(acc, mask, (size_t)e);
  }
}

// ... many outputs (the decoder's wide layer: 8192 -> 50): a wave per (sample, in), lane l sums the rows l, l + 64, ...
__global__ __launch_bounds__(kThreads) void train_linear_dgrad_wave_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                                           int fin, int fout, int N, const float* __restrict__ mask,
                                                                           float* __restrict__ gin) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * (kThreads / 64), total = (long long)N * fin;
  for (long long e = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); e < total; e += waves) {
    const long long nb = e / fin;
    const int i = (int)(e - nb * fin);
    float acc = 0.0f;
    for (int o = lane; o < fout; o += 64) acc = fmaf(g[(size_t)nb * fout + o], w[(size_t)o * fin + i], acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) gin[e] = masked(acc, mask, (size_t)e);
  }
}

// the weight with which output index o of an axis reads input index i
__device__ __forceinline__ float resize_weight(int o, int i, float scale, int n_in) {
  int i0, i1;
  float l1;
  resize_source(o, scale, n_in, i0, i1, l1);
  return (i0 == i ? 1.0f - l1 : 0.0f) + (i1 == i ? l1 : 0.0f);
}

// the outputs that can read input index i: floor(source) is i - 1 or i (a margin of one; resize_weight decides)
__device__ __forceinline__ void resize_readers(int i, float scale, int n_out, int& lo, int& hi) {
  lo = max(0, (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1);
  hi = min(n_out - 1, (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1);
}

// transposed resize: a thread per INPUT element sums the outputs that read it, x then y then z ascending
__global__ __launch_bounds__(kThreads) void train_resize_dgrad_kernel(const float* __restrict__ gout, float* __restrict__ gin,
                                                                      const float* __restrict__ mask, TrainOp op, int N) {
  const int n = op.n, m = op.m;
  const float scale = (float)n / (float)m;
  const long long mv = (long long)m * m * m, nv = (long long)n * n * n, total = (long long)N * op.cin * nv;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < total; it += (long long)gridDim.x * kThreads) {
    const long long nc = it / nv;
    const int pos = (int)(it - nc * nv);
    const int x = pos / (n * n), yz = pos - x * n * n, y = yz / n, z = yz - y * n;
    int xl, xh, yl, yh, zl, zh;
    resize_readers(x, scale, m, xl, xh);
    resize_readers(y, scale, m, yl, yh);
    resize_readers(z, scale, m, zl, zh);
    const float* g = gout + (size_t)nc * mv;
    float acc = 0.0f;
    for (int ox = xl; ox <= xh; ++ox) {
      const float wx = resize_weight(ox, x, scale, n);
      if (wx == 0.0f) continue;
      for (int oy = yl; oy <= yh; ++oy) {
        const float wxy = wx * resize_weight(oy, y, scale, n);
        if (wxy == 0.0f) continue;
        const float* row = g + ((size_t)ox * m + oy) * m;
        for (int oz = zl; oz <= zh; ++oz) acc = fmaf(wxy * resize_weight(oz, z, scale, n), row[oz], acc);
      }
    }
    gin[it] = masked(acc, mask, (size_t)it);
  }
}

// max pool: a thread per INPUT element sums the windows whose FIRST maximum (a, b, c order, as torch picks it) it is
__global__ __launch_bounds__(kThreads) void train_pool_dgrad_kernel(const float* __restrict__ gout, const float* __restrict__ in,
                                                                    float* __restrict__ gin, const float* __restrict__ mask,
                                                                    TrainOp op, int N) {
  const int n = op.n, m = op.m, k = op.k, s = op.s;
  const long long mv = (long long)m * m * m, nv = (long long)n * n * n, total = (long long)N * op.cin * nv;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < total; it += (long long)gridDim.x * kThreads) {
    const long long nc = it / nv;
    const int pos = (int)(it - nc * nv);
    const int x = pos / (n * n), yz = pos - x * n * n, y = yz / n, z = yz - y * n;
    const float* sc = in + (size_t)nc * nv;
    const float* g = gout + (size_t)nc * mv;
    const float mine = sc[pos];
    float acc = 0.0f;
    // windows o with o s <= i <= o s + k - 1
    for (int ox = max(0, (x - k + s) / s); ox <= min(m - 1, x / s); ++ox)
      for (int oy = max(0, (y - k + s) / s); oy <= min(m - 1, y / s); ++oy)
        for (int oz = max(0, (z - k + s) / s); oz <= min(m - 1, z / s); ++oz) {
          bool first = true;   // no element in front of mine is >= mine, none behind it is > mine
          for (int a = 0; a < k && first; ++a)
            for (int b = 0; b < k && first; ++b)
              for (int c = 0; c < k; ++c) {
                const int q = ((ox * s + a) * n + oy * s + b) * n + oz * s + c;
                const float v = sc[q];
                if (q < pos ? v >= mine : v > mine) { first = false; break; }
              }
          if (first) acc += g[((size_t)ox * m + oy) * m + oz];
        }
    gin[it] = masked(acc, mask, (size_t)it);
  }
}

// d total / d means and d log_var through z = eps exp(0.5 log_var) + means, plus the KLD's direct terms
__global__ __launch_bounds__(kThreads) void train_z_dgrad_kernel(const float* __restrict__ gz, const float* __restrict__ log_var,
                                                                 const float* __restrict__ gk_means,
                                                                 const float* __restrict__ gk_log_var, int N, int L,
                                                                 unsigned long long seed, float* __restrict__ g_means,
                                                                 float* __restrict__ g_log_var) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N * L) return;
  const int nb = i / L, j = i - nb * L;
  const float sd = expf(0.5f * log_var[i]);
  g_means[i] = gz[i] + gk_means[i];
  g_log_var[i] = gz[i] * (0.5f * normal_eps(seed, (unsigned)nb, (unsigned)j) * sd) + gk_log_var[i];
}

// ---- the point cloud term (train.py:230-269) --------------------------------------------------------------------------
struct PcArgs {
  int W, H, D;
  float cx0, cy0, fx, fy;   // cx0, cy0: pixel-centre-0 intrinsics (the lift's; pointset_utils.py:57)
  float tsdf;               // 0: no clamp
  float w2;                 // 2 pc_weight
};

// the columns [c0, c1) in which X / d of a point with X in [lo, hi] and depth d in [dmin, dmax] (dmin > 0) can fall:
// col = c + f X / d, one pixel of margin on either side
__device__ __forceinline__ void pc_screen_range(float lo, float hi, float dmin, float dmax, float f, float c, int n, int& c0,
                                                int& c1) {
  const float ulo = lo <= 0.0f ? lo / dmin : lo / dmax, uhi = hi >= 0.0f ? hi / dmin : hi / dmax;
  const float a = fmaf(f, ulo, c), b = fmaf(f, uhi, c);
  const float top = (float)n + 1.0f;
  c0 = max(0, (int)floorf(fminf(fmaxf(fminf(a, b), -1.0f), top)) - 1);
  c1 = min(n, (int)ceilf(fminf(fmaxf(fmaxf(a, b), -1.0f), top)) + 2);
}

// One pass over the depth pixels of sample blockIdx.y: workgroup blockIdx.x of its kPcGroups takes the 32 x 8-pixel tiles
// blockIdx.x, blockIdx.x + kPcGroups, ... of the screen rectangle of the volume's bounding sphere.  A hit pixel is
// lifted, taken to the object frame and to its cell; its eight corners are read through the loss's masked clamp; v^2
// goes to the thread's sum and 2 w v (trilinear weight) to the 64-bit fixed-point volume (integer adds: any order gives
// the same bits).  Record (sample, workgroup) = the workgroup's sum of v^2 (butterfly, then its waves in order).
__global__ __launch_bounds__(kThreads) void train_pc_term_kernel(const float* __restrict__ depth, PcArgs a,
                                                                 const float* __restrict__ pos,
                                                                 const float* __restrict__ quat,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ recon,
                                                                 const float* __restrict__ x,
                                                                 unsigned long long* __restrict__ fixed,
                                                                 float* __restrict__ records) {
  __shared__ float part[kThreads / 64];
  const int nb = blockIdx.y, D = a.D;
  const size_t vox = (size_t)D * D * D;
  const float px = pos[3 * nb], py = pos[3 * nb + 1], pz = pos[3 * nb + 2], sc = scale[nb];
  // R(q / |q|), row-major: object -> camera; a point goes the other way, o = R^T (P - p) (train.py:48-69)
  float rot[9];
  {
    const float x0 = quat[4 * nb], y0 = quat[4 * nb + 1], z0 = quat[4 * nb + 2], w0 = quat[4 * nb + 3];
    const float inv = 1.0f / sqrtf(x0 * x0 + y0 * y0 + z0 * z0 + w0 * w0);
    const float qx = x0 * inv, qy = y0 * inv, qz = z0 * inv, qw = w0 * inv;
    rot[0] = 1 - 2 * (qy * qy + qz * qz); rot[1] = 2 * (qx * qy - qw * qz);     rot[2] = 2 * (qx * qz + qw * qy);
    rot[3] = 2 * (qx * qy + qw * qz);     rot[4] = 1 - 2 * (qx * qx + qz * qz); rot[5] = 2 * (qy * qz - qw * qx);
    rot[6] = 2 * (qx * qz - qw * qy);     rot[7] = 2 * (qy * qz + qw * qx);     rot[8] = 1 - 2 * (qx * qx + qy * qy);
  }
  // the rectangle: every point of the volume lies within r of pos, so with the whole sphere in front of the camera
  // (dmin > 0) a pixel outside it lifts to a point outside the volume, whatever its depth
  int c0 = 0, c1 = a.W, r0 = 0, r1 = a.H;
  const float r = 1.7320508f * 1.001f * fabsf(sc), dmin = -pz - r, dmax = -pz + r;
  if (dmin > 0.0f && dmax < 1e30f && fabsf(px) < 1e30f && fabsf(py) < 1e30f) {
    pc_screen_range(px - r, px + r, dmin, dmax, a.fx, a.cx0, a.W, c0, c1);
    pc_screen_range(py - r, py + r, dmin, dmax, -a.fy, a.cy0, a.H, r0, r1);
  }
  const int ntx = c1 > c0 ? (c1 - c0 + kPcTileW - 1) / kPcTileW : 0, nty = r1 > r0 ? (r1 - r0 + kPcTileH - 1) / kPcTileH : 0;
  const int lx = threadIdx.x % kPcTileW, ly = threadIdx.x / kPcTileW;
  const float h = 0.5f * (float)(D - 1), top = (float)(D - 2);
  const float* __restrict__ rv = recon + (size_t)nb * vox;
  const float* __restrict__ xv = x + (size_t)nb * vox;
  unsigned long long* __restrict__ fv = fixed + (size_t)nb * vox;
  const float* __restrict__ img = depth + (size_t)nb * a.H * a.W;
  float sum = 0.0f;
  for (int t = blockIdx.x; t < ntx * nty; t += kPcGroups) {
    const int ty = t / ntx, tx = t - ty * ntx;
    const int col = c0 + tx * kPcTileW + lx, row = r0 + ty * kPcTileH + ly;
    if (col >= c1 || row >= r1) continue;
    const float d = img[(size_t)row * a.W + col];
    if (d == 0.0f) continue;
    // depth_to_pointcloud, "opengl"
    const float vx = ((float)col - a.cx0) * d / a.fx - px, vy = -((float)row - a.cy0) * d / a.fy - py, vz = -d - pz;
    const float ox = fmaf(rot[0], vx, fmaf(rot[3], vy, rot[6] * vz)) / sc;
    const float oy = fmaf(rot[1], vx, fmaf(rot[4], vy, rot[7] * vz)) / sc;
    const float oz = fmaf(rot[2], vx, fmaf(rot[5], vy, rot[8] * vz)) / sc;
    const float gx = (ox + 1.0f) * h, gy = (oy + 1.0f) * h, gz = (oz + 1.0f) * h;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    // train.py:78-80: outside where a base cell index is < 0 or > D - 2 (a NaN coordinate: outside)
    if (!(bx >= 0.0f && by >= 0.0f && bz >= 0.0f && bx <= top && by <= top && bz <= top)) continue;
    const float fx1 = gx - bx, fy1 = gy - by, fz1 = gz - bz, fx0 = 1.0f - fx1, fy0 = 1.0f - fy1, fz0 = 1.0f - fz1;
    const int lin = ((int)bx * D + (int)by) * D + (int)bz;
    float cv[8], pass[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // corner k = 4 ix + 2 iy + iz (train.py:84-91)
      const int at = lin + ((k & 4) ? D * D : 0) + ((k & 2) ? D : 0) + (k & 1);
      float rc = rv[at];
      pass[k] = 1.0f;
      if (a.tsdf > 0.0f && fabsf(xv[at]) >= a.tsdf && fabsf(rc) >= a.tsdf) {   // as train_loss_kernel
        pass[k] = (rc < -a.tsdf || rc > a.tsdf) ? 0.0f : 1.0f;
        rc = fminf(fmaxf(rc, -a.tsdf), a.tsdf);
      }
      cv[k] = rc;
    }
    // x, then y, then z (train.py:99-123)
    const float v = ((cv[0] * fx0 + cv[4] * fx1) * fy0 + (cv[2] * fx0 + cv[6] * fx1) * fy1) * fz0 +
                    ((cv[1] * fx0 + cv[5] * fx1) * fy0 + (cv[3] * fx0 + cv[7] * fx1) * fy1) * fz1;
    sum += v * v;
    const float gv = a.w2 * v;
    if (gv != 0.0f) {
      const float q = (float)(1ll << SDFR_FIXED_QUANTUM_BITS);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float wk = ((k & 4) ? fx1 : fx0) * ((k & 2) ? fy1 : fy0) * ((k & 1) ? fz1 : fz0);
        const long long c = __float2ll_rn(gv * wk * pass[k] * q);   // saturates; NaN -> 0
        if (c != 0)
          atomicAdd(fv + lin + ((k & 4) ? D * D : 0) + ((k & 2) ? D : 0) + (k & 1), (unsigned long long)c);
      }
    }
  }
#pragma unroll
  for (int dl = 32; dl >= 1; dl >>= 1) sum += __shfl_xor(sum, dl, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = part[0];
    for (int wv = 1; wv < kThreads / 64; ++wv) t += part[wv];
    records[(size_t)nb * kPcGroups + blockIdx.x] = t;
  }
}

// one workgroup: thread t sums the records t, t + 256, ... (fp64), a fixed tree over the threads; loss_pc and the total
__global__ __launch_bounds__(kThreads) void train_pc_finish_kernel(const float* __restrict__ records, long long n_records,
                                                                   float pc_weight, float* __restrict__ loss_pc,
                                                                   float* __restrict__ terms) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (long long r = threadIdx.x; r < n_records; r += kThreads) s += (double)records[r];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int half = kThreads / 2; half >= 1; half >>= 1) {
    if (threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_pc[0] = (float)red[0];
    terms[5] = (float)((double)terms[5] + (double)pc_weight * red[0]);
  }
}

// g_recon += fixed 2^-SDFR_FIXED_QUANTUM_BITS, in fp64, rounded once; a voxel no point touched keeps its bits
__global__ __launch_bounds__(kThreads) void train_pc_convert_kernel(const unsigned long long* __restrict__ fixed,
                                                                    float* __restrict__ g_recon, long long total) {
  const double quantum = 1.0 / (double)(1ll << SDFR_FIXED_QUANTUM_BITS);
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long f = (long long)fixed[i];
    if (f != 0) g_recon[i] = (float)((double)g_recon[i] + (double)f * quantum);
  }
}

// train.py:242-251 from the Philox stream (include/sdfr.h: counter {i, 0, 0, kPcStream}, 24 bits a uniform)
__global__ __launch_bounds__(kThreads) void train_pc_orientations_kernel(unsigned long long seed, int N,
                                                                         float* __restrict__ quat) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const U4 r = philox4x32_10(U4{(unsigned)i, 0u, 0u, kPcStream}, (unsigned)seed, (unsigned)(seed >> 32));
  const double k = 1.0 / 16777216.0, two_pi = 6.283185307179586;
  const double u1 = (double)(r.x >> 8) * k, u2 = (double)(r.y >> 8) * k, u3 = (double)(r.z >> 8) * k;
  const double a = sqrt(1.0 - u1), b = sqrt(u1);
  quat[4 * i] = (float)(a * sin(two_pi * u2));
  quat[4 * i + 1] = (float)(a * cos(two_pi * u2));
  quat[4 * i + 2] = (float)(b * sin(two_pi * u3));
  quat[4 * i + 3] = (float)(b * cos(two_pi * u3));
}

// ---- Adam -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v,
                                                             const int* __restrict__ step, size_t n, double lr) {
// torch's expressions as it rounds them: lerp, mul + addcmul, sqrt / sqrt(bc2) + eps, addcdiv
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int t = step[0] + 1;
  const double bc1 = 1.0 - pow(0.9, (double)t), bc2 = 1.0 - pow(0.999, (double)t);
  const float step_size = (float)(-(lr / bc1)), bc2_sqrt = (float)sqrt(bc2);
  const float gi = g[i];
  const float mi = fmaf((float)(1.0 - 0.9), gi - m[i], m[i]);
  const float vi = v[i] * 0.999f + ((float)(1.0 - 0.999) * gi) * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] = p[i] + (step_size * mi) / (sqrtf(vi) / bc2_sqrt + 1e-8f);
}
__global__ void adam_flat_advance_kernel(int* __restrict__ step) { step[0] += 1; }

template <typename K, typename... Args>
inline void launch_1d(K kernel, long long items, hipStream_t st, Args... args) {
  if (items > 0) hipLaunchKernelGGL(kernel, dim3(blocks_for(items)), dim3(kThreads), 0, st, args...);
}

inline size_t align_f(size_t floats) { return (floats + 63) & ~(size_t)63; }

// records of one conv op's weight gradient
inline int wgrad_ranges(const TrainOp& op) {
  const long long mv = (long long)op.m * op.m * op.m;
  return (int)((mv + (long long)kWgT * kWgChunks - 1) / ((long long)kWgT * kWgChunks));
}
inline long long wgrad_groups(const TrainOp& op) {   // grid.y of stage 1
  const long long R = (long long)op.cin * op.k * op.k * op.k;
  return ((op.cout + kWgCo - 1) / kWgCo) * ((R + kWgRows - 1) / kWgRows);
}
inline size_t wgrad_record_floats(const TrainOp& op, int N) {
  const size_t R = (size_t)op.cin * op.k * op.k * op.k;
  return (size_t)N * wgrad_ranges(op) * ((size_t)op.cout * R + op.cout);
}
inline long long loss_records(const sdfr_vae_trainer* t, int N) {
  const long long total = (long long)N * t->volume * t->volume * t->volume;
  return (total + (long long)kThreads * kLossItems - 1) / ((long long)kThreads * kLossItems);
}

struct Workspace {   // float offsets from the 256-byte aligned base
  size_t g[2], gz, gm, gl, records, loss, total;
};
inline Workspace workspace_layout(const sdfr_vae_trainer* t, int N) {
  Workspace w{};
  size_t off = 0;
  auto take = [&](size_t floats) { const size_t at = off; off += align_f(floats); return at; };
  w.g[0] = take((size_t)N * t->max_act);
  w.g[1] = take((size_t)N * t->max_act);
  w.gz = take((size_t)N * t->latent);
  w.gm = take((size_t)N * t->latent);
  w.gl = take((size_t)N * t->latent);
  size_t rec = 0;
  for (const TrainOp& op : t->ops)
    if (op.type == kOpConv) rec = std::max(rec, wgrad_record_floats(op, N));
  w.records = take(rec);
  w.loss = take((size_t)loss_records(t, N) * 4);
  w.total = off;
  return w;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_vae_trainer_create(int latent, int n_fc, const int* fc_out, int n_conv, const int* conv_in_size,
                                       const int* conv_cin, const int* conv_cout, const int* conv_k,
                                       const int* conv_relu, int volume, float tsdf, int n_ops, const int* h_ops,
                                       int device, sdfr_vae_trainer** out_handle) {
  if (!fc_out || !conv_in_size || !conv_cin || !conv_cout || !conv_k || !conv_relu || !out_handle ||
      (n_ops > 0 && !h_ops))
    return fail(SDFR_E_NULL, "sdfr_vae_trainer_create: NULL pointer argument");
  // the encoder: sdfr_encoder_create's checks and messages
  if (volume < 1 || volume > 512) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_create: volume %d out of range", volume);
  if (latent < 1 || latent > kMaxLatent)
    return fail(SDFR_E_INVALID, "sdfr_vae_trainer_create: latent size %d not in [1, %d]", latent, kMaxLatent);
  if (n_ops < 0 || n_ops > kMaxOps)
    return fail(SDFR_E_INVALID, "sdfr_vae_trainer_create: %d ops (at most %d)", n_ops, kMaxOps);
  if (!(tsdf >= 0.0f)) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_create: tsdf %g must be >= 0", (double)tsdf);
  std::vector<TrainOp> ops;
  long long C = 1, S = volume, off = 0, tape = 0, max_act = (long long)volume * volume * volume;
  bool flat = false;
  int first_param_op = -1;
  auto push = [&](TrainOp op) {
    op.src = ops.empty() ? kSrcX : (int)ops.size() - 1;
    op.src_relu = ops.empty() ? 0 : ops.back().relu;
    op.tape_off = tape;
    tape += op.out_f;
    max_act = std::max(max_act, std::max(op.in_f, op.out_f));
    ops.push_back(op);
  };
  for (int i = 0; i < n_ops; ++i) {
    const int* r = h_ops + (size_t)i * SDFR_ENC_OP_INTS;
    TrainOp op{};
    op.type = r[0];
    op.k = r[3]; op.s = r[4]; op.p = r[5]; op.relu = r[6] ? 1 : 0;
    op.in_f = flat ? C : C * S * S * S;
    if (r[6] != 0 && r[6] != 1) return fail(SDFR_E_INVALID, "op %d: relu flag %d", i, r[6]);
    switch (op.type) {
      case kOpConv:
      case kOpPool: {
        if (flat) return fail(SDFR_E_INVALID, "op %d: a 3-d op behind a linear op", i);
        const int cin = op.type == kOpConv ? r[1] : (int)C, cout = op.type == kOpConv ? r[2] : (int)C;
        if (op.type == kOpConv && cin != C)
          return fail(SDFR_E_INVALID, "op %d: in_channels %d, but the input has %lld channels", i, cin, C);
        if (cout < 1 || cout > 4096) return fail(SDFR_E_INVALID, "op %d: out_channels %d", i, cout);
        if (op.k < 1 || op.k > 16) return fail(SDFR_E_INVALID, "op %d: kernel_size %d", i, op.k);
        if (op.s < 1 || op.s > 16) return fail(SDFR_E_INVALID, "op %d: stride %d", i, op.s);
        if (op.p < 0 || op.p > 16 || (op.type == kOpPool && op.p != 0))
          return fail(SDFR_E_INVALID, "op %d: padding %d", i, op.p);
        const long long m = (S + 2 * op.p - op.k) / op.s + 1;
        if (S + 2 * op.p < op.k || m < 1)
          return fail(SDFR_E_INVALID, "op %d: kernel_size %d larger than the padded input %lld", i, op.k, S + 2 * op.p);
        op.cin = cin; op.cout = cout; op.n = (int)S; op.m = (int)m;
        if (op.type == kOpConv) {
          op.w_off = off;
          off += (long long)cout * cin * op.k * op.k * op.k;
          op.b_off = off;
          off += cout;
          if (first_param_op < 0) first_param_op = i;
        }
        C = cout; S = m;
        break;
      }
      case kOpLinear: {
        if (r[1] != op.in_f)
          return fail(SDFR_E_INVALID, "op %d: in_features %d, but the input has %lld", i, r[1], op.in_f);
        if (r[2] < 1) return fail(SDFR_E_INVALID, "op %d: out_features %d", i, r[2]);
        op.cin = r[1]; op.cout = r[2];
        op.w_off = off;
        off += (long long)op.cin * op.cout;
        op.b_off = off;
        off += op.cout;
        if (first_param_op < 0) first_param_op = i;
        flat = true; C = op.cout;
        break;
      }
      case kOpRelu:
        op.relu = 1;
        op.cin = op.cout = (int)C; op.n = op.m = (int)S;
        break;
      default:
        return fail(SDFR_E_INVALID, "op %d: unknown op type %d", i, op.type);
    }
    op.out_f = flat ? C : C * S * S * S;
    if (op.out_f > (1LL << 29)) return fail(SDFR_E_INVALID, "op %d: output of %lld floats per sample", i, op.out_f);
    push(op);
  }
  const long long F = flat ? C : C * S * S * S;
  if (F > (1LL << 30)) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_create: %lld features", F);
  const int n_enc = (int)ops.size();
  const long long hm_w = off, hm_b = hm_w + (long long)latent * F, hl_w = hm_b + latent, hl_b = hl_w + (long long)latent * F;
  off = hl_b + latent;
  const long long n_enc_params = off;

  // the decoder: sdfr_decoder_create's checks and messages
  if (latent > kMaxHidden || n_fc < 1 || n_fc > 8 || n_conv < 1 || n_conv > 16)
    return fail(SDFR_E_INVALID, "sdfr_vae_trainer_create: unsupported layer counts / sizes");
  int width = latent;
  for (int l = 0; l < n_fc; ++l) {
    if (fc_out[l] < 1) return fail(SDFR_E_INVALID, "fc layer %d has no outputs", l);
    if (l < n_fc - 1 && fc_out[l] > kMaxHidden)
      return fail(SDFR_E_INVALID, "hidden fc layer %d wider than %d", l, kMaxHidden);
    width = fc_out[l];
  }
  if ((long long)conv_cin[0] * conv_in_size[0] * conv_in_size[0] * conv_in_size[0] != width)
    return fail(SDFR_E_INVALID, "last fc layer (%d) does not match the first conv input", width);
  for (int l = 0; l < n_conv; ++l) {
    const int k = conv_k[l];
    if (k < 1 || conv_in_size[l] < k || conv_cin[l] < 1 || conv_cout[l] < 1)
      return fail(SDFR_E_INVALID, "conv layer %d has an invalid shape", l);
    if (conv_in_size[l] > 512) return fail(SDFR_E_INVALID, "conv layer %d: in_size %d out of range", l, conv_in_size[l]);
    if (l + 1 < n_conv && conv_cout[l] != conv_cin[l + 1])
      return fail(SDFR_E_INVALID, "conv layer %d out_channels != next in_channels", l);
    const size_t kpad = ((size_t)conv_cin[l] * k * k * k + 3) / 4 * 4;
    if (kpad * 17 * sizeof(float) > 64 * 1024)
      return fail(SDFR_E_INVALID, "conv layer %d: Cin*k^3 = %zu too large for the LDS-resident weight tile", l, kpad);
  }
  if (conv_cout[n_conv - 1] != 1) return fail(SDFR_E_INVALID, "last conv layer must have one output channel");

  width = latent;
  for (int l = 0; l < n_fc; ++l) {
    TrainOp op{};
    op.type = kOpLinear; op.cin = width; op.cout = fc_out[l]; op.relu = 1;
    op.in_f = width; op.out_f = fc_out[l];
    op.w_off = off; off += (long long)op.cin * op.cout;
    op.b_off = off; off += op.cout;
    push(op);
    if (l == 0) { ops.back().src = kSrcZ; ops.back().src_relu = 0; }
    width = fc_out[l];
  }
  long long size = conv_in_size[0];
  auto resize_to = [&](int channels, long long from, long long to) {
    TrainOp op{};
    op.type = kOpResize; op.cin = op.cout = channels; op.n = (int)from; op.m = (int)to;
    op.in_f = channels * from * from * from; op.out_f = channels * to * to * to;
    push(op);
  };
  for (int l = 0; l < n_conv; ++l) {
    if (size != conv_in_size[l]) resize_to(conv_cin[l], size, conv_in_size[l]);
    const int k = conv_k[l], n = conv_in_size[l], m = n - k + 1;
    TrainOp op{};
    op.type = kOpConv; op.cin = conv_cin[l]; op.cout = conv_cout[l]; op.n = n; op.m = m; op.k = k; op.s = 1; op.p = 0;
    op.relu = conv_relu[l] ? 1 : 0;
    op.in_f = (long long)op.cin * n * n * n; op.out_f = (long long)op.cout * m * m * m;
    op.w_off = off; off += (long long)op.cout * op.cin * k * k * k;
    op.b_off = off; off += op.cout;
    push(op);
    size = m;
  }
  if (size != volume) resize_to(1, size, volume);
  for (size_t i = 0; i < ops.size(); ++i)
    if (ops[i].type == kOpConv && wgrad_groups(ops[i]) > 65535)
      return fail(SDFR_E_INVALID, "layer %zu: %d x %d x %d^3 weights are more than the weight gradient's grid takes", i,
                  ops[i].cout, ops[i].cin, ops[i].k);
  tape -= ops.back().out_f;        // the last op writes recon
  ops.back().to_recon = 1;

  sdfr_vae_trainer* t = new sdfr_vae_trainer();
  t->device = device; t->volume = volume; t->latent = latent; t->F = (int)F; t->tsdf = tsdf;
  t->ops = ops; t->n_enc = n_enc;
  t->first_param_op = first_param_op < 0 ? n_enc : first_param_op;
  t->hm_w = hm_w; t->hm_b = hm_b; t->hl_w = hl_w; t->hl_b = hl_b;
  t->n_params = (size_t)off; t->n_enc_params = (size_t)n_enc_params;
  t->tape_f = tape; t->max_act = max_act;
  *out_handle = t;
  return 0;
}

extern "C" void sdfr_vae_trainer_destroy(sdfr_vae_trainer* t) { delete t; }

extern "C" size_t sdfr_vae_trainer_param_count(const sdfr_vae_trainer* t) { return t ? t->n_params : 0; }
extern "C" size_t sdfr_vae_trainer_encoder_param_count(const sdfr_vae_trainer* t) { return t ? t->n_enc_params : 0; }

extern "C" size_t sdfr_vae_trainer_tape_bytes(const sdfr_vae_trainer* t, int N) {
  if (!t || N < 1) return 0;
  return ((size_t)N * t->tape_f + 64) * sizeof(float);
}

extern "C" size_t sdfr_vae_trainer_workspace_bytes(const sdfr_vae_trainer* t, int N) {
  if (!t || N < 1) return 0;
  return workspace_layout(t, N).total * sizeof(float) + 256;
}

namespace {
// where op i's output / input live
inline const float* op_output(const sdfr_vae_trainer* t, int i, int N, const float* tape, const float* recon) {
  const TrainOp& op = t->ops[i];
  return op.to_recon ? recon : tape + (size_t)N * op.tape_off;
}
inline const float* op_input(const sdfr_vae_trainer* t, int i, int N, const float* tape, const float* x, const float* z) {
  const int src = t->ops[i].src;
  return src == kSrcX ? x : (src == kSrcZ ? z : tape + (size_t)N * t->ops[src].tape_off);
}
}  // namespace

extern "C" int sdfr_vae_trainer_forward(const sdfr_vae_trainer* t, const float* params, float* x, int N,
                                        unsigned long long seed, int post, float* means, float* log_var, float* z,
                                        float* recon, float* tape, size_t tape_bytes, void* stream) {
  if (!t) return fail(SDFR_E_NULL, "sdfr_vae_trainer_forward: NULL trainer");
  if (N < 1 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_forward: N=%d out of range", N);
  if (!params || !x || !means || !log_var || !z || !recon || !tape)
    return fail(SDFR_E_NULL, "sdfr_vae_trainer_forward: NULL pointer argument");
  const size_t need = sdfr_vae_trainer_tape_bytes(t, N);
  if (tape_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_vae_trainer_forward: tape %zu < %zu bytes", tape_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t voxels = (size_t)N * t->volume * t->volume * t->volume;
  if (post && t->tsdf > 0.0f)
    hipLaunchKernelGGL(clamp_kernel, dim3((unsigned)((voxels + 255) / 256)), dim3(256), 0, st, x, voxels, t->tsdf);
  for (int i = 0; i < (int)t->ops.size(); ++i) {
    if (i == t->n_enc) {
      const float* h = t->n_enc > 0 ? op_output(t, t->n_enc - 1, N, tape, recon) : x;
      launch_1d(train_heads_forward_kernel, (long long)N * t->latent * 64, st, h, t->F, t->latent, N, params, t->hm_w,
                t->hm_b, t->hl_w, t->hl_b, means, log_var, z, seed);
    }
    const TrainOp& op = t->ops[i];
    const float* in = op_input(t, i, N, tape, x, z);
    float* out = const_cast<float*>(op_output(t, i, N, tape, recon));
    switch (op.type) {
      case kOpConv:
        launch_1d(train_conv_forward_kernel, (long long)N * ((op.cout + kCT - 1) / kCT) * op.m * op.m * op.m, st, in, out,
                  op, params, N);
        break;
      case kOpLinear:
        launch_1d(train_linear_forward_kernel, (long long)N * op.cout * 64, st, in, out, op, params, N);
        break;
      case kOpPool: launch_1d(train_pool_forward_kernel, (long long)N * op.out_f, st, in, out, op, N); break;
      case kOpResize: launch_1d(train_resize_forward_kernel, (long long)N * op.out_f, st, in, out, op, N); break;
      default: launch_1d(train_relu_forward_kernel, (long long)N * op.out_f, st, in, out, (long long)N * op.out_f); break;
    }
  }
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_vae_trainer_loss(const sdfr_vae_trainer* t, const float* recon, const float* x, const float* means,
                                     const float* log_var, int N, float w_l2_small, float w_l2_large, float w_l1_small,
                                     float w_l1_large, float w_kld, int post, float* terms, float* g_recon,
                                     float* g_means, float* g_log_var, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!t) return fail(SDFR_E_NULL, "sdfr_vae_trainer_loss: NULL trainer");
  if (N < 1 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_loss: N=%d out of range", N);
  if (!recon || !x || !means || !log_var || !terms || !g_recon || !g_means || !g_log_var)
    return fail(SDFR_E_NULL, "sdfr_vae_trainer_loss: NULL pointer argument");
  if (!workspace) return fail(SDFR_E_NULL, "sdfr_vae_trainer_loss: NULL workspace");
  const size_t need = sdfr_vae_trainer_workspace_bytes(t, N);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_vae_trainer_loss: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* records = ws + workspace_layout(t, N).loss;
  const long long total = (long long)N * t->volume * t->volume * t->volume, n_records = loss_records(t, N);
  const LossArgs a{w_l2_small, w_l2_large, w_l1_small, w_l1_large, post ? w_kld : 0.0f, post ? t->tsdf : 0.0f};
  hipLaunchKernelGGL(train_loss_kernel, dim3((unsigned)n_records), dim3(kThreads), 0, st, recon, x, total, a, g_recon,
                     records);
  hipLaunchKernelGGL(train_loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, records, n_records, means, log_var,
                     (long long)N * t->latent, a, terms, g_means, g_log_var);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_vae_trainer_backward(const sdfr_vae_trainer* t, const float* params, const float* x, int N,
                                         unsigned long long seed, const float* log_var, const float* z,
                                         const float* tape, const float* recon, const float* g_recon,
                                         const float* g_means, const float* g_log_var, float* grads, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  if (!t) return fail(SDFR_E_NULL, "sdfr_vae_trainer_backward: NULL trainer");
  if (N < 1 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_backward: N=%d out of range", N);
  if (!params || !x || !log_var || !z || !tape || !recon || !g_recon || !g_means || !g_log_var || !grads)
    return fail(SDFR_E_NULL, "sdfr_vae_trainer_backward: NULL pointer argument");
  if (!workspace) return fail(SDFR_E_NULL, "sdfr_vae_trainer_backward: NULL workspace");
  const size_t need = sdfr_vae_trainer_workspace_bytes(t, N);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_vae_trainer_backward: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const Workspace lay = workspace_layout(t, N);
  float* gbuf[2] = {ws + lay.g[0], ws + lay.g[1]};
  float *gz = ws + lay.gz, *gm = ws + lay.gm, *gl = ws + lay.gl, *records = ws + lay.records;
  const int L = t->latent, n_ops = (int)t->ops.size();

  // gout: the gradient w.r.t. the output of the op at hand, its ReLU applied; gin: w.r.t. its input, masked likewise
  const float* gout = g_recon;
  int cur = 0;
  if (t->ops[n_ops - 1].relu) {
    const long long total = (long long)N * t->ops[n_ops - 1].out_f;
    launch_1d(train_mask_kernel, total, st, gout, recon, gbuf[cur], total);
    gout = gbuf[cur];
  }
  const int last = t->first_param_op < t->n_enc ? t->first_param_op : t->n_enc;   // no data gradient from here on
  for (int i = n_ops - 1; i >= last && i >= 0; --i) {
    const TrainOp& op = t->ops[i];
    const float* in = op_input(t, i, N, tape, x, z);
    const bool want_gin = i > last || i >= t->n_enc;
    const float* mask = op.src_relu ? in : nullptr;
    float* gin = op.src == kSrcZ ? gz : gbuf[cur ^ 1];
    switch (op.type) {
      case kOpConv: {
        const int R = op.cin * op.k * op.k * op.k, ranges = wgrad_ranges(op);
        if ((long long)N * ranges > 0x7fffffffLL)
          return fail(SDFR_E_INVALID, "sdfr_vae_trainer_backward: N=%d x %d position ranges exceed the grid", N, ranges);
        hipLaunchKernelGGL(train_conv_wgrad_kernel, dim3((unsigned)(N * ranges), (unsigned)wgrad_groups(op)),
                           dim3(kThreads), 0, st, gout, in, op, ranges, records);
        const long long n_w = (long long)op.cout * R, per_block = kThreads / kCombineSlices;
        hipLaunchKernelGGL(train_conv_wgrad_combine_kernel, dim3((unsigned)((n_w + op.cout + per_block - 1) / per_block)),
                           dim3(kThreads), 0, st, (const float*)records, N * ranges, n_w, (long long)op.cout,
                           grads + op.w_off, grads + op.b_off);
        if (want_gin)
          launch_1d(train_conv_dgrad_kernel, (long long)N * ((op.cin + kCT - 1) / kCT) * op.n * op.n * op.n, st, gout, gin,
                    mask, op, params, N);
        break;
      }
      case kOpLinear:
        launch_1d(train_linear_wgrad_kernel, (long long)op.cin * op.cout + op.cout, st, gout, in, op.cin, op.cout, N,
                  grads + op.w_off, grads + op.b_off);
        if (want_gin) {
          if (op.cout >= 128)
            launch_1d(train_linear_dgrad_wave_kernel, (long long)N * op.cin * 64, st, gout, params + op.w_off, op.cin,
                      op.cout, N, mask, gin);
          else
            launch_1d(train_linear_dgrad_kernel, (long long)N * op.cin, st, gout, params + op.w_off,
                      (const float*)nullptr, (const float*)nullptr, op.cin, op.cout, N, mask, gin);
        }
        break;
      case kOpPool:
        if (want_gin) launch_1d(train_pool_dgrad_kernel, (long long)N * op.in_f, st, gout, in, gin, mask, op, N);
        break;
      case kOpResize:
        if (want_gin) launch_1d(train_resize_dgrad_kernel, (long long)N * op.in_f, st, gout, gin, mask, op, N);
        break;
      default:   // a stand-alone relu: its own output is the mask
        if (want_gin)
          launch_1d(train_mask_kernel, (long long)N * op.in_f, st, gout, op_output(t, i, N, tape, nullptr), gin,
                    (long long)N * op.in_f);
        break;
    }
    if (op.src == kSrcZ) {
      // z -> means, log_var; the heads' parameter gradients; the gradient w.r.t. the encoder's features where the
      // encoder has parameters
      launch_1d(train_z_dgrad_kernel, (long long)N * L, st, (const float*)gz, log_var, g_means, g_log_var, N, L, seed, gm,
                gl);
      const float* h = t->n_enc > 0 ? op_output(t, t->n_enc - 1, N, tape, nullptr) : x;
      launch_1d(train_linear_wgrad_kernel, (long long)t->F * L + L, st, (const float*)gm, h, t->F, L, N,
                grads + t->hm_w, grads + t->hm_b);
      launch_1d(train_linear_wgrad_kernel, (long long)t->F * L + L, st, (const float*)gl, h, t->F, L, N,
                grads + t->hl_w, grads + t->hl_b);
      if (last < t->n_enc)
        launch_1d(train_linear_dgrad_kernel, (long long)N * t->F, st, (const float*)gm, params + t->hm_w,
                  (const float*)gl, params + t->hl_w, t->F, L, N,
                  t->ops[t->n_enc - 1].relu ? h : (const float*)nullptr, gbuf[cur]);
      gout = gbuf[cur];
    } else {
      cur ^= 1;
      gout = gbuf[cur];
    }
  }
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t sdfr_vae_trainer_pc_term_workspace_bytes(const sdfr_vae_trainer* t, int N) {
  if (!t || N < 1) return 0;
  const size_t vox = (size_t)t->volume * t->volume * t->volume;
  return (size_t)N * vox * sizeof(unsigned long long) + (size_t)N * kPcGroups * sizeof(float) + 256;
}

extern "C" int sdfr_vae_trainer_pc_term(const sdfr_vae_trainer* t, const float* depth, int N, int W, int H, float cx,
                                        float cy, float fx, float fy, const float* pos, const float* quat,
                                        const float* scale, const float* recon, const float* x, int post,
                                        float pc_weight, float* loss_pc, float* terms, float* g_recon, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (!t) return fail(SDFR_E_NULL, "sdfr_vae_trainer_pc_term: NULL trainer");
  if (N < 1 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_pc_term: N=%d out of range", N);
  if (W < 1 || W > 65535 || H < 1 || H > 65535)
    return fail(SDFR_E_INVALID, "sdfr_vae_trainer_pc_term: image %d x %d out of range", W, H);
  if (!(fabsf(fx) > 0.0f) || !(fabsf(fy) > 0.0f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) ||
      !std::isfinite(cy))
    return fail(SDFR_E_INVALID, "sdfr_vae_trainer_pc_term: intrinsics fx=%g fy=%g cx=%g cy=%g", (double)fx, (double)fy,
                (double)cx, (double)cy);
  if (t->volume < 2) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_pc_term: a volume of %d has no cell", t->volume);
  if (!std::isfinite(pc_weight))
    return fail(SDFR_E_INVALID, "sdfr_vae_trainer_pc_term: pc_weight %g is not finite", (double)pc_weight);
  if (!depth || !pos || !quat || !scale || !recon || !x || !loss_pc || !terms || !g_recon)
    return fail(SDFR_E_NULL, "sdfr_vae_trainer_pc_term: NULL pointer argument");
  if (!workspace) return fail(SDFR_E_NULL, "sdfr_vae_trainer_pc_term: NULL workspace");
  const size_t need = sdfr_vae_trainer_pc_term_workspace_bytes(t, N);
  if (workspace_bytes < need)
    return fail(SDFR_E_WORKSPACE, "sdfr_vae_trainer_pc_term: workspace %zu < %zu bytes", workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t vox = (size_t)t->volume * t->volume * t->volume;
  unsigned long long* fixed = (unsigned long long*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* records = (float*)(fixed + (size_t)N * vox);
  const PcArgs a{W, H, t->volume, cx - 0.5f, cy - 0.5f, fx, fy, post ? t->tsdf : 0.0f, 2.0f * pc_weight};
  zero_words_async((float*)fixed, (size_t)N * vox * 2, st);
  hipLaunchKernelGGL(train_pc_term_kernel, dim3(kPcGroups, (unsigned)N), dim3(kThreads), 0, st, depth, a, pos, quat, scale,
                     recon, x, fixed, records);
  hipLaunchKernelGGL(train_pc_finish_kernel, dim3(1), dim3(kThreads), 0, st, (const float*)records,
                     (long long)N * kPcGroups, pc_weight, loss_pc, terms);
  launch_1d(train_pc_convert_kernel, (long long)(N * vox), st, (const unsigned long long*)fixed, g_recon,
            (long long)(N * vox));
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_vae_trainer_pc_orientations(unsigned long long seed, int N, float* quat, int device, void* stream) {
  if (N < 0 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_vae_trainer_pc_orientations: N=%d out of range", N);
  if (N == 0) return 0;
  if (!quat) return fail(SDFR_E_NULL, "sdfr_vae_trainer_pc_orientations: NULL quat");
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(train_pc_orientations_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, seed, N, quat);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_adam_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int* step, size_t n,
                              double lr, int device, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step)
    return fail(SDFR_E_NULL, "sdfr_adam_flat: NULL pointer argument");
  if (n < 1 || n > (size_t)0x7fffffffu * kThreads) return fail(SDFR_E_INVALID, "sdfr_adam_flat: n=%zu out of range", n);
  if (!(lr >= 0.0)) return fail(SDFR_E_INVALID, "sdfr_adam_flat: lr %g must be >= 0", lr);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, params,
                     grads, exp_avg, exp_avg_sq, (const int*)step, n, lr);
  hipLaunchKernelGGL(adam_flat_advance_kernel, dim3(1), dim3(1), 0, st, step);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
