// encoder.hip -- the VAE encoder forward (sdf_vae.py: SDFEncoder.forward, SDFVAE.encode / sample), gfx950.
//
// An encoder is a list of ops over one sample's activation, (C, D, D, D) in torch's order, then the two heads:
//   conv    Conv3d (cubic kernel k, stride s, zero padding p, bias), ReLU fused
//   pool    MaxPool3d (kernel k, stride s, no padding, floor), ReLU fused
//   linear  Linear on the flattened activation, ReLU fused
//   relu    a ReLU with nothing in front of it to fuse into
// (Flatten is no op: (C, D, H, W) is already the flattened order.)  The heads linear_means and linear_log_var are one
// product with 2L rows; z = means + exp(0.5 log_var) eps comes out of the same launch.
//
// Launch structure, planned when the handle is created from the layer shapes alone (never from the batch):
//   * the CHAIN -- the longest tail of the op list whose activations fit in LDS -- runs in ONE launch, one workgroup
//     of 1024 threads per sample: its first op reads global memory, every later op reads the LDS buffer the op before
//     it wrote (two buffers at the two ends of the workgroup's LDS), and the heads read the last one.  Nothing of the
//     tail touches HBM but the first op's input and the outputs.
//   * the ops in front of the chain run one launch each over global memory (grid: blocks x N), ping-ponging between two
//     workspace buffers.
// The mug encoder (64 -> 31 -> 15 -> 7, 4 / 8 / 16 channels, L = 8) is conv1 over global memory (1 MiB in, 476 KB
// out per sample), then one chain launch: conv2 reads conv1's output and keeps its 108 KB in LDS, conv3 (22 KB) goes
// to the other end of the LDS, the heads read it there.
//
// Arithmetic, the same for every op wherever it runs:
//   conv    one thread per (output position, CT output channels): acc[t] = fmaf(in, w, acc[t]) over ci, a, b, c in that
//           order (taps in the padding are skipped: they add zero), then + bias, then ReLU
//   linear  one wave per output row: lane l sums the features f = l, l + 64, ... in order, then a fixed butterfly over
//           the 64 lanes; + bias; ReLU
//   pool    fmaxf over the window in (a, b, c) order
// Every output element has one owner and a fixed order of summation, no atomics: a row's results are the same bits
// whatever the batch size, its place in the batch, or the run.
//
// Noise: eps[i][j] = Box-Muller in fp64 on Philox-4x32-10 (key = seed, counter = {i, j, 0, kNoiseStream}): words
// (x, y) -> u1 = ((x >> 5) 2^26 + (y >> 6)) 2^-53, (z, w) -> u2 likewise, eps = sqrt(-2 ln(1 - u1)) cos(2 pi u2),
// rounded to fp32.  It depends on (seed, i, j) only; the first M rows of a batch equal a batch of M.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "philox.hpp"

// z = means + std * eps as two roundings, like the reference's torch expression
#pragma clang fp contract(off)

namespace {
constexpr int kOpConv = SDFR_ENC_CONV, kOpPool = SDFR_ENC_MAXPOOL, kOpLinear = SDFR_ENC_LINEAR, kOpRelu = SDFR_ENC_RELU;
constexpr int kMaxOps = 32;
constexpr int kMaxChainOps = 16;
constexpr int kMaxLatent = 512;
constexpr int kChainThreads = 512;
constexpr int kLayerThreads = 256;
constexpr size_t kChainLdsMax = 152 * 1024;     // dynamic; + the heads' 4 KiB static row <= 160 KiB
}  // namespace

struct EncOp {
  int type, cin, cout;      // linear: cin = in features, cout = out features
  int n, m, k, s, p;        // conv / pool: input side, output side, kernel, stride, padding
  int relu, ct;             // ct: conv output channels per thread (4 or 8; weights padded to a multiple)
  long long w_off, b_off;   // into the device parameter image
  long long in_f, out_f;    // floats per sample
  long long dst;            // chain ops: LDS float offset of the output
};

struct ChainDesc {
  int n_ops, F, L;          // F: the heads' input features
  long long in_stride;      // floats between samples of the chain's (global) input
  long long hw_off, hb_off; // heads: [2L][F] (means rows, then log_var rows), [2L]
  long long head_off;       // LDS float offset of the heads' input (-1: the global input)
  const EncOp* ops;         // [n_ops], device memory (read through the scalar cache)
};

struct sdfr_encoder {
  int device = 0, volume = 0, latent = 0, F = 0;
  std::vector<EncOp> ops;
  int chain_start = 0;      // ops [chain_start, n) run in the chain launch
  size_t chain_lds = 0;     // bytes
  long long global_max = 0; // floats per sample of the largest output in front of the chain
  long long hw_off = 0, hb_off = 0;
  ChainDesc chain{};        // ops: d_ops
  float* d_params = nullptr;
  EncOp* d_ops = nullptr;
};

namespace sdfr {
namespace {

// ---- the ops, each over a range of a sample's items; `src` / `dst` may point to global memory or LDS ---------------
// PAD = false (padding 0): every tap is inside, no branch between the loads -- with KC = 3 all 27 of an item's loads
// are issued before the first FMA waits (a load per branch-guarded tap waited out its latency alone: 4x slower)
template <int CT, int KC, bool PAD>
__device__ __forceinline__ void conv_items(const float* __restrict__ src, float* __restrict__ dst, const EncOp& op,
                                           const float* __restrict__ prm, int t0, int tstep) {
  const int n = op.n, m = op.m, k = KC ? KC : op.k, s = op.s, p = op.p;
  const int mv = m * m * m, nv = n * n * n, chunks = (op.cout + CT - 1) / CT, coutp = chunks * CT;
  const float* __restrict__ w = prm + op.w_off;
  const float* __restrict__ bias = prm + op.b_off;
  for (int it = t0; it < chunks * mv; it += tstep) {
    const int ch = it / mv, pos = it - ch * mv;
    const int x = pos / (m * m), yz = pos - x * m * m, y = yz / m, z = yz - y * m;
    float acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = 0.0f;
    const float* wc = w + ch * CT;
    for (int ci = 0; ci < op.cin; ++ci) {
      const float* sc = src + (size_t)ci * nv;
#pragma unroll 3
      for (int a = 0; a < k; ++a) {
        const int ix = x * s - p + a;
        if (PAD && (unsigned)ix >= (unsigned)n) continue;
#pragma unroll 3
        for (int b = 0; b < k; ++b) {
          const int iy = y * s - p + b;
          if (PAD && (unsigned)iy >= (unsigned)n) continue;
          const float* row = sc + ((size_t)ix * n + iy) * n;
          const float* wr = wc + (size_t)(((ci * k + a) * k + b) * k) * coutp;
#pragma unroll 3
          for (int c = 0; c < k; ++c) {
            const int iz = z * s - p + c;
            if (PAD && (unsigned)iz >= (unsigned)n) continue;
            const float v = row[iz];
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = fmaf(v, wr[c * coutp + t], acc[t]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int co = ch * CT + t;
      if (co < op.cout) {
        float r = acc[t] + bias[co];
        if (op.relu) r = fmaxf(r, 0.0f);
        dst[(size_t)co * mv + pos] = r;
      }
    }
  }
}

__device__ __forceinline__ void conv_any(const float* src, float* dst, const EncOp& op, const float* prm, int t0,
                                         int tstep) {
  if (op.p == 0 && op.k == 3) {
    if (op.ct == 8) conv_items<8, 3, false>(src, dst, op, prm, t0, tstep);
    else conv_items<4, 3, false>(src, dst, op, prm, t0, tstep);
  } else if (op.ct == 8) {
    if (op.k == 3) conv_items<8, 3, true>(src, dst, op, prm, t0, tstep);
    else conv_items<8, 0, true>(src, dst, op, prm, t0, tstep);
  } else {
    if (op.k == 3) conv_items<4, 3, true>(src, dst, op, prm, t0, tstep);
    else conv_items<4, 0, true>(src, dst, op, prm, t0, tstep);
  }
}

__device__ __forceinline__ void pool_items(const float* __restrict__ src, float* __restrict__ dst, const EncOp& op,
                                           int t0, int tstep) {
  const int n = op.n, m = op.m, k = op.k, s = op.s;
  const int mv = m * m * m, nv = n * n * n;
  for (int it = t0; it < op.cout * mv; it += tstep) {
    const int c = it / mv, pos = it - c * mv;
    const int x = pos / (m * m), yz = pos - x * m * m, y = yz / m, z = yz - y * m;
    const float* sc = src + (size_t)c * nv + ((size_t)(x * s) * n + y * s) * n + z * s;
    float r = -INFINITY;
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b)
        for (int cc = 0; cc < k; ++cc) r = fmaxf(r, sc[((size_t)a * n + b) * n + cc]);
    if (op.relu) r = fmaxf(r, 0.0f);
    dst[it] = r;
  }
}

__device__ __forceinline__ void relu_items(const float* __restrict__ src, float* __restrict__ dst, long long count,
                                           int t0, int tstep) {
  for (long long i = t0; i < count; i += tstep) dst[i] = fmaxf(src[i], 0.0f);
}

__device__ __forceinline__ void linear_rows(const float* __restrict__ src, float* __restrict__ dst, const EncOp& op,
                                            const float* __restrict__ prm, int wave, int nwaves, int lane) {
  for (int o = wave; o < op.cout; o += nwaves) {
    float r = wave_dot(src, prm + op.w_off + (size_t)o * op.cin, op.cin, lane) + prm[op.b_off + o];
    if (op.relu) r = fmaxf(r, 0.0f);
    if (lane == 0) dst[o] = r;
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------
// one op over global memory.  grid: (blocks, N); block 256
__global__ __launch_bounds__(kLayerThreads) void encoder_layer_kernel(const float* __restrict__ in,
                                                                      float* __restrict__ out, EncOp op,
                                                                      const float* __restrict__ prm) {
  const int nb = blockIdx.y;
  const float* src = in + (size_t)nb * op.in_f;
  float* dst = out + (size_t)nb * op.out_f;
  const int t0 = blockIdx.x * kLayerThreads + threadIdx.x, tstep = gridDim.x * kLayerThreads;
  switch (op.type) {
    case kOpConv: conv_any(src, dst, op, prm, t0, tstep); break;
    case kOpPool: pool_items(src, dst, op, t0, tstep); break;
    case kOpRelu: relu_items(src, dst, op.out_f, t0, tstep); break;
    default: linear_rows(src, dst, op, prm, t0 >> 6, tstep >> 6, threadIdx.x & 63); break;
  }
}

// the chain + heads + z, one workgroup per sample.  grid: N; block 1024; dynamic LDS: chain_lds bytes
__global__ __launch_bounds__(kChainThreads) void encoder_chain_kernel(const float* __restrict__ in, ChainDesc d,
                                                                      const float* __restrict__ prm,
                                                                      float* __restrict__ means,
                                                                      float* __restrict__ log_var,
                                                                      float* __restrict__ z, unsigned long long seed) {
  extern __shared__ float lds[];
  __shared__ float head[2 * kMaxLatent];
  const int nb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* gin = in + (size_t)nb * d.in_stride;
  const float* src = gin;
  for (int i = 0; i < d.n_ops; ++i) {
    const EncOp op = d.ops[i];
    float* dst = lds + op.dst;
    switch (op.type) {
      case kOpConv: conv_any(src, dst, op, prm, tid, kChainThreads); break;
      case kOpPool: pool_items(src, dst, op, tid, kChainThreads); break;
      case kOpRelu: relu_items(src, dst, op.out_f, tid, kChainThreads); break;
      default: linear_rows(src, dst, op, prm, wave, kChainThreads / 64, lane); break;
    }
    __syncthreads();
    src = dst;
  }
  const float* hin = d.head_off < 0 ? gin : lds + d.head_off;
  for (int o = wave; o < 2 * d.L; o += kChainThreads / 64) {
    const float r = wave_dot(hin, prm + d.hw_off + (size_t)o * d.F, d.F, lane) + prm[d.hb_off + o];
    if (lane == 0) head[o] = r;
  }
  __syncthreads();
  for (int j = tid; j < d.L; j += kChainThreads) {
    const float mu = head[j], lv = head[d.L + j];
    means[(size_t)nb * d.L + j] = mu;
    log_var[(size_t)nb * d.L + j] = lv;
    if (z) {
      const float sd = expf(0.5f * lv);
      z[(size_t)nb * d.L + j] = normal_eps(seed, (unsigned)nb, (unsigned)j) * sd + mu;
    }
  }
}

// grid: ceil(n L / 256)
__global__ __launch_bounds__(256) void normal_sample_kernel(float* __restrict__ out, long long count, int L,
                                                            unsigned long long seed) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = normal_eps(seed, (unsigned)(i / L), (unsigned)(i % L));
}

// the chain kernel's dynamic-LDS limit raised once (the mug's chain takes 130 KB); false: the runtime refused
bool chain_lds_limit() {
  static std::once_flag once;
  static bool ok = false;
  std::call_once(once, [] {
    ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&encoder_chain_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kChainLdsMax) == hipSuccess;
    if (!ok) (void)hipGetLastError();
  });
  return ok;
}

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" int sdfr_encoder_create(const float* h_params, size_t n_params, int volume, int latent, int n_ops,
                                   const int* h_ops, int device, sdfr_encoder** out_handle) {
  if (!h_params || !out_handle || (n_ops > 0 && !h_ops))
    return fail(SDFR_E_NULL, "sdfr_encoder_create: NULL pointer argument");
  if (volume < 1 || volume > 512) return fail(SDFR_E_INVALID, "sdfr_encoder_create: volume %d out of range", volume);
  if (latent < 1 || latent > kMaxLatent)
    return fail(SDFR_E_INVALID, "sdfr_encoder_create: latent size %d not in [1, %d]", latent, kMaxLatent);
  if (n_ops < 0 || n_ops > kMaxOps) return fail(SDFR_E_INVALID, "sdfr_encoder_create: %d ops (at most %d)", n_ops, kMaxOps);

  // shapes: (C, S, S, S) until a linear op, then (features)
  std::vector<EncOp> ops;
  long long C = 1, S = volume;
  bool flat = false;
  size_t need = 0;
  for (int i = 0; i < n_ops; ++i) {
    const int* r = h_ops + (size_t)i * SDFR_ENC_OP_INTS;
    EncOp op{};
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
          op.ct = cout > 4 && (long long)((cout + 7) / 8) * m * m * m >= 2 * kChainThreads ? 8 : 4;
          need += (size_t)cout * cin * op.k * op.k * op.k + cout;
        }
        C = cout; S = m;
        break;
      }
      case kOpLinear: {
        if (r[1] != op.in_f)
          return fail(SDFR_E_INVALID, "op %d: in_features %d, but the input has %lld", i, r[1], op.in_f);
        if (r[2] < 1) return fail(SDFR_E_INVALID, "op %d: out_features %d", i, r[2]);
        op.cin = r[1]; op.cout = r[2];
        need += (size_t)op.cin * op.cout + op.cout;
        flat = true; C = op.cout;
        break;
      }
      case kOpRelu:
        op.relu = 1;
        break;
      default:
        return fail(SDFR_E_INVALID, "op %d: unknown op type %d", i, op.type);
    }
    op.out_f = flat ? C : C * S * S * S;
    if (op.out_f > (1LL << 29)) return fail(SDFR_E_INVALID, "op %d: output of %lld floats per sample", i, op.out_f);
    ops.push_back(op);
  }
  const long long F = flat ? C : C * S * S * S;
  if (F > (1LL << 30)) return fail(SDFR_E_INVALID, "sdfr_encoder_create: %lld features", F);
  need += 2 * ((size_t)latent * F + latent);
  if (need != n_params)
    return fail(SDFR_E_INVALID, "parameter count %zu does not match the layer description (%zu)", n_params, need);

  // the chain: the longest tail whose ops fit in LDS (see the file comment) -- from the shapes alone
  const long long budget = (long long)(kChainLdsMax / sizeof(float));
  int s = n_ops;
  while (s > 0 && n_ops - s < kMaxChainOps && ops[s - 1].out_f <= budget &&
         (s == n_ops || ops[s].in_f + ops[s].out_f <= budget))
    --s;

  sdfr_encoder* e = new sdfr_encoder();
  e->device = device; e->volume = volume; e->latent = latent; e->F = (int)F;
  e->chain_start = s;
  long long lds_floats = 0;
  for (int i = s; i < n_ops; ++i)
    lds_floats = std::max(lds_floats, ops[i].out_f + (i > s ? ops[i].in_f : 0));
  e->chain_lds = (size_t)lds_floats * sizeof(float);
  for (int i = s; i < n_ops; ++i)
    ops[i].dst = ((i - s) & 1) ? lds_floats - ops[i].out_f : 0;   // alternate ends: an op never writes what it reads
  for (int i = 0; i < s; ++i) e->global_max = std::max(e->global_max, ops[i].out_f);

  // device image: conv weights [ci][a][b][c][cout padded to ct] and bias padded; linear [out][in], bias; heads
  std::vector<float> img;
  auto align = [&]() { while (img.size() % 64) img.push_back(0.0f); };
  const float* p = h_params;
  for (EncOp& op : ops) {
    if (op.type == kOpConv) {
      const int k3 = op.k * op.k * op.k, coutp = (op.cout + op.ct - 1) / op.ct * op.ct;
      align();
      op.w_off = (long long)img.size();
      img.resize(img.size() + (size_t)op.cin * k3 * coutp, 0.0f);
      for (int co = 0; co < op.cout; ++co)
        for (int ci = 0; ci < op.cin; ++ci)
          for (int t = 0; t < k3; ++t)
            img[op.w_off + ((size_t)ci * k3 + t) * coutp + co] = p[((size_t)co * op.cin + ci) * k3 + t];
      p += (size_t)op.cout * op.cin * k3;
      align();
      op.b_off = (long long)img.size();
      img.insert(img.end(), p, p + op.cout);
      p += op.cout;
    } else if (op.type == kOpLinear) {
      align();
      op.w_off = (long long)img.size();
      img.insert(img.end(), p, p + (size_t)op.cin * op.cout);
      p += (size_t)op.cin * op.cout;
      align();
      op.b_off = (long long)img.size();
      img.insert(img.end(), p, p + op.cout);
      p += op.cout;
    }
  }
  // heads: means W, means b, log_var W, log_var b -> [2L][F], [2L]
  align();
  e->hw_off = (long long)img.size();
  img.insert(img.end(), p, p + (size_t)latent * F);
  img.insert(img.end(), p + (size_t)latent * F + latent, p + (size_t)2 * latent * F + latent);
  e->hb_off = (long long)img.size();
  img.insert(img.end(), p + (size_t)latent * F, p + (size_t)latent * F + latent);
  img.insert(img.end(), p + (size_t)2 * latent * F + latent, p + (size_t)2 * latent * F + 2 * latent);
  e->ops = ops;
  ChainDesc& d = e->chain;
  d.n_ops = n_ops - s;
  d.F = (int)F;
  d.L = latent;
  d.in_stride = s > 0 ? ops[s - 1].out_f : (long long)volume * volume * volume;
  d.hw_off = e->hw_off;
  d.hb_off = e->hb_off;
  d.head_off = d.n_ops > 0 ? ops[n_ops - 1].dst : -1;

  hipError_t err = hipSetDevice(device);
  if (err == hipSuccess) err = hipMalloc(&e->d_params, img.size() * sizeof(float));
  if (err == hipSuccess)
    err = hipMemcpy(e->d_params, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMalloc(&e->d_ops, sizeof(EncOp) * std::max(1, d.n_ops));
  if (err == hipSuccess && d.n_ops > 0)
    err = hipMemcpy(e->d_ops, ops.data() + s, sizeof(EncOp) * d.n_ops, hipMemcpyHostToDevice);
  d.ops = e->d_ops;
  if (err != hipSuccess) {
    if (e->d_params) (void)hipFree(e->d_params);
    if (e->d_ops) (void)hipFree(e->d_ops);
    delete e;
    return hip_fail(err, "sdfr_encoder_create (device image)");
  }
  *out_handle = e;
  return 0;
}

extern "C" void sdfr_encoder_destroy(sdfr_encoder* e) {
  if (!e) return;
  if (e->d_params) {
    (void)hipSetDevice(e->device);
    (void)hipFree(e->d_params);
    (void)hipFree(e->d_ops);
  }
  delete e;
}

extern "C" size_t sdfr_encoder_workspace_bytes(const sdfr_encoder* e, int N) {
  if (!e || N <= 0) return 0;
  return 2 * (size_t)N * e->global_max * sizeof(float) + 256;
}

extern "C" int sdfr_encoder_forward(const sdfr_encoder* e, const float* x, int N, float* means, float* log_var,
                                    float* z, unsigned long long seed, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!e) return fail(SDFR_E_NULL, "sdfr_encoder_forward: NULL encoder");
  if (N < 0 || N > 65535) return fail(SDFR_E_INVALID, "sdfr_encoder_forward: N=%d out of range", N);
  if (N == 0) return 0;
  if (!x || !means || !log_var) return fail(SDFR_E_NULL, "sdfr_encoder_forward: NULL pointer argument");
  const size_t ws_need = sdfr_encoder_workspace_bytes(e, N);
  if (e->chain_start > 0 && !workspace) return fail(SDFR_E_NULL, "sdfr_encoder_forward: NULL workspace");
  if (e->chain_start > 0 && workspace_bytes < ws_need)
    return fail(SDFR_E_WORKSPACE, "sdfr_encoder_forward: workspace %zu < %zu bytes", workspace_bytes, ws_need);
  SDFR_HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;

  const float* cur = x;
  if (e->chain_start > 0) {
    const uintptr_t wsp = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    float* buf[2] = {(float*)wsp, (float*)wsp + (size_t)N * e->global_max};
    for (int i = 0; i < e->chain_start; ++i) {
      const EncOp& op = e->ops[i];
      long long items;
      if (op.type == kOpConv) items = (long long)((op.cout + op.ct - 1) / op.ct) * op.m * op.m * op.m;
      else if (op.type == kOpLinear) items = (long long)op.cout * 64;
      else items = op.out_f;
      const unsigned blocks = (unsigned)std::min<long long>((items + kLayerThreads - 1) / kLayerThreads, 1 << 20);
      hipLaunchKernelGGL(encoder_layer_kernel, dim3(blocks, N), dim3(kLayerThreads), 0, st, cur, buf[i & 1], op,
                         e->d_params);
      cur = buf[i & 1];
    }
  }

  if (e->chain_lds > 64 * 1024 && !chain_lds_limit())
    return fail(SDFR_E_INVALID, "sdfr_encoder_forward: the runtime refused %zu bytes of LDS", e->chain_lds);
  hipLaunchKernelGGL(encoder_chain_kernel, dim3(N), dim3(kChainThreads), e->chain_lds, st, cur, e->chain, e->d_params, means,
                     log_var, z, seed);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_normal_sample(float* out, int n, int L, unsigned long long seed, int device, void* stream) {
  if (n < 0 || L < 1) return fail(SDFR_E_INVALID, "sdfr_normal_sample: n=%d, L=%d", n, L);
  if (n == 0) return 0;
  if (!out) return fail(SDFR_E_NULL, "sdfr_normal_sample: NULL output");
  SDFR_HIP_TRY(hipSetDevice(device));
  const long long count = (long long)n * L;
  hipLaunchKernelGGL(normal_sample_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     out, count, L, seed);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_clamp(float* x, size_t count, float t, int device, void* stream) {
  if (!(t >= 0.0f)) return fail(SDFR_E_INVALID, "sdfr_clamp: bound %g must be >= 0", (double)t);
  if (count == 0) return 0;
  if (!x) return fail(SDFR_E_NULL, "sdfr_clamp: NULL tensor");
  if (count > (size_t)0xffffffffu * 256) return fail(SDFR_E_INVALID, "sdfr_clamp: %zu elements", count);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(clamp_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, count,
                     t);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
