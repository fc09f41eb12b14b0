// decoder_jvp.hip -- forward-mode derivative of the decoder w.r.t. the latent (gfx950 only): sdfr_decoder_jvp, and
// sdfr_sdf_std, the per-voxel standard deviation that a latent covariance gives the decoded volume.
//
// The decoder is Linear, ReLU, trilinear resize and Conv3d.  Its derivative along a latent direction is the same chain
// without the biases and with every ReLU replaced by the mask [activation > 0] of the PRIMAL run: the N T tangents of a
// call are a batch of rows r = n T + t through that masked, bias-free network, row r taking its masks from latent n of
// the tape a preceding sdfr_decoder_forward wrote.  (The tape holds the wide Linear layer's output and every ReLU'd
// convolution output; the small leading Linear layers are recomputed from z with the forward's own fmaf chains -- bias
// first, inputs ascending --, as the VJP recomputes them: the same bits, so the same masks.)
//
// Every step is an fmaf chain in a fixed order by one thread per output (channels, then taps a, b, c ascending), the
// resize is resize3_kernel's expression tree: no atomics, the same bits on every call, and a row never reads another
// latent's data.  A layer's weights are read from the handle's device image ([co / 16][kpad][16], the MFMA forms'
// matrix) at wave-uniform addresses: scalar loads.  The last step -- the final resize, or the last convolution where
// the volume needs none -- stores voxel-major, jac[n][voxel][t] with the row padded to Tp floats, and applies the clamp
// mask; there is no transposing launch.  The call runs once per uncertainty query, not per iteration: the inputs of a
// convolution come straight from L2 (a layer of the mug decoder at T = 8 is 8 x 4 x 32^3 floats = 4 MiB).
#include <cmath>
#include <type_traits>

#include "common.hpp"
#include "decoder_jvp.hpp"

namespace sdfr {
namespace {

// resize_axis / blend of decoder.hip's resize3_kernel (ATen upsample_trilinear3d, align_corners=False), term for term
__device__ __forceinline__ void jvp_resize_axis(int d, float ratio, int n_in, int& i0, int& i1, float& l1) {
  float src = fmaf(ratio, (float)d + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  i0 = min((int)src, n_in - 1);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}
__device__ __forceinline__ float jvp_blend(float w0, float a, float w1, float b) { return fmaf(w0, a, w1 * b); }

// where a step's last form stores: jac[n][voxel][t], Tp floats per voxel; the thread of t = T - 1 zeroes the padding
__device__ __forceinline__ void store_final(float* __restrict__ jac, size_t n, size_t vox, size_t v, int t, int T, int Tp,
                                            float value) {
  float* row = jac + (n * vox + v) * (size_t)Tp;
  row[t] = value;
  if (t == T - 1)
    for (int p = T; p < Tp; ++p) row[p] = 0.0f;
}

// The Linear stack.  grid (ceil(out_last / 256), N T).  The leading layers' primal activations (from z[n]) and their
// tangents side by side in LDS; the wide layer's mask is the tape's.  tangents == NULL: row t is the basis vector e_t.
__global__ __launch_bounds__(kFcBlock) void jvp_fc_kernel(const float* __restrict__ params, FcDesc d,
                                                          const float* __restrict__ z,
                                                          const float* __restrict__ tangents, int T,
                                                          const float* __restrict__ tape_fc, float* __restrict__ out) {
  __shared__ float act[2][kMaxHidden], tan[2][kMaxHidden];
  const int tid = threadIdx.x, row = blockIdx.y, n = row / T, t = row - n * T;
  int cur = 0;
  for (int i = tid; i < d.width[0]; i += kFcBlock) {
    act[0][i] = z[(size_t)n * d.width[0] + i];
    tan[0][i] = tangents ? tangents[(size_t)row * d.width[0] + i] : (i == t ? 1.0f : 0.0f);
  }
  __syncthreads();
  for (int l = 0; l < d.n_fc - 1; ++l) {
    const int win = d.width[l], wout = d.width[l + 1];
    const float* w = params + d.w_off[l];
    const float* b = params + d.b_off[l];
    for (int o = tid; o < wout; o += kFcBlock) {
      float acc = b[o], dacc = 0.0f;
      for (int i = 0; i < win; ++i) {
        const float wi = w[(size_t)o * win + i];
        acc = fmaf(wi, act[cur][i], acc);
        dacc = fmaf(wi, tan[cur][i], dacc);
      }
      act[cur ^ 1][o] = fmaxf(acc, 0.0f);
      tan[cur ^ 1][o] = acc > 0.0f ? dacc : 0.0f;
    }
    __syncthreads();
    cur ^= 1;
  }
  const int l = d.n_fc - 1, win = d.width[l], wout = d.width[l + 1];
  const int o = blockIdx.x * kFcBlock + tid;
  if (o < wout) {
    const float* wt = params + d.w_off[l];   // transposed: [in][out]
    float dacc = 0.0f;
#pragma unroll 16
    for (int i = 0; i < win; ++i) dacc = fmaf(wt[(size_t)i * wout + o], tan[cur][i], dacc);
    out[(size_t)row * wout + o] = tape_fc[(size_t)n * wout + o] > 0.0f ? dacc : 0.0f;
  }
}

// A valid convolution without its bias.  grid (ceil(m^3 / 256), cout, N T): in [row][cin][n^3] -> out [row][cout][m^3],
// m = n - k + 1.  mask (NULL: none): the layer's tape slot, [N][cout][m^3]; the output is kept where it is > 0.
// FINAL (cout == 1): the store goes to jac, zero where clamp_out (NULL: no clamp) sits on the clamp.
// KT: the kernel size at compile time (1, 3), 0 = any.  With the taps unrolled a channel's k^3 weights and inputs are in
// flight together; the runtime-k loop waits for one scalar and one vector load per fmaf (a kernel trace of the mug
// decoder's JVP put 100 us into each 3x3x3 layer whatever its size, 320 of the call's 357 us).  The chain's order is the
// same either way: the same bits.
template <bool FINAL, int KT>
__global__ __launch_bounds__(256) void jvp_conv_kernel(const float* __restrict__ in, const float* __restrict__ wmat,
                                                       int kpad, int cin, int cout, int kr, int n, int T,
                                                       const float* __restrict__ mask,
                                                       const float* __restrict__ clamp_out, float tsdf, int Tp,
                                                       float* __restrict__ out) {
  const int k = KT > 0 ? KT : kr;
  const int m = n - k + 1;
  const size_t vo = (size_t)m * m * m, vi = (size_t)n * n * n;
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= vo) return;
  const int co = blockIdx.y, row = blockIdx.z, nl = row / T, t = row - nl * T;
  const int zc = (int)(v % m), yc = (int)((v / m) % m), xc = (int)(v / ((size_t)m * m));
  // column co of the weight matrix [co / 16][kpad][16]: a wave-uniform address per row
  const float* w = wmat + (size_t)(co >> 4) * kpad * 16 + (co & 15);
  const float* src = in + (size_t)row * cin * vi + ((size_t)xc * n + yc) * n + zc;
  float acc = 0.0f;
  for (int ci = 0; ci < cin; ++ci) {
    const float* wc = w + (size_t)ci * (k * k * k) * 16;
    const float* pc = src + (size_t)ci * vi;
    if constexpr (KT > 0) {
      constexpr int K1 = KT, K3 = KT * KT * KT;
      float wv[K3], xv[K3];
#pragma unroll
      for (int e = 0; e < K3; ++e) {
        wv[e] = wc[e * 16];
        xv[e] = pc[((size_t)(e / (K1 * K1)) * n + (e / K1) % K1) * n + e % K1];
      }
#pragma unroll
      for (int e = 0; e < K3; ++e) acc = fmaf(wv[e], xv[e], acc);
    } else {
      int kk = 0;
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
          const float* p = pc + ((size_t)a * n + b) * n;
          for (int c = 0; c < k; ++c, ++kk) acc = fmaf(wc[(size_t)kk * 16], p[c], acc);
        }
    }
  }
  if (mask && !(mask[((size_t)nl * cout + co) * vo + v] > 0.0f)) acc = 0.0f;
  if (FINAL) {
    if (clamp_out && !(fabsf(clamp_out[(size_t)nl * vo + v]) < tsdf)) acc = 0.0f;
    store_final(out, (size_t)nl, vo, v, t, T, Tp, acc);
  } else {
    out[((size_t)row * cout + co) * vo + v] = acc;
  }
}

// The trilinear resize, resize3_kernel's expression.  grid (ceil(C n_out^3 / 256), N): a thread forms its output's
// sources and weights once and walks the T rows of its latent.  mask: [N][C][n_out^3] as above.  FINAL (C == 1): the
// thread stores its voxel's T tangents one after the other, then the padding.
template <bool FINAL>
__global__ __launch_bounds__(256) void jvp_resize_kernel(const float* __restrict__ in, int C, int n_in, int n_out, int T,
                                                         const float* __restrict__ mask,
                                                         const float* __restrict__ clamp_out, float tsdf, int Tp,
                                                         float* __restrict__ out) {
  const size_t vo = (size_t)n_out * n_out * n_out, vi = (size_t)n_in * n_in * n_in;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)C * vo) return;
  const int n = blockIdx.y;
  const int c = (int)(idx / vo);
  const size_t r = idx - (size_t)c * vo;
  const int z = (int)(r % n_out), y = (int)((r / n_out) % n_out), x = (int)(r / ((size_t)n_out * n_out));
  const float ratio = (float)n_in / (float)n_out;
  int x0, x1, y0, y1, z0, z1;
  float lx, ly, lz;
  jvp_resize_axis(x, ratio, n_in, x0, x1, lx);
  jvp_resize_axis(y, ratio, n_in, y0, y1, ly);
  jvp_resize_axis(z, ratio, n_in, z0, z1, lz);
  const float wx0 = 1.0f - lx, wy0 = 1.0f - ly, wz0 = 1.0f - lz;
  bool keep = true;
  if (mask) keep = mask[((size_t)n * C + c) * vo + r] > 0.0f;
  if (FINAL && clamp_out) keep = keep && fabsf(clamp_out[(size_t)n * vo + r]) < tsdf;
  for (int t = 0; t < T; ++t) {
    const size_t row = (size_t)n * T + t;
    const float* p = in + (row * C + c) * vi;
#define AT(ix, iy, iz) p[((size_t)(ix) * n_in + (iy)) * n_in + (iz)]
    float v = jvp_blend(wx0, jvp_blend(wy0, jvp_blend(wz0, AT(x0, y0, z0), lz, AT(x0, y0, z1)),
                                       ly, jvp_blend(wz0, AT(x0, y1, z0), lz, AT(x0, y1, z1))),
                        lx, jvp_blend(wy0, jvp_blend(wz0, AT(x1, y0, z0), lz, AT(x1, y0, z1)),
                                      ly, jvp_blend(wz0, AT(x1, y1, z0), lz, AT(x1, y1, z1))));
#undef AT
    if (!keep) v = 0.0f;
    if (FINAL) store_final(out, (size_t)n, vo, r, t, T, Tp, v);
    else out[(row * C + c) * vo + r] = v;
  }
}

// sqrt(max(0, j^T S j)) per voxel: one thread per voxel, the latent's T x T covariance in LDS, fp64 sums in a fixed
// order (rows, then columns, ascending).  grid (ceil(voxels / 256), K)
__global__ __launch_bounds__(256) void sdf_std_kernel(const float* __restrict__ jac, long long voxels, int Tp, int T,
                                                      const double* __restrict__ cov, float* __restrict__ out) {
  __shared__ double S[SDFR_INFO_MAX_TANGENTS * SDFR_INFO_MAX_TANGENTS];
  const int n = blockIdx.y;
  for (int e = threadIdx.x; e < T * T; e += 256) S[e] = cov[(size_t)n * T * T + e];
  __syncthreads();
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= voxels) return;
  const float* j = jac + ((size_t)n * voxels + v) * Tp;
  double q = 0.0;   // (the voxel's row is at most 96 bytes: after the first pass its loads hit the L1)
  for (int a = 0; a < T; ++a) {
    double s = 0.0;
    for (int b = 0; b < T; ++b) s = fma(S[a * T + b], (double)j[b], s);
    q = fma((double)j[a], s, q);
  }
  out[(size_t)n * voxels + v] = (float)sqrt(q < 0.0 ? 0.0 : q);   // (a NaN covariance stays NaN)
}

inline int padded(int T) { return (T + 3) & ~3; }
inline float* aligned256(void* p) { return (float*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

}  // namespace
}  // namespace sdfr

using namespace sdfr;

extern "C" size_t sdfr_decoder_jvp_workspace_bytes(const sdfr_decoder* d, int N, int T) {
  if (!d || N < 1 || T < 1 || T > SDFR_INFO_MAX_TANGENTS || (long long)N * T > 65535) return 0;
  JvpDesc j;
  decoder_jvp_desc(d, &j);
  return 2 * (size_t)N * T * (size_t)j.max_act * sizeof(float) + 512;
}

extern "C" int sdfr_decoder_jvp(const sdfr_decoder* d, const float* z, const float* tape, const float* out,
                                const float* tangents, int N, int T, int enforce_tsdf, float* jac, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* fn = "sdfr_decoder_jvp";
  if (!d) return fail(SDFR_E_NULL, "%s: NULL decoder", fn);
  if (N < 1 || T < 1 || T > SDFR_INFO_MAX_TANGENTS || (long long)N * T > 65535)
    return fail(SDFR_E_INVALID, "%s: N=%d, T=%d: need N >= 1, 1 <= T <= %d and N T <= 65535", fn, N, T,
                SDFR_INFO_MAX_TANGENTS);
  JvpDesc j;
  decoder_jvp_desc(d, &j);
  if (!tangents && T != j.latent)
    return fail(SDFR_E_INVALID, "%s: tangents == NULL is the identity basis, T=%d must be the latent size %d", fn, T, j.latent);
  const bool clamp = enforce_tsdf && j.tsdf > 0.0f;
  if (!z || !tape || !jac || !workspace || (clamp && !out)) return fail(SDFR_E_NULL, "%s: NULL pointer argument", fn);
  if ((uintptr_t)jac & 15u) return fail(SDFR_E_INVALID, "%s: jac must be 16-byte aligned", fn);
  const size_t need = sdfr_decoder_jvp_workspace_bytes(d, N, T);
  if (workspace_bytes < need) return fail(SDFR_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  SDFR_HIP_TRY(hipSetDevice(j.device));
  hipStream_t st = (hipStream_t)stream;
  const int rows = N * T, Tp = padded(T), nc = j.n_conv;
  float* buf[2] = {aligned256(workspace), nullptr};
  buf[1] = buf[0] + (size_t)rows * j.max_act;
  const float* clamp_out = clamp ? out : nullptr;
  auto slot = [&](int l) { return tape + (size_t)N * j.tape_conv_off[l]; };   // the tape is slot-major: [slot][N][...]
  auto blocks = [](size_t count) { return (unsigned)((count + 255) / 256); };
  const int m_last = j.in_size[nc - 1] - j.k[nc - 1] + 1;

  int cur = 0;
  const int wide = j.fc.width[j.fc.n_fc];
  hipLaunchKernelGGL(jvp_fc_kernel, dim3(blocks((size_t)wide), (unsigned)rows), dim3(kFcBlock), 0, st, j.params, j.fc, z,
                     tangents, T, tape + (size_t)N * j.tape_fc_off, buf[cur]);
  // src = buf[cur]; a step writes the other buffer, the call's last step jac
  auto resize = [&](int C, int ni, int no, const float* mask, bool last) {
    const dim3 grid(blocks((size_t)C * no * no * no), (unsigned)N);
    if (last)
      hipLaunchKernelGGL((jvp_resize_kernel<true>), grid, dim3(256), 0, st, buf[cur], C, ni, no, T, mask, clamp_out,
                         j.tsdf, Tp, jac);
    else
      hipLaunchKernelGGL((jvp_resize_kernel<false>), grid, dim3(256), 0, st, buf[cur], C, ni, no, T, mask,
                         (const float*)nullptr, 0.0f, Tp, buf[cur ^ 1]);
    cur ^= 1;
  };
  auto conv = [&](int l, int n, const float* mask, bool last) {
    const int m = n - j.k[l] + 1;
    const dim3 grid(blocks((size_t)m * m * m), (unsigned)j.cout[l], (unsigned)rows);
    const float* w = j.params + j.w_off[l];
    const int kt = j.k[l] == 1 || j.k[l] == 3 ? j.k[l] : 0;
    auto launch = [&](auto last_c, auto kt_c) {
      hipLaunchKernelGGL((jvp_conv_kernel<decltype(last_c)::value, decltype(kt_c)::value>), grid, dim3(256), 0, st, buf[cur],
                         w, j.kpad[l], j.cin[l], j.cout[l], j.k[l], n, T, mask, last ? clamp_out : (const float*)nullptr,
                         last ? j.tsdf : 0.0f, Tp, last ? jac : buf[cur ^ 1]);
    };
    auto with_kt = [&](auto last_c) {
      if (kt == 1) launch(last_c, std::integral_constant<int, 1>{});
      else if (kt == 3) launch(last_c, std::integral_constant<int, 3>{});
      else launch(last_c, std::integral_constant<int, 0>{});
    };
    if (last) with_kt(std::true_type{});
    else with_kt(std::false_type{});
    cur ^= 1;
  };
  for (int l = 0; l < nc; ++l) {
    const float* mask = j.relu[l] ? slot(l) : nullptr;
    const bool last_layer = l == nc - 1 && m_last == j.volume;
    if (j.swap[l]) {   // the 1x1x1 convolution at the incoming size, then the layer's resize (with its ReLU mask)
      conv(l, j.prev[l], nullptr, false);
      resize(j.cout[l], j.prev[l], j.in_size[l], mask, last_layer);
    } else {
      if (j.prev[l] != j.in_size[l]) resize(j.cin[l], j.prev[l], j.in_size[l], nullptr, false);
      conv(l, j.in_size[l], mask, last_layer);
    }
  }
  if (m_last != j.volume) resize(1, m_last, j.volume, nullptr, true);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int sdfr_sdf_std(const float* jac, int K, long long voxels, int Tp, int T, const double* covariance,
                            float* out, int device, void* stream) {
  const char* fn = "sdfr_sdf_std";
  if (K < 1 || K > 65535 || voxels < 1 || voxels > (1ll << 31) || T < 1 || T > SDFR_INFO_MAX_TANGENTS || Tp < T ||
      (Tp & 3))
    return fail(SDFR_E_INVALID, "%s: K=%d, voxels=%lld, T=%d, Tp=%d: need 1 <= K <= 65535, 1 <= voxels <= 2^31, "
                "1 <= T <= %d, Tp >= T a multiple of 4", fn, K, voxels, T, Tp, SDFR_INFO_MAX_TANGENTS);
  if (!jac || !covariance || !out) return fail(SDFR_E_INVALID, "%s: NULL pointer argument", fn);
  if (((uintptr_t)jac & 15u) || ((uintptr_t)covariance & 7u))
    return fail(SDFR_E_INVALID, "%s: jac must be 16-byte and covariance 8-byte aligned", fn);
  SDFR_HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(sdf_std_kernel, dim3((unsigned)((voxels + 255) / 256), (unsigned)K), dim3(256), 0,
                     (hipStream_t)stream, jac, voxels, Tp, T, covariance, out);
  SDFR_HIP_TRY(hipGetLastError());
  return 0;
}
