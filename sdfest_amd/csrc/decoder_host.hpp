// decoder_host.hpp -- the host's copy of the index arithmetic of decoder.hip's kernels, one statement of each formula.
// The host sizes LDS, picks tiles and builds the tables the kernels index with, so these functions repeat the kernels'
// float operations exactly (resize_axis, resize_weight, resize_sources).  Plain C++: no HIP calls, no kernels; included
// by decoder.hip only.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <type_traits>
#include <vector>

namespace sdfr {

// resize_axis on the host: the two sources of fine index dd and the weight of the second
inline void host_resize_axis(int dd, float ratio, int ni, int& i0, int& i1, float& l1) {
  float sp = fmaf(ratio, (float)dd + 0.5f, -0.5f);
  sp = sp < 0.0f ? 0.0f : sp;
  i0 = std::min((int)sp, ni - 1);
  i1 = i0 + (i0 < ni - 1 ? 1 : 0);
  l1 = sp - (float)i0;
}

// resize_weight on the host: what fine index d takes from coarse index i (ratio = n_in / n_out)
inline float host_resize_weight(int d, int i, float ratio, int n_in) {
  int i0, i1;
  float l1;
  host_resize_axis(d, ratio, n_in, i0, i1, l1);
  return (i0 == i ? 1.0f - l1 : 0.0f) + (i1 == i ? l1 : 0.0f);
}

// Coarse indices (of ni) under a tile's patch of a resize ni -> n, worst tile: the tiles start every T fine indices
// below m, and a patch is I wide (cut at n).
inline int host_resize_span(int ni, int n, int m, int T, int I) {
  const float ratio = (float)ni / (float)n;
  int worst = 0;
  for (int t0 = 0; t0 < m; t0 += T) {
    int lo, hi, t;
    float f;
    host_resize_axis(t0, ratio, ni, lo, t, f);
    host_resize_axis(std::min(t0 + I, n) - 1, ratio, ni, t, hi, f);
    worst = std::max(worst, hi - lo + 1);
  }
  return worst;
}

// The transposed resize n_out -> n_in: per coarse index i the fine indices that may feed it (c0 .. c1: resize_sources'
// candidate range) and those that do (lo .. hi: the zero-weight ends dropped; hi < lo where none does).
struct ResizeSources {
  int n_in = 0, n_out = 0;
  std::vector<int> c0, c1, lo, hi;
  int max_span = 1, max_taps = 1;   // longest candidate range, longest exact range
  bool empty = false;               // some coarse index has no source at all
};
inline ResizeSources host_resize_sources(int n_in, int n_out) {
  ResizeSources r;
  r.n_in = n_in;
  r.n_out = n_out;
  r.c0.resize(n_in); r.c1.resize(n_in); r.lo.resize(n_in); r.hi.resize(n_in);
  const float ratio = (float)n_in / (float)n_out, inv = (float)n_out / (float)n_in;
  for (int i = 0; i < n_in; ++i) {
    int d0 = std::max((int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1, 0);
    int d1 = std::min((int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1, n_out - 1);
    r.c0[i] = d0; r.c1[i] = d1;
    r.max_span = std::max(r.max_span, d1 - d0 + 1);
    while (d0 <= d1 && host_resize_weight(d0, i, ratio, n_in) == 0.0f) ++d0;
    while (d1 >= d0 && host_resize_weight(d1, i, ratio, n_in) == 0.0f) --d1;
    r.lo[i] = d0; r.hi[i] = d1;
    if (d0 > d1) r.empty = true;
    r.max_taps = std::max(r.max_taps, d1 - d0 + 1);
  }
  return r;
}

// Few latents, columns per workgroup of the fused MFMA forms (m^2 columns, ZT z-tiles each): the smallest tile that
// gives every workgroup a CU of its own (<= 16 MFMA tiles each).  others: workgroups per tile, the other grid axes x N.
inline void few_latent_tile(int m, int ZT, long long others, int& TX, int& TY) {
  static const int kShapes[][2] = {{1, 1}, {1, 2}, {2, 2}, {2, 3}, {3, 3}, {2, 4}, {3, 4}, {4, 4}};
  TX = TY = 1;
  for (const auto& sh : kShapes) {
    if (sh[0] * sh[1] * ZT > 16) break;
    TX = sh[0]; TY = sh[1];
    if ((long long)((m + TX - 1) / TX) * ((m + TY - 1) / TY) * others <= 256) break;
  }
}

// A convolution layer's parameters [co][ci][k][k][k] as the two contractions read them, out[x] = sum w(a,b,c) in[x + (a,b,c)]
struct ConvWeights {
  const float* W = nullptr;
  const float* bias = nullptr;
  int ci_n = 0, k = 0;
  // the layer itself: weight of input channel ci at tap (a,b,c) for output channel co
  float corr(int co, int ci, int a, int b, int c) const {
    return W[((size_t)co * ci_n + ci) * (k * k * k) + (a * k + b) * k + c];
  }
  // its data gradient: the channels swap roles, the taps are flipped (the input is the zero-padded output gradient)
  float grad(int co, int ci, int a, int b, int c) const { return corr(ci, co, k - 1 - a, k - 1 - b, k - 1 - c); }
};

// Row kk of an im2col matrix over k x k x kz taps (kz > k: the z-grouped forms): its channel and tap
struct Tap {
  int ch, a, b, c;
};
inline Tap tap_of(int kk, int k, int kz) {
  const int r = kk % (k * k * kz);
  return {kk / (k * k * kz), r / (k * kz), (r / kz) % k, r % kz};
}

// A runtime integer from a fixed list as a template argument: calls f(std::integral_constant<int, V>) for the V that
// equals v; false (and no call) where none does.
template <int... Vs, class F>
bool dispatch_int(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// ... with the list's last value as the catch-all
template <int... Vs, class F>
void dispatch_int_else_last(int v, F&& f) {
  constexpr int vs[] = {Vs...};
  constexpr int last = vs[sizeof...(Vs) - 1];
  if (!dispatch_int<Vs...>(v, f)) f(std::integral_constant<int, last>{});
}

}  // namespace sdfr
