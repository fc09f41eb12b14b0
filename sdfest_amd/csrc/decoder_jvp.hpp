// decoder_jvp.hpp -- what decoder_jvp.hip knows of a decoder handle: the layer description and where each layer's
// weights lie in the handle's device image.  Filled by decoder_jvp_desc (decoder.hip, next to decoder_fc_desc), so that
// the handle's definition stays where it is.
#pragma once

#include "decoder_fc.hpp"

namespace sdfr {

struct JvpDesc {
  int device, latent, n_conv, volume;
  float tsdf;
  // per convolution layer: the size its convolution reads at, channels, kernel, ReLU, "1x1x1 swapped with its resize"
  // (the convolution then runs at `prev`, the size of the tensor that enters the layer, and the resize follows), the
  // rows of its weight matrix [co / 16][kpad][16] (row = ci k^3 + (a k + b) k + c) and the matrix's float offset
  int in_size[16], cin[16], cout[16], k[16], relu[16], swap[16], prev[16], kpad[16];
  long long w_off[16];
  long long tape_fc_off, tape_conv_off[16];   // float offsets of the tape's slots, per latent
  long long max_act;                          // floats of the largest tensor between two steps, per latent
  const float* params;                        // the device image
  FcDesc fc;
};

void decoder_jvp_desc(const sdfr_decoder* d, JvpDesc* out);

}  // namespace sdfr
