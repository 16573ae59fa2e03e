// fleet_amd/csrc/cifar_forward.h -- the Driver's test() (Driver/src/main/c++/
// cppNN_backend.cpp:53-75) on the reference's CIFAR network (:128-138), per image, host +
// device on eval_forward.h's pattern over teacher_math.h: cifar_kernels.hip runs these
// functions per lane, cifar_forward_host / cifar_reduce_host below run them in plain
// loops, and tests/native/check_cifar_forward.cpp checks the latter against the
// reference's bits, every layer's node included.
//
//   I1 input 32 32 3 | C1 convolution 3 16 1 elu | P1 max_pool 3 2 | C2 convolution 3 64 1 elu
//   | P2 max_pool 4 4 | local4 fully_connected 384 relu | local5 fully_connected 192 relu
//   | FC2 fully_connected N softmax, N = 10 or 100
//
// Per image (commonLib/cppNN/network.h:510-515 predict_class, :523-592 forward at
// temperature 1, train == 0):
//   convolution (layer.h:805-872, the non-AVX unwrap_aligned_NxN + dotsum_unwrapped_NxN of
//     core_math.h:136-148, :172-185): every output is one running binary32 sum from 0, the
//     input channel the outer loop, the nine taps the inner one in row-major order, a
//     rounded product and a rounded add per step; the weight of map m, channel k, tap i
//     is w[(m + k*maps)*9 + i]; then elu::fc with the map's bias (activation.h:172-179);
//   max_pool (layer.h:363-456): the maximum starts at the window's first element and
//     is replaced on a strict `max < n`, row-major: ties keep the first, a NaN in first
//     place stays, a later NaN never wins; no bias, no activation;
//   fully_connected (layer.h:200-239, the else arm: P2's maps are not padded):
//     node = 0.f + dot(top, w + j*cols, size), dot the default arm of core_math.h:67-70 (a
//     loop from v = 0), then relu::f with the bias (activation.h:199-206):
//     (in + b) < 0 ? 0 : in + b, so -0 and NaN pass through; FC2 takes softmax::f
//     (activation.h:273-286), which adds no bias;
//   arg_max, mse::cost against the label and test()'s closing lines: eval_forward.h's.
//
// The reference keeps C1's 30x30 maps 904 floats apart, not 900 (layer.h:765 asks for a
// channel-aligned matrix, core_math.h:590-598 rounds the map up to 8 floats), and its
// dotsum walks 8 outputs at a time, so it also accumulates into the four padding
// elements behind each map. Nothing reads them: P1's windows end at row 29, column 29.
// Here the maps are 900 apart, on the host and in LDS, and the padding does not exist.
// P1 (14x14x16, 196 apart), C2 (12x12x64, 144 apart) and P2 (3x3x64, 9 apart) are
// unpadded in the reference too.
#pragma once
#include <stdint.h>

#include "eval_forward.h"
#include "teacher_math.h"

namespace fleet {
namespace cifarnet {

constexpr int kIn = 32, kChans = 3, kC1 = 30, kP1 = 14, kC2 = 12, kP2 = 3;
constexpr int kMaps1 = 16, kMaps2 = 64, kFc4 = 384, kFc5 = 192, kMaxClasses = 100;
constexpr int kInMap = kIn * kIn;                  // 1024
constexpr int kPix = kChans * kInMap;              // 3072
constexpr int kC1Map = kC1 * kC1;                  // 900 (the reference: 904, see above)
constexpr int kC1Out = kMaps1 * kC1Map;            // 14400
constexpr int kP1Map = kP1 * kP1;                  // 196
constexpr int kP1Out = kMaps1 * kP1Map;            // 3136
constexpr int kC2Map = kC2 * kC2;                  // 144
constexpr int kC2Out = kMaps2 * kC2Map;            // 9216
constexpr int kFcIn = kMaps2 * kP2 * kP2;          // 576: local4 reads P2 as c*9 + y*3 + x
constexpr int kW1 = 0, kW2 = kW1 + kMaps1 * kChans * 9, kW4 = kW2 + kMaps2 * kMaps1 * 9;
constexpr int kW5 = kW4 + kFc4 * kFcIn, kWfc = kW5 + kFc5 * kFc4;  // 0, 432, 9648, 230832, 304560
constexpr int kB1 = 0, kB2 = kB1 + kMaps1, kB4 = kB2 + kMaps2, kB5 = kB4 + kFc4, kBfc = kB5 + kFc5;  // .., 656
constexpr int kConvMaps = 4;  // maps whose sums one conv_taps call advances from one 3x3 patch

FLEET_TM bool classes_ok(int classes) { return classes == 10 || classes == 100; }
FLEET_TM int weight_count(int classes) { return classes_ok(classes) ? kWfc + classes * kFc5 : 0; }  // 306480, 323760
FLEET_TM int bias_count(int classes) { return classes_ok(classes) ? kBfc + classes : 0; }           // 666, 756

// the 3x3 of one input channel (src: rows of row_len floats) under output place (y, x)
FLEET_TM void conv_patch(float (&patch)[9], const float* src, int row_len, int y, int x) {
#pragma unroll
  for (int i = 0; i < 9; ++i) patch[i] = src[(y + i / 3) * row_len + x + i % 3];
}

// one input channel: its nine taps into the sums of kConvMaps maps at one output place.
// wk: the channel's nine weights of the first of the maps, the next map's nine behind them
FLEET_TM void conv_taps(float (&acc)[kConvMaps], const float (&patch)[9], const float* wk) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
#pragma unroll
    for (int m = 0; m < kConvMaps; ++m) acc[m] = acc[m] + patch[i] * wk[m * 9 + i];
  }
}

// one convolution output with the x86 rule per operation (a sum that came out NaN).
// top: chans channels chan_stride apart, rows of row_len; w: at (map + k*maps)*9 + tap
FLEET_TM float conv_x86(const float* top, int row_len, int chan_stride, int chans, const float* w, int maps, int map,
                        int y, int x) {
  float a = 0.0f;
#pragma unroll 1
  for (int k = 0; k < chans; ++k) {
    const float* wm = w + (map + k * maps) * 9;
    const float* src = top + k * chan_stride;
    for (int i = 0; i < 9; ++i) a = MacX86{}(a, src[(y + i / 3) * row_len + x + i % 3], wm[i]);
  }
  return a;
}

// the kConvMaps outputs of map group mg at place (y, x) of a convolution layer, bias and elu
// applied, stored out_stride apart at out[m * out_stride]
FLEET_TM void conv_place(const float* top, int row_len, int chan_stride, int chans, const float* w, const float* bias,
                         int maps, int mg, int y, int x, float* out, int out_stride) {
  float acc[kConvMaps];
#pragma unroll
  for (int m = 0; m < kConvMaps; ++m) acc[m] = 0.0f;
#pragma unroll 1
  for (int k = 0; k < chans; ++k) {
    float patch[9];
    conv_patch(patch, top + k * chan_stride, row_len, y, x);
    conv_taps(acc, patch, w + (mg * kConvMaps + k * maps) * 9);
  }
#pragma unroll
  for (int m = 0; m < kConvMaps; ++m) {
    const int map = mg * kConvMaps + m;
    float a = acc[m];
    if (a != a) a = conv_x86(top, row_len, chan_stride, chans, w, maps, map, y, x);
    out[m * out_stride] = mojo_elu(a, bias[map]);
  }
}

// C1: item = mg*900 + place, the maps 4*mg .. 4*mg + 3 at that place. c1: [16][900], the
// reference's padding of four floats per map left out (see the head of this file)
FLEET_TM void c1_item(const float* image, const float* w1, const float* b1, int item, float* c1) {
  const int mg = item / kC1Map, pl = item % kC1Map;
  conv_place(image, kIn, kInMap, kChans, w1, b1, kMaps1, mg, pl / kC1, pl % kC1, c1 + mg * kConvMaps * kC1Map + pl,
             kC1Map);
}

// C2: item = mg*144 + place over P1's 16 channels. p1: [16][196]; c2: [64][144]
FLEET_TM void c2_item(const float* p1, const float* w2, const float* b2, int item, float* c2) {
  const int mg = item / kC2Map, pl = item % kC2Map;
  conv_place(p1, kP1, kP1Map, kMaps1, w2, b2, kMaps2, mg, pl / kC2, pl % kC2, c2 + mg * kConvMaps * kC2Map + pl,
             kC2Map);
}
constexpr int kC1Items = kC1Out / kConvMaps, kC2Items = kC2Out / kConvMaps;  // 3600, 2304

// max_pool's window of P x P at src (rows of row_len floats)
template <int P>
FLEET_TM float max_pool(const float* src, int row_len) {
  float mx = src[0];
#pragma unroll
  for (int i = 1; i < P * P; ++i) {
    const float n = src[(i / P) * row_len + i % P];
    if (mx < n) mx = n;
  }
  return mx;
}

// P1: output o = map*196 + row*14 + col, window 3 at stride 2 of c1 [16][900]
FLEET_TM float p1_out(const float* c1, int o) {
  const int map = o / kP1Map, py = (o / kP1) % kP1, px = o % kP1;
  return max_pool<3>(c1 + map * kC1Map + 2 * py * kC1 + 2 * px, kC1);
}

// P2: output o = map*9 + row*3 + col, window 4 at stride 4 of c2 [64][144]
FLEET_TM float p2_out(const float* c2, int o) {
  const int map = o / (kP2 * kP2), wy = (o / kP2) % kP2, wx = o % kP2;
  return max_pool<4>(c2 + map * kC2Map + 4 * wy * kC2 + 4 * wx, kC2);
}

// a fully_connected row's dot with the x86 rule per operation (a sum that came out NaN)
FLEET_TM float fc_x86(const float* top, const float* wrow, int n) {
  float a = 0.0f;
  for (int i = 0; i < n; ++i) a = MacX86{}(a, top[i], wrow[i]);
  return a;
}

// a fully_connected row: dot's loop from v = 0
FLEET_TM float fc_dot(const float* top, const float* wrow, int n) {
  float a = 0.0f;
  for (int i = 0; i < n; ++i) a = a + top[i] * wrow[i];
  return a == a ? a : fc_x86(top, wrow, n);
}

// node = 0.f + dot, then relu::f with the neuron's bias
FLEET_TM float fc_relu(float dot, float bias) {
  const float v = mojo_add(mojo_add(0.0f, dot), bias);
  return v < 0.0f ? 0.0f : v;
}

// softmax::f at temperature 1 in place on node[N] (activation.h:273-286), arg_max
// (network.h:146-153) and mse::cost against the label itself (cost.h:49-51): eval_forward.h's
// tail at a size given at run time, on memory instead of registers. probsN: N floats, or NULL
FLEET_TM evalnet::Verdict tail(float* node, int N, int32_t label, float* probsN) {
  const float temperature = 1.0f;
  float mx = node[0];
  for (int j = 1; j < N; ++j)
    if (node[j] > mx) mx = mojo_div(node[j], temperature);
  float denom = 0.0f;
  for (int j = 0; j < N; ++j) denom = mojo_add(denom, mojo_expf(mojo_sub(mojo_div(node[j], temperature), mx)));
  for (int j = 0; j < N; ++j) node[j] = mojo_div(mojo_expf(mojo_sub(mojo_div(node[j], temperature), mx)), denom);
  int max_j = 0;
  float best = node[0];
  for (int j = 0; j < N; ++j)
    if (best < node[j]) max_j = j, best = node[j];
  if (probsN)
    for (int j = 0; j < N; ++j) probsN[j] = node[j];
  const float d = mojo_sub(best, (float)label);
  return evalnet::Verdict{max_j, best, mojo_mul(mojo_mul(0.5f, d), d)};
}

#if !defined(__HIP_DEVICE_COMPILE__)
// every layer's node of one image, for the checks (any pointer may be NULL)
struct Layers {
  float *c1 = nullptr, *p1 = nullptr, *c2 = nullptr, *p2 = nullptr, *local4 = nullptr, *local5 = nullptr,
        *fc2 = nullptr;  // [16][900], [16][196], [64][144], [64][9], [384], [192], [N] (the probabilities)
};

// The kernel's stages in plain loops: one image. w: weight_count(classes) floats, b:
// bias_count(classes); image: 3072 floats, planar.
inline evalnet::Verdict cifar_forward_host(const float* w, const float* b, int classes, const float* image,
                                           int32_t label, float* probsN, const Layers* keep = nullptr) {
  static thread_local float c1[kC1Out], p1[kP1Out], c2[kC2Out];
  float p2[kFcIn], h4[kFc4], h5[kFc5], node[kMaxClasses];
  for (int it = 0; it < kC1Items; ++it) c1_item(image, w + kW1, b + kB1, it, c1);
  for (int o = 0; o < kP1Out; ++o) p1[o] = p1_out(c1, o);
  for (int it = 0; it < kC2Items; ++it) c2_item(p1, w + kW2, b + kB2, it, c2);
  for (int o = 0; o < kFcIn; ++o) p2[o] = p2_out(c2, o);
  for (int j = 0; j < kFc4; ++j) h4[j] = fc_relu(fc_dot(p2, w + kW4 + j * kFcIn, kFcIn), b[kB4 + j]);
  for (int j = 0; j < kFc5; ++j) h5[j] = fc_relu(fc_dot(h4, w + kW5 + j * kFc4, kFc4), b[kB5 + j]);
  for (int j = 0; j < classes; ++j) node[j] = mojo_add(0.0f, fc_dot(h5, w + kWfc + j * kFc5, kFc5));
  const evalnet::Verdict v = tail(node, classes, label, probsN);
  if (keep) {
    auto copy = [](float* dst, const float* src, int n) {
      for (int i = 0; dst && i < n; ++i) dst[i] = src[i];
    };
    copy(keep->c1, c1, kC1Out);
    copy(keep->p1, p1, kP1Out);
    copy(keep->c2, c2, kC2Out);
    copy(keep->p2, p2, kFcIn);
    copy(keep->local4, h4, kFc4);
    copy(keep->local5, h5, kFc5);
    copy(keep->fc2, node, classes);
  }
  return v;
}

// test()'s loop over images[idx[k]] and its last two lines do not depend on the network
inline void cifar_reduce_host(const float* cost, const int32_t* pred, const int32_t* labels, const int32_t* idx, int B,
                              float* error, float* accuracy, int32_t* correct) {
  evalnet::eval_reduce_host(cost, pred, labels, idx, B, error, accuracy, correct);
}
#endif

}  // namespace cifarnet
}  // namespace fleet
