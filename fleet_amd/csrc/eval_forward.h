// fleet_amd/csrc/eval_forward.h -- the Driver's test() (Driver/src/main/c++/
// cppNN_backend.cpp:53-75) per image and its closing arithmetic, host + device on
// teacher_math.h's FLEET_TM pattern: eval_kernels.hip runs these functions per lane,
// eval_forward_host / eval_reduce_host below run them in plain loops, and
// tests/native/check_eval_forward.cpp checks the latter against the reference's bits.
//
// Per image (commonLib/cppNN/network.h:510-515 predict_class):
//   out  = forward(x, 1.f, thread, 0) (network.h:523-592): teacher.hip's arithmetic,
//          documented at its head, at temperature 1 and with both semi-stochastic
//          pools at train == 0 (layer.h:540: the largest value always, the scan and
//          the denom == 0 branch as written);
//   argm = arg_max(out, 10) (network.h:146-153): the first index no later value
//          exceeds by `<`; a NaN never wins and never loses its place;
//   p    = out[argm], cost = ((0.5f * d) * d), d = p - (float)label (cost.h:49-51).
// After the loop: error = (0.f + cost_0 + cost_1 ...) / (float)B in image order,
// accuracy = ((float)correct / (float)B) * 100.f.
//
// The stages are cut where the kernel cuts them: C1 with P1 (one pooled value from
// its nine C1 outputs), C2i, C2 with P2 (the four C2 outputs of a window advance one
// input channel at a time, from the window's 6x6 patch and the map's 25 weights of
// the channel), FC2, and the softmax / arg_max / cost tail. A sum runs with plain
// operations and is repeated with the x86 NaN rule only when it comes out NaN, as
// mojo_sum does.
#pragma once
#include <stdint.h>

#include "teacher_math.h"

namespace fleet {
namespace evalnet {

constexpr int kIn = 28, kC1 = 24, kP1 = 8, kC2 = 4, kP2 = 2;
constexpr int kMaps1 = 8, kMaps2i = 16, kMaps2 = 48, kClasses = 10;
constexpr int kPix = kIn * kIn;                   // 784
constexpr int kP1Out = kMaps1 * kP1 * kP1;        // 512
constexpr int kC2iOut = kMaps2i * kP1 * kP1;      // 1024
constexpr int kFcIn = kP2 * kP2 * kMaps2;         // 192
constexpr int kC2Slice = kMaps2 * 25;             // C2's weights of one input channel
constexpr int kW1 = 0, kW2i = kW1 + kMaps1 * 25, kW2 = kW2i + kMaps2i * kMaps1, kWfc = kW2 + kMaps2 * kMaps2i * 25;
constexpr int kWTotal = kWfc + kClasses * kFcIn;  // 21448
constexpr int kB1 = 0, kB2i = kB1 + kMaps1, kB2 = kB2i + kMaps2i, kBfc = kB2 + kMaps2;
constexpr int kBTotal = kBfc + kClasses;          // 82

// one C1 output with the x86 rule per operation (a sum that came out NaN)
FLEET_TM float c1_x86(const float* in, const float* wm, int y, int x) {
  float a = 0.0f;
  for (int i = 0; i < 25; ++i) a = MacX86{}(a, in[(y + i / 5) * kIn + x + i % 5], wm[i]);
  return a;
}

// C1 + P1: pooled value o = map*64 + row*8 + col from the 7x7 input patch under its
// 3x3 window of C1 outputs. in: the image [28][28]; w1: C1's [8][25]; b1: C1's biases.
FLEET_TM float c1p1(const float* in, const float* w1, const float* b1, int o) {
  const int map = o / (kP1 * kP1), py = (o / kP1) % kP1, px = o % kP1;
  const float* wm = w1 + map * 25;
  float patch[49], wr[25], v[9];
#pragma unroll
  for (int i = 0; i < 49; ++i) patch[i] = in[(3 * py + i / 7) * kIn + 3 * px + i % 7];
#pragma unroll
  for (int i = 0; i < 25; ++i) wr[i] = wm[i];
  const float bias = b1[map];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < 25; ++i) a = a + patch[(q / 3 + i / 5) * 7 + q % 3 + i % 5] * wr[i];
    if (a != a) a = c1_x86(in, wm, 3 * py + q / 3, 3 * px + q % 3);
    v[q] = mojo_elu(a, bias);
  }
  return mojo_semi_pool<3>(v, false);
}

// C2i: output o = map*64 + p over P1's 8 channels. p1: [8][64]; w2i: at map + k*16.
FLEET_TM float c2i(const float* p1, const float* w2i, const float* b2i, int o) {
  const int map = o / (kP1 * kP1), p = o % (kP1 * kP1);
  const float acc = mojo_sum([&](auto mac) {
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < kMaps1; ++k) a = mac(a, p1[k * kP1 * kP1 + p], w2i[map + k * kMaps2i]);
    return a;
  });
  return mojo_elu(acc, b2i[map]);
}

// the 6x6 patch of one C2i channel (src: [8][8]) under P2 window (wy, wx)
FLEET_TM void c2_patch(float (&patch)[36], const float* src, int wy, int wx) {
#pragma unroll
  for (int i = 0; i < 36; ++i) patch[i] = src[(2 * wy + i / 6) * kP1 + 2 * wx + i % 6];
}

// C2, one input channel: its 25 taps into the four C2 outputs of a P2 window, q = 2*dy + dx,
// from the window's patch and one map's 25 weights of the channel
FLEET_TM void c2_taps(float (&acc)[4], const float (&patch)[36], const float (&wk)[25]) {
#pragma unroll
  for (int i = 0; i < 25; ++i) {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = acc[q] + patch[(q / 2 + i / 5) * 6 + q % 2 + i % 5] * wk[i];
  }
}

// one C2 output with the x86 rule per operation. c2i_all: [16][64]; w2: C2's weights
// at (k*48 + map)*25 + tap.
FLEET_TM float c2_x86(const float* c2i_all, const float* w2, int map, int y, int x) {
  float a = 0.0f;
  for (int k = 0; k < kMaps2i; ++k) {
    const float* wm = w2 + (k * kMaps2 + map) * 25;
    const float* src = c2i_all + k * kP1 * kP1;
    for (int i = 0; i < 25; ++i) a = MacX86{}(a, src[(y + i / 5) * kP1 + x + i % 5], wm[i]);
  }
  return a;
}

// C2's bias + elu on the four finished sums of a window, then P2
FLEET_TM float c2p2_finish(const float (&acc)[4], const float* c2i_all, const float* w2, float bias, int map, int wy,
                           int wx) {
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float a = acc[q];
    if (a != a) a = c2_x86(c2i_all, w2, map, 2 * wy + q / 2, 2 * wx + q % 2);
    v[q] = mojo_elu(a, bias);
  }
  return mojo_semi_pool<2>(v, false);
}

// FC2: node = 0 + dot(P2, W row)
FLEET_TM float fc(const float* p2, const float* wrow) {
  const float v = mojo_sum([&](auto mac) {
    float a = 0.0f;
    for (int i = 0; i < kFcIn; ++i) a = mac(a, p2[i], wrow[i]);
    return a;
  });
  return mojo_add(0.0f, v);
}

struct Verdict {
  int32_t pred;
  float p, cost;
};

// softmax::fc at temperature 1 (activation.h:271-313, as teacher.hip restates it),
// arg_max and mse::cost against the label itself. probs10: the ten probabilities, or NULL.
FLEET_TM Verdict tail(const float (&in)[kClasses], int32_t label, float* probs10) {
  const float temperature = 1.0f;
  float out[kClasses];
  float mx = in[0];
#pragma unroll
  for (int j = 1; j < kClasses; ++j)
    if (in[j] > mx) mx = mojo_div(in[j], temperature);
  float denom = 0.0f;
#pragma unroll
  for (int j = 0; j < kClasses; ++j) denom = mojo_add(denom, mojo_expf(mojo_sub(mojo_div(in[j], temperature), mx)));
#pragma unroll
  for (int j = 0; j < kClasses; ++j) out[j] = mojo_div(mojo_expf(mojo_sub(mojo_div(in[j], temperature), mx)), denom);
  int max_j = 0;
  float best = out[0];
#pragma unroll
  for (int j = 0; j < kClasses; ++j)
    if (best < out[j]) max_j = j, best = out[j];
  if (probs10) {
#pragma unroll
    for (int j = 0; j < kClasses; ++j) probs10[j] = out[j];
  }
  const float d = mojo_sub(best, (float)label);
  return Verdict{max_j, best, mojo_mul(mojo_mul(0.5f, d), d)};
}

// the ordered sum again with the x86 rule per addition (a sum that came out NaN)
FLEET_TM float sum_x86(const float* cost, int B) {
  float e = 0.0f;
  for (int k = 0; k < B; ++k) e = mojo_add(e, cost[k]);
  return e;
}

// test()'s last two lines from the ordered sum and the count
FLEET_TM void finish(float sum, int32_t correct, int B, float* error, float* accuracy) {
  *error = mojo_div(sum, (float)B);
  *accuracy = mojo_mul(mojo_div((float)correct, (float)B), 100.0f);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The kernel's stages in plain loops: one image.
inline Verdict eval_forward_host(const float* w, const float* b, const float* image, int32_t label, float* probs10) {
  float p1[kP1Out], c2[kC2iOut], p2[kFcIn], node[kClasses];
  for (int o = 0; o < kP1Out; ++o) p1[o] = c1p1(image, w + kW1, b + kB1, o);
  for (int o = 0; o < kC2iOut; ++o) c2[o] = c2i(p1, w + kW2i, b + kB2i, o);
  for (int t = 0; t < kFcIn; ++t) {
    const int map = t / 4, wy = (t % 4) / 2, wx = t % 2;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < kMaps2i; ++k) {
      float wk[25], patch[36];
      for (int i = 0; i < 25; ++i) wk[i] = w[kW2 + (k * kMaps2 + map) * 25 + i];
      c2_patch(patch, c2 + k * kP1 * kP1, wy, wx);
      c2_taps(acc, patch, wk);
    }
    p2[t] = c2p2_finish(acc, c2, w + kW2, b[kB2 + map], map, wy, wx);
  }
  for (int j = 0; j < kClasses; ++j) node[j] = fc(p2, w + kWfc + j * kFcIn);
  return tail(node, label, probs10);
}

// test()'s loop over images[idx[k]] (idx NULL: image k), then its last two lines
inline void eval_reduce_host(const float* cost, const int32_t* pred, const int32_t* labels, const int32_t* idx, int B,
                             float* error, float* accuracy, int32_t* correct) {
  float sum = 0.0f;
  int32_t c = 0;
  for (int k = 0; k < B; ++k) {
    sum = sum + cost[k];
    c += pred[k] == labels[idx ? idx[k] : k];
  }
  if (sum != sum) sum = sum_x86(cost, B);
  finish(sum, c, B, error, accuracy);
  *correct = c;
}
#endif

}  // namespace evalnet
}  // namespace fleet
