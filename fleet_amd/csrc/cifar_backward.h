// fleet_amd/csrc/cifar_backward.h -- the client's gradient computation on the reference's CIFAR
// network (cifar_forward.h names its layers): what cnn.gradients() returns after B train_class
// calls (commonLib/cppNN/network.h:1806-2008 train_class, :1551-1611 backward_hidden, :1289-1331
// sync_mini_batch, :1038-1056 gradients()), host + device on client_backward.h's pattern:
// cifar_client_kernels.hip runs sample_stages() with one block per sample, sum_element() with a
// lane per element and fc_step() in the tiles of its ordered rank-B sum; rgb_grads_host() below
// runs the same functions in plain loops, and tests/native/check_cifar_backward.cpp drives it.
// What is claimed: the device equals this mirror in bits, and the mirror follows the lines cited
// here. No fixture recorded from the reference's own network class exists for this path yet.
//
// The single-thread order with the cross_entropy cost, as client_backward.h states it for MNIST.
// The reference is built -O0 without MOJO_AVX or NEON: one binary32 rounding per operation, no
// contraction, every sum in the order written there.
//
// Per sample:
//   shift    m.shift(dx, dy, mojo::edge) on each of the three planes (network.h:1840,
//            core_math.h:721-731): out[y][x] = in[clamp(y - dy)][clamp(x - dx)]
//   forward  cifar_forward.h's arithmetic; both max_pools keep the index they picked
//            (layer.h:363-456: _max_map); the head is softmax::f at the call's temperature
//   delta    FC2: 1.f * (node[j] - target[j]), target one-hot, all zeros for a label outside
//            [0, N) (network.h:1896-1903, 1949); E = the mean of mse::cost, NaN is `bail`
//   pass 1   (network.h:1561-1578) from FC2 down: delta[i] *= df(node, i) below the last layer,
//            then distribute_delta into the layer above. relu::df is node > 0 ? 1.f : 0.f and
//            elu::df node > 0 ? 1.f : 0.1f*expf(node), both on the ACTIVATED node
//            (activation.h:180, 214); the pools and the input have df = 1.f, not written out.
//            FC2 -> local5 -> local4 -> P2 (layer.h:244-255, the first arm): per t one running
//                       sum from 0, b in order: += delta[b] * w[t + b*cols]
//            P2 -> C2   (layer.h:461-466) top.delta[p_map[k]] += delta[k]: the windows do not
//                       overlap, an element receives 0.f + delta[k] or stays 0.f
//            P1 -> C1   the same line, but the windows (3 wide, stride 2) overlap: up to four
//                       pool outputs point at one C1 element, and they are added in k order.
//                       Here every C1 element gathers its (at most four) windows in ascending k
//            C2 -> P1, C1 -> I1 (layer.h:1025-1049, kernel_cols == 3): the delta padded by 2 with
//                       zeros, unwrap_aligned_NxN(3) and dotsum_unwrapped_NxN(3) (core_math.h:
//                       112-185) into a copy of the top delta: per element one running sum from
//                       its current value (0), the map the outer loop, tap i = row*3 + col inner,
//                       += pad[map][y + row][x + col] * w[(k*maps + map)*9 + 8 - i].
//                       The padded copy does not exist here: a tap outside the map multiplies
//                       0.f, so the sum takes the same steps. dotsum walks 8 outputs at a time
//                       and so runs past P1's 196 into the padding of its aligned copy
//                       (layer.h:939); only the 196 values are copied back (:1046).
//   pass 2   (network.h:1587-1603) calculate_dw per edge, dbias = the layer's delta for every
//            layer that is no convolution (I1 3072, P1 3136, P2 576, local4 384, local5 192, FC2 N)
//            local4, local5, FC2 (layer.h:276-302): dw[t + b*cols] = top[t] * delta[b], a bare
//                       product (-0 stays)
//            C2, C1 (layer.h:1195-1215): dw.fill(0), then += unwrap_2d_dot(top + tap, delta, n,
//                       top_n, n) (core_math.h:58-81): v = 0; per row j: v += dot(row), dot the
//                       default arm from 0 (rows of 12 and 30). Every element is 0.f + v.
// Across samples (network.h:1289-1331, 1038-1056): dW_sets[0] += dW_sets[b], b = 1 .. B-1 in
// order per element in binary32, the same for dbias_sets, laid out as fleet_amd/layouts.py
// CIFAR10 / CIFAR100: 313,867 or 331,237 values.
//
// The reference keeps C1's node and delta channel-aligned, maps 904 floats apart (layer.h:771);
// here they are 900 apart (cifar_forward.h), p_map indexes that layout, and the padding does
// not exist. Nothing reads it: P1's windows end at row 28, the taps are bounded by the map.
//
// 96 % of the vector is the three fully connected dW blocks: outer products of two short
// vectors. A sample therefore leaves no gradient row but a RECORD of 18,160 + N floats: C1's and
// C2's dW, the six dbias blocks (the fully connected layers' deltas among them) and the three
// fully connected inputs. sum_element() adds the records' first part in sample order, fc_step()
// the outer products.
//
// DPgradients(C, sigma): further down, beside the functions it uses (FLEET_RGB_CLIP_ORDER,
// record_sqsum, dp_sum_element; rgb_dp_host is the plain form, tests/native/check_cifar_dp.cpp
// drives it).
//
// NaN: client_backward.h's rule. A NaN forward makes E NaN: sample_stages reports it and the
// client's row is unspecified. With a NaN met only in the backward pass, nothing is pinned.
#pragma once
#include <stdint.h>

#include "cifar_forward.h"
#include "client_backward.h"  // clip_scale and noisy: DPgradients' two formulas, network-independent

namespace fleet {
namespace rgbnet {

using namespace cifarnet;

// gradients(): [7, 432, C1, 0, 9216, C2, 0, 221184, local4, 73728, local5, 192N, FC2,
//               8, 3072, I1, 0, 3136, P1, 0, 576, P2, 384, local4, 192, local5, N, FC2]
constexpr int kG_W1 = 2, kG_W2 = kG_W1 + 432 + 2, kG_W4 = kG_W2 + 9216 + 2, kG_W5 = kG_W4 + kFc4 * kFcIn + 1;
constexpr int kG_Wfc = kG_W5 + kFc5 * kFc4 + 1;  // 304568
FLEET_TM int g_nB(int N) { return kG_Wfc + kFc5 * N; }
FLEET_TM int g_BI1(int N) { return g_nB(N) + 2; }
FLEET_TM int g_BP1(int N) { return g_BI1(N) + kPix + 2; }
FLEET_TM int g_BP2(int N) { return g_BP1(N) + kP1Out + 2; }
FLEET_TM int g_B4(int N) { return g_BP2(N) + kFcIn + 1; }
FLEET_TM int g_B5(int N) { return g_B4(N) + kFc4 + 1; }
FLEET_TM int g_Bfc(int N) { return g_B5(N) + kFc5 + 1; }
FLEET_TM int grad_len(int N) { return classes_ok(N) ? g_Bfc(N) + N : 0; }  // 313867, 331237

// a sample's record: [dW C1 | dW C2 | dbias I1 | P1 | P2 | local4 | local5 | FC2 (N) | the nodes
// of P2 | local4 | local5]; the summed part is everything before the nodes
constexpr int kR_W1 = 0, kR_W2 = 432, kR_BI1 = kR_W2 + 9216, kR_BP1 = kR_BI1 + kPix, kR_BP2 = kR_BP1 + kP1Out;
constexpr int kR_B4 = kR_BP2 + kFcIn, kR_B5 = kR_B4 + kFc4, kR_Bfc = kR_B5 + kFc5;  // 17008
FLEET_TM int r_X4(int N) { return kR_Bfc + N; }
FLEET_TM int r_X5(int N) { return r_X4(N) + kFcIn; }
FLEET_TM int r_Xfc(int N) { return r_X5(N) + kFc4; }
FLEET_TM int record_len(int N) { return r_Xfc(N) + kFc5; }  // 18160 + N
FLEET_TM int summed_len(int N) { return kR_Bfc + N; }

constexpr int kHeaders = 17;
struct Header {
  int pos;
  float value;
};
FLEET_TM Header header(int i, int N) {  // (a switch, not a table: a table indexed at run time lives in scratch)
  switch (i) {
    case 0: return {0, 7.f};
    case 1: return {1, 432.f};
    case 2: return {kG_W2 - 2, 0.f};
    case 3: return {kG_W2 - 1, 9216.f};
    case 4: return {kG_W4 - 2, 0.f};
    case 5: return {kG_W4 - 1, (float)(kFc4 * kFcIn)};
    case 6: return {kG_W5 - 1, (float)(kFc5 * kFc4)};
    case 7: return {kG_Wfc - 1, (float)(kFc5 * N)};
    case 8: return {g_nB(N), 8.f};
    case 9: return {g_BI1(N) - 1, (float)kPix};
    case 10: return {g_BP1(N) - 2, 0.f};
    case 11: return {g_BP1(N) - 1, (float)kP1Out};
    case 12: return {g_BP2(N) - 2, 0.f};
    case 13: return {g_BP2(N) - 1, (float)kFcIn};
    case 14: return {g_B4(N) - 1, (float)kFc4};
    case 15: return {g_B5(N) - 1, (float)kFc5};
    default: return {g_Bfc(N) - 1, (float)N};
  }
}

// position in gradients() of element q of a record's summed part
FLEET_TM int summed_pos(int q, int N) {
  if (q < kR_W2) return kG_W1 + q;
  if (q < kR_BI1) return kG_W2 + q - kR_W2;
  if (q < kR_BP1) return g_BI1(N) + q - kR_BI1;
  if (q < kR_BP2) return g_BP1(N) + q - kR_BP1;
  if (q < kR_B4) return g_BP2(N) + q - kR_BP2;
  if (q < kR_B5) return g_B4(N) + q - kR_B4;
  if (q < kR_Bfc) return g_B5(N) + q - kR_B5;
  return g_Bfc(N) + q - kR_Bfc;
}

// sync_mini_batch for element q of the summed part: the records added in sample order
FLEET_TM float sum_element(const float* recs, int64_t pitch, int B, int q) {
  float a = recs[q];
  for (int k = 1; k < B; ++k) a = a + recs[(int64_t)k * pitch + q];
  return a;
}

// a fully connected edge's dW block: rows x cols values at `pos` of gradients(), element
// (b, t) the sum over the samples of node[t] * delta[b], node and delta in the records
struct FcBlock {
  int rows, cols, node, delta, pos;
};
constexpr int kFcBlocks = 3;
FLEET_TM FcBlock fc_block(int i, int N) {
  if (i == 0) return {kFc4, kFcIn, r_X4(N), kR_B4, kG_W4};
  if (i == 1) return {kFc5, kFc4, r_X5(N), kR_B5, kG_W5};
  return {N, kFc5, r_Xfc(N), kR_Bfc, kG_Wfc};
}

// one sample's step of that sum: calculate_dw's bare product for sample 0 (-0 stays), then
// sync_mini_batch's += of the next sample's rounded product
FLEET_TM float fc_step(float acc, bool first, float node, float delta) {
  const float p = node * delta;
  return first ? p : acc + p;
}

// ---- DPgradients(C, sigma) on this network (network.h:1092-1181, as client_backward.h states it
// for MNIST; clientnet::clip_scale and clientnet::noisy are used as they are).
//
// scale_gradients' walk for a batch slot b >= 1: the layers of cppNN_backend.cpp:128-138 (I1, C1,
// P1, C2, P2, local4, local5, FC2) last to first, per layer the backward link's dW block element
// by element, then the layer's dbias block; the convolutions' dbias and the pools' dW blocks have
// size 0. In terms of a sample's record: `fc` >= 0 is fully connected dW block fc_block(fc), which
// no record holds: its element (b, t) is the bare product node[t] * delta[b], row b outer, t
// inner; otherwise `len` values at `rec` of the record. 313,850 + 193 (N - 10) squares.
struct ClipSegment {
  int fc, rec, len;
};
constexpr int kClipSegments = 11;
#define FLEET_RGB_CLIP_ORDER(N)                                                                               \
  {{2, 0, 0}, {-1, kR_Bfc, N}, {1, 0, 0}, {-1, kR_B5, kFc5}, {0, 0, 0}, {-1, kR_B4, kFc4}, {-1, kR_BP2, kFcIn}, \
   {-1, kR_W2, kR_BI1 - kR_W2}, {-1, kR_BP1, kP1Out}, {-1, kR_W1, kR_W2 - kR_W1}, {-1, kR_BI1, kPix}}
FLEET_TM ClipSegment clip_segment(int i, int N) {  // (selects, not an indexed read: see header())
  const ClipSegment seg[kClipSegments] = FLEET_RGB_CLIP_ORDER(N);
  ClipSegment s = seg[0];
#pragma unroll
  for (int j = 1; j < kClipSegments; ++j)
    if (i == j) s = seg[j];
  return s;
}

// sqsum += x*x: the rounded square, then the rounded add
FLEET_TM float clip_add(float sqsum, float x) { return sqsum + x * x; }

// one sample's sqsum from its record, in the walk's order (the plain form of k_rgb_clip's chain)
FLEET_TM float record_sqsum(const float* rec, int N) {
  float sqsum = 0.0f;
  for (int i = 0; i < kClipSegments; ++i) {
    const ClipSegment s = clip_segment(i, N);
    if (s.fc < 0) {
      for (int j = 0; j < s.len; ++j) sqsum = clip_add(sqsum, rec[s.rec + j]);
      continue;
    }
    const FcBlock f = fc_block(s.fc, N);
    for (int b = 0; b < f.rows; ++b)
      for (int t = 0; t < f.cols; ++t) sqsum = clip_add(sqsum, rec[f.node + t] * rec[f.delta + b]);
  }
  return sqsum;
}

// sum_element under DPgradients, before the noise: the second loop of scale_gradients scales
// the dbias blocks of slots >= 1 and no dW (client_backward.h has why), so the convolutions' dW
// elements are added as they are
FLEET_TM float dp_sum_element(const float* recs, int64_t pitch, int B, int q, const float* scale) {
  if (q < kR_BI1) return sum_element(recs, pitch, B, q);
  float a = recs[q];
  for (int k = 1; k < B; ++k) a = a + recs[(int64_t)k * pitch + q] * scale[k];
  return a;
}

constexpr int kFcCols = 8;  // columns of a fully connected layer staged at a time in the forward

// One sample's layers. C1's and C2's nodes become their own deltas in place once df is applied;
// the padded deltas, I1's delta and C2's weights are never stored (158 KB: the block's LDS in
// cifar_client_kernels.hip, whose head has the budget).
struct Sample {
  float img[kPix];     // the shifted sample: C1's input, and C1's dW reads it again
  float w1[kW2 - kW1];
  float c1[kC1Out];    // [16][900] node, then delta
  float c2[kC2Out];    // [64][144] node, then delta
  float p1[kP1Out];    // node: lives until C2's dW
  float d_p1[kP1Out];  // in the forward: the fully connected layers' weight tile
  float p2[kFcIn], d_p2[kFcIn], h4[kFc4], d4[kFc4], h5[kFc5], d5[kFc5], fc[kMaxClasses], d_fc[kMaxClasses];
  int32_t pm1[kP1Out], pm2[kFcIn];  // the pools' picks: indices into c1 and c2
  float E;
};
static_assert(kFcCols * (kFc4 + 1) <= kP1Out, "the weight tile lies where P1's delta will be");

// max_pool's window of P x P at src (layer.h:363-456): the offset of the maximum, the first on ties
template <int P>
FLEET_TM int pool_pick(const float* src, int row_len) {
  float mx = src[0];
  int at = 0;
#pragma unroll
  for (int i = 1; i < P * P; ++i) {
    const int off = (i / P) * row_len + i % P;
    const float n = src[off];
    if (mx < n) mx = n, at = off;
  }
  return at;
}

FLEET_TM float relu_df(float node) { return node > 0.0f ? 1.0f : 0.0f; }
FLEET_TM float elu_df(float node) { return node > 0.0f ? 1.0f : 0.1f * mojo_expf(node); }

// the output delta and E (network.h:1896-1903, 1945-1982); mse::cost is (0.5f*d)*d (cost.h:49-51)
FLEET_TM float out_delta(const float* node, int N, int32_t label, float* delta) {
  float E = 0.0f;
  for (int j = 0; j < N; ++j) {
    const float target = (label >= 0 && label < N && j == label) ? 1.0f : 0.0f;
    const float d = node[j] - target;
    delta[j] = 1.0f * d;
    E += (0.5f * d) * d;
  }
  return E / (float)N;
}

// fully_connected distribute_delta, element t of the layer above: w rows of `cols` floats
FLEET_TM float fc_back(const float* delta, int n, const float* w, int cols, int t) {
  float a = 0.0f;
  for (int b = 0; b < n; ++b) a = a + delta[b] * w[t + (int64_t)b * cols];
  return a;
}

// 3x3 distribute_delta: element (k, y, x) of the layer above from this layer's delta
// [maps][n][n] (maps `stride` apart) and the edge's weights; a tap outside the map reads the
// padding's 0.f
FLEET_TM float conv3_back(const float* delta, int n, int stride, const float* w, int maps, int k, int y, int x) {
  float a = 0.0f;
#pragma unroll 1
  for (int map = 0; map < maps; ++map) {
    const float* d = delta + map * stride;
    const float* wm = w + (k * maps + map) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int py = y + i / 3 - 2, px = x + i % 3 - 2;
      const float v = (py >= 0 && py < n && px >= 0 && px < n) ? d[py * n + px] : 0.0f;
      a = a + v * wm[8 - i];
    }
  }
  return a;
}

// unwrap_2d_dot with dot's loop form: v = 0, per row v += (d = 0; d += x1[i]*x2[i])
FLEET_TM float dot2d(const float* x1, const float* x2, int size, int stride1, int stride2) {
  float v = 0.0f;
  for (int j = 0; j < size; ++j) {
    float d = 0.0f;
    for (int i = 0; i < size; ++i) d = d + x1[stride1 * j + i] * x2[stride2 * j + i];
    v = v + d;
  }
  return v;
}

// P1 -> C1 for C1 element o = map*900 + y*30 + x: the windows that cover it in ascending k
// (rows first), each adding its delta where its pick is o
FLEET_TM float p1_gather(const float* d_p1, const int32_t* pm1, int o) {
  const int map = o / kC1Map, y = (o / kC1) % kC1, x = o % kC1;
  const int py0 = y < 2 ? 0 : (y - 1) / 2, py1 = y / 2 < kP1 - 1 ? y / 2 : kP1 - 1;
  const int px0 = x < 2 ? 0 : (x - 1) / 2, px1 = x / 2 < kP1 - 1 ? x / 2 : kP1 - 1;
  float a = 0.0f;
  for (int py = py0; py <= py1; ++py)
    for (int px = px0; px <= px1; ++px) {
      const int k = map * kP1Map + py * kP1 + px;
      if (pm1[k] == o) a = a + d_p1[k];
    }
  return a;
}

// a fully connected layer of the forward, `rows` neurons over x[cols], on cifar_forward.h's
// fc_dot / fc_relu: kFcCols columns of every row at a time go through `tile` transposed
// (pitch rows + 1), so that neighbouring lanes read neighbouring rows without striding memory;
// out[j] carries neuron j's running sum from tile to tile, every step in fc_dot's order
template <class Par>
FLEET_TM void fc_forward(Par par, float* tile, const float* w, const float* bias, int rows, int cols, const float* x,
                         float* out) {
  par(rows, [&](int j) { out[j] = 0.0f; });
  for (int c0 = 0; c0 < cols; c0 += kFcCols) {
    par(rows * kFcCols, [&](int e) {
      const int row = e / kFcCols, col = e % kFcCols;
      tile[col * (rows + 1) + row] = w[(int64_t)row * cols + c0 + col];
    });
    par(rows, [&](int j) {
      float a = out[j];
#pragma unroll
      for (int i = 0; i < kFcCols; ++i) a = a + x[c0 + i] * tile[i * (rows + 1) + j];
      out[j] = a;
    });
  }
  par(rows, [&](int j) {
    float a = out[j];
    if (a != a) a = fc_x86(x, w + (int64_t)j * cols, cols);
    out[j] = fc_relu(a, bias[j]);
  });
}

// One sample, every stage in the reference's order. `par(n, f)` runs f(o) for o in [0, n) and
// returns once all of them are done (the block's lanes and a barrier in the kernel, a loop on
// the host). w, b: the model (cifar_forward.h's offsets), image: the unshifted sample [3072],
// rec: the sample's record [record_len(N)]. Returns false where E is NaN (the reference's bail).
template <class Par>
FLEET_TM bool sample_stages(Par par, Sample& S, int N, const float* w, const float* b, const float* image, int32_t label,
                            int dx, int dy, float temperature, float* rec) {
  static_assert(kFcIn % kFcCols == 0 && kFc4 % kFcCols == 0, "whole tiles");
  // shift, per plane
  par(kPix, [&](int o) {
    int y = (o / kIn) % kIn - dy, x = o % kIn - dx;
    y = y < 0 ? 0 : (y > kIn - 1 ? kIn - 1 : y);
    x = x < 0 ? 0 : (x > kIn - 1 ? kIn - 1 : x);
    S.img[o] = image[(o / kInMap) * kInMap + y * kIn + x];
    if (o < kW2 - kW1) S.w1[o] = w[kW1 + o];
  });
  // forward, train mode: the pools keep their picks
  par(kC1Items, [&](int it) { c1_item(S.img, S.w1, b + kB1, it, S.c1); });
  par(kP1Out, [&](int o) {
    const int base = (o / kP1Map) * kC1Map + 2 * ((o / kP1) % kP1) * kC1 + 2 * (o % kP1);
    S.pm1[o] = base + pool_pick<3>(S.c1 + base, kC1);
    S.p1[o] = S.c1[S.pm1[o]];
  });
  par(kC2Items, [&](int it) { c2_item(S.p1, w + kW2, b + kB2, it, S.c2); });
  par(kFcIn, [&](int o) {
    const int base = (o / (kP2 * kP2)) * kC2Map + 4 * ((o / kP2) % kP2) * kC2 + 4 * (o % kP2);
    S.pm2[o] = base + pool_pick<4>(S.c2 + base, kC2);
    S.p2[o] = S.c2[S.pm2[o]];
  });
  fc_forward(par, S.d_p1, w + kW4, b + kB4, kFc4, kFcIn, S.p2, S.h4);
  fc_forward(par, S.d_p1, w + kW5, b + kB5, kFc5, kFc4, S.h4, S.h5);
  par(N, [&](int j) { S.fc[j] = mojo_add(0.0f, fc_dot(S.h5, w + kWfc + j * kFc5, kFc5)); });
  par(1, [&](int) {
    softmax_at(S.fc, N, temperature);
    S.E = out_delta(S.fc, N, label, S.d_fc);
  });
  // pass 1
  par(kFc5, [&](int t) { S.d5[t] = fc_back(S.d_fc, N, w + kWfc, kFc5, t) * relu_df(S.h5[t]); });
  par(kFc4, [&](int t) { S.d4[t] = fc_back(S.d5, kFc5, w + kW5, kFc4, t) * relu_df(S.h4[t]); });
  par(kFcIn, [&](int t) { S.d_p2[t] = fc_back(S.d4, kFc4, w + kW4, kFcIn, t); });
  // P2 -> C2 and C2's df: the node becomes the delta
  par(kC2Out, [&](int o) {
    const int win = (o / kC2Map) * kP2 * kP2 + (((o / kC2) % kC2) / 4) * kP2 + (o % kC2) / 4;
    const float d = S.pm2[win] == o ? 0.0f + S.d_p2[win] : 0.0f;
    S.c2[o] = d * elu_df(S.c2[o]);
  });
  par(kP1Out, [&](int o) {
    S.d_p1[o] = conv3_back(S.c2, kC2, kC2Map, w + kW2, kMaps2, o / kP1Map, (o / kP1) % kP1, o % kP1);
  });
  // P1 -> C1 and C1's df, in place (a lane reads and writes its own element only)
  par(kC1Out, [&](int o) { S.c1[o] = p1_gather(S.d_p1, S.pm1, o) * elu_df(S.c1[o]); });
  // C1 -> I1: the input's delta is its dbias block and nothing else
  par(kPix, [&](int o) {
    rec[kR_BI1 + o] = conv3_back(S.c1, kC1, kC1Map, S.w1, kMaps1, o / kInMap, (o / kIn) % kIn, o % kIn);
  });
  // pass 2: the convolutions' dW; element o = (map + k*maps)*9 + tap, as the weights lie
  par(kMaps2 * kMaps1 * 9, [&](int o) {
    const int tap = o % 9, map = (o / 9) % kMaps2, k = o / (9 * kMaps2);
    rec[kR_W2 + o] = 0.0f + dot2d(S.p1 + k * kP1Map + (tap / 3) * kP1 + tap % 3, S.c2 + map * kC2Map, kC2, kP1, kC2);
  });
  par(kMaps1 * kChans * 9, [&](int o) {
    const int tap = o % 9, map = (o / 9) % kMaps1, k = o / (9 * kMaps1);
    rec[kR_W1 + o] = 0.0f + dot2d(S.img + k * kInMap + (tap / 3) * kIn + tap % 3, S.c1 + map * kC1Map, kC1, kIn, kC1);
  });
  // the dbias blocks and the fully connected layers' inputs
  par(kP1Out, [&](int o) {
    rec[kR_BP1 + o] = S.d_p1[o];
    if (o < kFcIn) rec[kR_BP2 + o] = S.d_p2[o], rec[r_X4(N) + o] = S.p2[o];
    if (o < kFc4) rec[kR_B4 + o] = S.d4[o], rec[r_X5(N) + o] = S.h4[o];
    if (o < kFc5) rec[kR_B5 + o] = S.d5[o], rec[r_Xfc(N) + o] = S.h5[o];
    if (o < N) rec[kR_Bfc + o] = S.d_fc[o];
  });
  return S.E == S.E;
}

#if !defined(__HIP_DEVICE_COMPILE__)
struct HostPar {
  template <class F>
  void operator()(int n, F f) const {
    for (int o = 0; o < n; ++o) f(o);
  }
};

// One client's call in plain loops: images [B][3072] (already gathered), labels [B], shifts
// [B][2] = (dx, dy) or NULL, out [grad_len(N)]. recs: scratch [B][record_len(N)]. Returns the
// number of samples whose E is NaN.
inline int rgb_grads_host(int N, const float* w, const float* b, const float* images, const int32_t* labels,
                          const int32_t* shifts, int B, float temperature, float* recs, float* out) {
  Sample* S = new Sample;
  const int64_t pitch = record_len(N);
  int blown = 0;
  for (int k = 0; k < B; ++k)
    blown += !sample_stages(HostPar{}, *S, N, w, b, images + (int64_t)k * kPix, labels[k], shifts ? shifts[2 * k] : 0,
                            shifts ? shifts[2 * k + 1] : 0, temperature, recs + k * pitch);
  delete S;
  for (int i = 0; i < kHeaders; ++i) out[header(i, N).pos] = header(i, N).value;
  for (int q = 0; q < summed_len(N); ++q) out[summed_pos(q, N)] = sum_element(recs, pitch, B, q);
  for (int i = 0; i < kFcBlocks; ++i) {
    const FcBlock f = fc_block(i, N);
    for (int r = 0; r < f.rows; ++r)
      for (int t = 0; t < f.cols; ++t) {
        float a = 0.0f;
        for (int k = 0; k < B; ++k) a = fc_step(a, k == 0, recs[k * pitch + f.node + t], recs[k * pitch + f.delta + r]);
        out[f.pos + r * f.cols + t] = a;
      }
  }
  return blown;
}

// DPgradients(clip, sigma), sigma > 0, from the records rgb_grads_host left: z [grad_len(N)] the
// draws (clientnet::dp_noise_draws), out [grad_len(N)] is overwritten, scale: scratch [B]
inline void rgb_dp_host(int N, const float* recs, int B, float clip, float sigma, const double* z, float* scale,
                        float* out) {
  const int64_t pitch = record_len(N);
  const double s = (double)(clip * sigma);
  for (int k = 0; k < B; ++k) scale[k] = k ? clientnet::clip_scale(record_sqsum(recs + k * pitch, N), clip) : 1.0f;
  for (int q = 0; q < summed_len(N); ++q) {
    const int pos = summed_pos(q, N);
    out[pos] = clientnet::noisy(dp_sum_element(recs, pitch, B, q, scale), z[pos], s);
  }
  for (int i = 0; i < kFcBlocks; ++i) {
    const FcBlock f = fc_block(i, N);
    for (int r = 0; r < f.rows; ++r)
      for (int t = 0; t < f.cols; ++t) {
        float a = 0.0f;
        for (int k = 0; k < B; ++k) a = fc_step(a, k == 0, recs[k * pitch + f.node + t], recs[k * pitch + f.delta + r]);
        out[f.pos + r * f.cols + t] = clientnet::noisy(a, z[f.pos + r * f.cols + t], s);
      }
  }
  for (int i = 0; i < kHeaders; ++i) out[header(i, N).pos] = header(i, N).value;
}
#endif

}  // namespace rgbnet
}  // namespace fleet
