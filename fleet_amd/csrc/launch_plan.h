// fleet_amd/csrc/launch_plan.h -- the launch plan of the aggregation: which kernel form a
// bucket of a given size runs on, on what grid, and under what name it is reported. Plain
// C++ (no HIP header): kernels.hip asks with the device's CU count and only launches what
// the plan says; the plan's overrides (fleet_set_plan / FLEET_EXPERIMENTS) live here too.
#pragma once
#include <stdint.h>

#include <string>

namespace fleet {

// Launch-plan overrides: experiments, and the tests that run every launch variant on
// small inputs. Process-wide; set by fleet_set_plan (spec "key=value,..." -- update=
// auto|stream|tiled|pipe, grid=auto|plain|lanes|balanced, fused=on|off,
// stage_threads=N, stage_pieces=N, tile=auto|classic|flat|weave6|8, flat_w2=auto|N,
// tile_enc_prio=auto|0..3,
// tile_enc_rows=N) or, once at first
// use, from FLEET_EXPERIMENTS (the
// same spec). The default (empty spec) is the measured plan.
enum class UpdateForm { Auto, Stream, Tiled, Pipe };  // Tiled: 64-group tiles, Pipe: 16-group pipelined tiles
// stream grid: a group per lane everywhere (Plain), a value per lane everywhere (Lanes),
// whole rounds of group-per-lane waves and the rest a value per lane (Balanced)
enum class StreamGrid { Auto, Plain, Lanes, Balanced };
// tiles: Auto (flat alone, classic fused); a woven form's value is its waves per block
enum class TileForm { Auto = 0, Classic = 1, Flat = 2, Weave6 = 6, Weave8 = 8 };
struct PlanOverrides {
  UpdateForm update = UpdateForm::Auto;
  StreamGrid grid = StreamGrid::Auto;
  TileForm tile = TileForm::Auto;
  int flat_w2 = 0;        // flat tiles: width of the tiles after the whole 64-group rounds (0 auto)
  int tile_enc_prio = -1; // tiled / flat fused step: the encode blocks' issue priority (-1 auto)
  int tile_enc_rows = 0;  // fused steps (tiles and stream): rows per encode block (0 auto: 24)
  bool fused = true;      // false: the pipelined step as two launches (update, then encode)
  int stage_threads = 0;  // host staging copy threads (0 auto)
  int stage_pieces = 0;   // host staging H2D parts (0 auto)
};
// 0, or -1 with *err set; *norm: the spec normalised ("" = the measured default plan)
int parse_plan(const char* spec, PlanOverrides* o, std::string* norm, std::string* err);
PlanOverrides plan_overrides();
int set_plan_overrides(const char* spec, std::string* err);  // 0, or -1 (nothing changed)
std::string plan_spec();                                     // normalised active spec, "" = default

// The widest flat tile: E = 192 values, one per phase-2 thread. 85-group tiles (six
// whole clients per pass, a fourth phase-2 wave, 23.4 KB of LDS: 6 blocks per CU) were
// slower everywhere: cifar10_256 update 275.5 against 268.4 us, the N = 4 window 250.3
// against 230.6 (r05, profiles/r05/ab_flat_width85.txt).
constexpr int kFlatTG = 64;
constexpr int kFlatSlots = 7;   // blocks per CU (LDS 22.6 KB, 92 SGPRs; r05 residency traces)
constexpr int kWeaveTG = 64;    // groups of a woven tile
constexpr int kPipeNW = 5;      // waves per block of the pipelined tiles: 4 producers + one consumer
// waves per block of the Kardam pipelined form (one consumer, the rest producers): the
// side outputs double the producers' work, and 8 producer waves keep the consumer fed
// where 4 do not (mnist64 under rocprof, r06 call a10: 27.3 us with 4 producer waves,
// 24.4 with 8, 28.3 with 10, 43.2 with 12; the plain update 16.1 us)
#ifndef FLEET_KD_NW
#define FLEET_KD_NW 9
#endif
constexpr int kKdPipeNW = FLEET_KD_NW;

// The grid of k_update_flat: blocks [0, nW) are tiles of w1 groups, [nW, nU) tiles of
// w2 groups (the last one ragged), each run in XCD-aware order (xcd_tile).
struct FlatGrid {  // a kernel argument
  int nW, nU, w1, w2;
};

// The aggregation's launch plan for a bucket (or window) of `groups` 3-value groups.
//   stream -- k_update_mixed<256> (fused: k_update_encode<256>): a lane walks its group
//             down all M rows, whole rounds group-per-lane and the rest a value per lane;
//   tiled  -- the one-width 64-group tiles of k_update_tiled_encode<64> (the fused step);
//   flat   -- k_update_flat: two-phase tiles of a runtime width, one balanced round;
//   woven  -- k_update_weave<8> / k_update_weave_encode<8 | 6>: both phases in one barrier
//             interval (small windows, latency-bound);
//   pipe   -- k_update_pipe<16, 1, 5, 0>: 16-group tiles, 4 producer waves + one consumer
//             wave (MNIST-size buckets: the serial chain is the critical path).
// Default ranges (DESIGN.md §4, 256 CUs): the update alone -- stream from 131,072 groups,
// flat above 49,152 (three 64-group tiles per CU), woven 8-wave from 24 k, pipe below;
// the fused step -- stream from 131,072, tiled from 65,536, flat from 40 k, woven 6-wave
// from 32 k, woven 8-wave from 14 k, pipe below; Kardam's side outputs -- stream from
// 131,072, flat from 32 k, pipe below.
enum class UpdateKind { Stream = 0, Tiled = 1, Pipe = 2, Weave = 3, Flat = 4 };  // fleet_update_plan_grid's `kind`
// what the planned launch carries besides the update
// Update alone; UpdateEncode: the fused step, the client encode's blocks after the update's;
// UpdateThenEncode (fused=off): the update alone, then the standalone k_encode_f32;
// UpdateKardam: the update with Kardam's side outputs
enum class PlanStep { Update, UpdateEncode, UpdateThenEncode, UpdateKardam };
// the reduce of Kardam's per-wave partials: blocks of the update's own launch (the
// pipelined form), or k_kardam_reduce<NT, U> after it (one wave per client up to 2,048
// partials, four beyond)
enum class KardamReduce { InLaunch, Wave8, Wave32, Block32 };
struct LaunchPlan {
  PlanStep step;
  UpdateKind kind;
  int64_t blocks;  // the update's own blocks (stream: nU, value-per-lane blocks included)
  int64_t grid;    // blocks of the launch: `blocks`, then the encode's or the in-launch reduce's
  int threads;     // per block
  int nA;          // stream: blocks of group-per-lane waves (the rest a value per lane)
  int nw;          // woven tiles: waves per block (6 or 8)
  FlatGrid fg;     // flat tiles
  // UpdateEncode: k_encode_f32's grid flattened x-fastest behind the update's blocks
  int64_t enc_gx;  // blocks along a row (of `threads` lanes, a group each)
  int enc_rpb;     // rows per block
  int enc_prio;    // issue priority of the encode's waves
  // UpdateKardam
  int n_waves;     // partial slots per client: a wave of the stream grid or a tile
  int flag_slots;  // the pipelined form's tile flags (per producer wave)
  int norm_parts;  // pairs of sums per client
  KardamReduce reduce;
};
// Pure: `cus` is the device's CU count, nothing else is read.
LaunchPlan plan_update(int64_t groups, const PlanOverrides& o, int cus);
LaunchPlan plan_update_encode(int64_t groups, int M, const PlanOverrides& o, int cus);
LaunchPlan plan_update_kardam(int64_t groups, int M, const PlanOverrides& o, int cus);
// The kernel a plan launches, as profiles and bench.py key on it.
std::string kernel_name(const LaunchPlan& p);

// rows per block of the standalone client encode (k_encode_f32; the fused pipelined form keeps its rule)
int encode_rows_per_block(int64_t gx, int rows);

}  // namespace fleet
