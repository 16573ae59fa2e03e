// fleet_amd/csrc/launch_plan.cpp -- the launch plan (launch_plan.h): the overrides' store
// and parser, the three planners and the kernel names. Host code only.
#include "launch_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>

namespace fleet {

// Launch-plan overrides (launch_plan.h): process-wide, set by fleet_set_plan or, once at
// first use, from FLEET_EXPERIMENTS (the same spec) -- the only environment read of
// the launch path. Validated: an unknown key or value rejects the whole spec.
namespace {
std::mutex g_plan_mu;
PlanOverrides g_plan;
std::string g_plan_spec;  // normalised, "" = the measured default plan
std::once_flag g_plan_env_once;

bool parse_int(const std::string& v, int lo, int hi, int* out) {
  if (v.empty() || v.size() > 6 || v.find_first_not_of("0123456789") != std::string::npos) return false;
  const int x = atoi(v.c_str());
  if (x < lo || x > hi) return false;
  *out = x;
  return true;
}

// v among names[0..n): *out = values[its index]
template <class E, int N>
bool parse_enum(const std::string& v, const char* const (&names)[N], const E (&values)[N], E* out) {
  for (int i = 0; i < N; ++i)
    if (v == names[i]) {
      *out = values[i];
      return true;
    }
  return false;
}
}  // namespace

int parse_plan(const char* spec, PlanOverrides* o, std::string* norm, std::string* err) {
  *o = PlanOverrides{};
  norm->clear();
  std::string s = spec ? spec : "";
  for (char& ch : s)
    if (ch == ';' || ch == ' ') ch = ',';
  size_t p = 0;
  while (p <= s.size()) {
    size_t q = s.find(',', p);
    if (q == std::string::npos) q = s.size();
    const std::string item = s.substr(p, q - p);
    p = q + 1;
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    if (eq == std::string::npos) {
      *err = "plan item '" + item + "' is not key=value";
      return -1;
    }
    const std::string k = item.substr(0, eq), v = item.substr(eq + 1);
    bool ok = true;
    if (k == "update") {
      ok = parse_enum(v, {"auto", "stream", "tiled", "pipe"},
                      {UpdateForm::Auto, UpdateForm::Stream, UpdateForm::Tiled, UpdateForm::Pipe}, &o->update);
    } else if (k == "grid") {
      ok = parse_enum(v, {"auto", "plain", "lanes", "balanced"},
                      {StreamGrid::Auto, StreamGrid::Plain, StreamGrid::Lanes, StreamGrid::Balanced}, &o->grid);
    } else if (k == "tile") {
      ok = parse_enum(v, {"auto", "classic", "flat", "weave6", "weave8"},
                      {TileForm::Auto, TileForm::Classic, TileForm::Flat, TileForm::Weave6, TileForm::Weave8}, &o->tile);
    } else if (k == "tile_enc_prio") {
      if (v == "auto") o->tile_enc_prio = -1;
      else ok = parse_int(v, 0, 3, &o->tile_enc_prio);
    } else if (k == "flat_w2") {
      if (v == "auto") o->flat_w2 = 0;
      else ok = parse_int(v, 1, kFlatTG, &o->flat_w2);
    } else if (k == "tile_enc_rows") {
      ok = parse_int(v, 1, 4096, &o->tile_enc_rows);
    } else if (k == "fused") {
      ok = parse_enum(v, {"on", "off"}, {true, false}, &o->fused);
    } else if (k == "stage_threads") {
      ok = parse_int(v, 1, 64, &o->stage_threads);
    } else if (k == "stage_pieces") {
      ok = parse_int(v, 1, 64, &o->stage_pieces);
    } else {
      *err = "unknown plan key '" + k + "' (update, grid, tile, flat_w2, tile_enc_prio, tile_enc_rows, fused, "
             "stage_threads, stage_pieces)";
      return -1;
    }
    if (!ok) {
      *err = "bad value '" + v + "' for plan key '" + k + "'";
      return -1;
    }
    if (!norm->empty()) *norm += ",";
    *norm += k + "=" + v;
  }
  return 0;
}

static void plan_env_init() {
  std::call_once(g_plan_env_once, [] {
    const char* e = getenv("FLEET_EXPERIMENTS");
    if (!e || !*e) return;
    PlanOverrides o;
    std::string norm, err;
    if (parse_plan(e, &o, &norm, &err) != 0) {
      fprintf(stderr, "[fleet] FLEET_EXPERIMENTS rejected (%s): the default launch plan is used\n", err.c_str());
      return;
    }
    std::lock_guard<std::mutex> lk(g_plan_mu);
    g_plan = o;
    g_plan_spec = norm;
  });
}

PlanOverrides plan_overrides() {
  plan_env_init();
  std::lock_guard<std::mutex> lk(g_plan_mu);
  return g_plan;
}

int set_plan_overrides(const char* spec, std::string* err) {
  plan_env_init();
  PlanOverrides o;
  std::string norm;
  if (parse_plan(spec, &o, &norm, err) != 0) return -1;
  std::lock_guard<std::mutex> lk(g_plan_mu);
  g_plan = o;
  g_plan_spec = norm;
  return 0;
}

std::string plan_spec() {
  plan_env_init();
  std::lock_guard<std::mutex> lk(g_plan_mu);
  return g_plan_spec;
}

static inline int64_t ceil_div(int64_t n, int64_t t) { return (n + t - 1) / t; }

// k_update_flat's grid for `groups` groups: r whole rounds of kFlatTG-group tiles over the
// CUs, the rest in tiles of w2 = kFlatTG, 1/2 or 1/4 of it dealt round robin after them.
// Picks the w2 that leaves the most loaded CU the fewest groups (r * kFlatTG +
// ceil(n2 / CUs) * w2) with every tile resident at once (r + ceil(n2 / CUs) <= kFlatSlots),
// the wider on a tie; more than one round of the widest tiles when the groups do not fit
// one. (On the N = 8 window, 2.7 tiles per CU, the 16-group tiles' extra serial chains
// also hide latency: the update 156-159 us on one width, 143 us with them; r05.)
static FlatGrid flat_grid(int64_t groups, int forced_w2, bool fused, int64_t cus) {
  const int64_t w1 = kFlatTG;
  const int64_t r = groups / (w1 * cus);
  const int64_t rest = groups - r * w1 * cus;
  int best = -1;
  int64_t best_load = INT64_MAX;
  // the fused step: no quarter-width tiles (their extra blocks take the slots the encode's
  // blocks would start in) and half-width ones on a tie (the N = 8 window, 192 groups per
  // CU either way: 175.4 us with quarter-width, 173.1 / 176.6 with half-width against
  // 182.3 with full-width narrow tiles; r05 same-process A/Bs)
  for (int k = 0; k < (fused ? 2 : 3); ++k) {
    const int w2 = forced_w2 ? forced_w2 : kFlatTG >> k;  // a forced width: that one, even past a round
    const int64_t n2 = ceil_div(rest, w2), per_cu = ceil_div(n2, cus);
    if (r + per_cu > kFlatSlots && !forced_w2) continue;
    const int64_t load = r * w1 + per_cu * w2;
    if (load < best_load || (fused && load == best_load)) {  // the fused step: the narrower on a tie
      best_load = load;
      best = w2;
    }
  }
  if (best < 0) best = kFlatTG;  // more than a round: the widest tiles throughout
  const int64_t n2 = ceil_div(rest, best);
  return FlatGrid{(int)(r * cus), (int)(r * cus + n2), kFlatTG, best};
}

// The stream grid of k_update_mixed<256>: p->nA blocks of group-per-lane waves, p->blocks in all.
static void stream_grid(LaunchPlan* p, int64_t groups, StreamGrid grid, int cus) {
  const int64_t plain = ceil_div(groups, 256);
  if (grid == StreamGrid::Plain) {
    p->nA = (int)plain;
  } else if (grid == StreamGrid::Lanes) {
    p->nA = 0;
  } else {  // whole rounds of group-per-lane waves (a multiple of one wave per SIMD)
    const int simds = 4 * cus;
    const int64_t waves = ceil_div(groups, 64);
    p->nA = waves < simds ? (int)plain : (int)(waves / simds * simds * 64 / 256);
  }
  // the value-per-lane blocks take what the group-per-lane rounds leave (none when
  // the plain grid covers every group: its last block is ragged)
  const int64_t rest = groups - (int64_t)p->nA * 256;
  p->blocks = p->nA + (rest > 0 ? ceil_div(rest, 84) : 0);
}

// The form's own grid: p->blocks (and nA / fg), one launch of them, 64 lanes per wave.
static void size_update(LaunchPlan* p, int64_t groups, StreamGrid grid, int forced_w2, bool fused, int cus) {
  p->threads = 256;
  switch (p->kind) {
    case UpdateKind::Pipe: p->blocks = ceil_div(groups, 16), p->threads = 64 * kPipeNW; break;
    case UpdateKind::Flat: p->fg = flat_grid(groups, forced_w2, fused, cus), p->blocks = p->fg.nU; break;
    case UpdateKind::Weave: p->blocks = ceil_div(groups, kWeaveTG), p->threads = 64 * p->nw; break;
    // one width (the fused step's tiles; the update alone under tile=classic)
    case UpdateKind::Tiled: p->blocks = ceil_div(groups, 64); break;
    case UpdateKind::Stream: stream_grid(p, groups, grid, cus); break;
  }
  p->grid = p->blocks;
}

// the form asked for, or: stream from 131,072 groups, the tiles from `tile_min`, the
// pipelined tiles below
static UpdateKind pick_form(int64_t groups, UpdateForm want, int64_t tile_min) {
  if (want == UpdateForm::Stream) return UpdateKind::Stream;
  if (want == UpdateForm::Tiled) return UpdateKind::Tiled;
  if (want == UpdateForm::Pipe) return UpdateKind::Pipe;
  return groups >= 256LL * 4 * 2 * 64 ? UpdateKind::Stream : groups >= tile_min ? UpdateKind::Tiled : UpdateKind::Pipe;
}

static LaunchPlan plan_forms(PlanStep step, int64_t groups, const PlanOverrides& o, int cus) {
  const bool fused = step == PlanStep::UpdateEncode;  // (UpdateThenEncode: the update alone's plan)
  const bool tile_auto = o.tile == TileForm::Auto;
  LaunchPlan p{};
  p.step = step;
  // the tiles from 32 k groups; the update alone (auto tiles) from 24 k, where its woven
  // tiles already beat the pipelined ones (cifar10_256's N = 4 window, 26 k groups: 100.8
  // against 141.3 us; 20.9 k: 106.9 / 109.4; 18.4 k and below the pipelined tiles win;
  // r05, profiles/r05/ab_weave_vs_pipe.txt)
  p.kind = pick_form(groups, o.update, (!fused && tile_auto) ? 24LL * 1024 : 32LL * 1024);
  if (p.kind == UpdateKind::Tiled && (o.tile == TileForm::Weave6 || o.tile == TileForm::Weave8)) {
    p.kind = UpdateKind::Weave;  // the woven tiles (one width)
    p.nw = (int)o.tile;
  }
  // the flat tiles for the update alone; the fused step keeps the one-width 64-group tiles
  // from 64 k groups, whose free block slots start the encode's blocks beside them
  // (same-process A/B, r05: the update alone 276 -> 261 us on cifar10_256, 241 -> 227 on
  // the N = 4 window, 1133 -> 1099 on cifar100_1024; the fused step 380 against 392 on
  // cifar10_256, but 170.6 against 181.4 us on the N = 8 window)
  // the update alone up to three 64-group tiles per CU (the N = 8 window: 2.7, latency-
  // bound): the woven 8-wave tiles, whose serial steps run between the producers' stages,
  // one round of them at most (synth1m_256's N = 8 window 125.3 against 143.8 us for the
  // flat tiles, cifar10_256's N = 3 122.2 against 146.2; at 3.2 and 3.6 tiles per CU they
  // lose, 190-194 against 161-165 us; r05 same-process A/B, profiles/r05/ab_weave_small.txt)
  if (p.kind == UpdateKind::Tiled && tile_auto && !fused && groups <= 3LL * 64 * cus) {
    p.kind = UpdateKind::Weave;
    p.nw = 8;
  }
  // the fused step on small windows: the woven tiles with the encode's blocks after them
  // from 14 k to 40 k groups (8 waves up to 32 k, 6 above), the pipelined tiles below
  // (cifar10_256's N = 5 window 134.7 -> 107.5 us, cifar100_1024's N = 4 672.4 -> 463.0,
  // cifar10_256's N = 3 160.2 -> 147.6 against the flat tiles; 13 k groups: 90.0 pipelined
  // against 94.1; r05 same-process A/B, profiles/r05/ab_weave_fused.txt)
  if (fused && o.update == UpdateForm::Auto && tile_auto && groups >= 14LL * 1024 && groups < 40LL * 1024) {
    p.kind = UpdateKind::Weave;
    p.nw = groups < 32LL * 1024 ? 8 : 6;
  }
  if (p.kind == UpdateKind::Tiled && (o.tile == TileForm::Flat || (tile_auto && (!fused || groups < 65536))))
    p.kind = UpdateKind::Flat;
  size_update(&p, groups, o.grid, o.flat_w2, fused, cus);
  return p;
}

LaunchPlan plan_update(int64_t groups, const PlanOverrides& o, int cus) {
  return plan_forms(PlanStep::Update, groups, o, cus);
}

// rows per block of the standalone client encode: about 65,536 blocks in all (a
// lane walks its group down rpb rows, so the LDS table copy is paid once per rpb
// rows). Measured on one box (gpu_encode_rpb.sh (r04 tree), two rows of loads in
// flight): synth1m_256 encodes in 478-480 us at 4-8 rows per block, 483 at 16, 501
// at 2 and 32, 595 at 1; the same access pattern without the codec arithmetic
// (scripts/ubench_stream.hip, 12 B in / 16 B out per lane) runs 452-486 us.
int encode_rows_per_block(int64_t gx, int rows) {
  return (int)std::min<int64_t>(rows, std::max<int64_t>(1, (gx * rows + 65535) / 65536));
}

// The aggregation and the client encode in one launch (the pipelined step):
// k_update_encode on the stream grid, k_update_tiled_encode on the wide tiles, the
// pipelined tiles with the encode's blocks after them; plan fused=off runs the two
// kernels back to back.
LaunchPlan plan_update_encode(int64_t groups, int M, const PlanOverrides& o, int cus) {
  if (!o.fused) return plan_forms(PlanStep::UpdateThenEncode, groups, o, cus);
  LaunchPlan p = plan_forms(PlanStep::UpdateEncode, groups, o, cus);
  // the tiles' encode blocks at issue priority 3 beside the tiles' ladder (3 -> 0) from
  // 64 k groups, 0 below: cifar10_256 394 -> 380 us, the N = 4 window 319 -> 311,
  // cifar100_1024 1622 -> 1593, the N = 8 window 174.5 -> 178.5 (r05 same-process A/B)
  int auto_prio = groups >= 65536 ? 3 : 0;
  if (p.kind == UpdateKind::Weave) auto_prio = 0;
  if (p.kind == UpdateKind::Stream) {
    // the stream grid group-per-lane everywhere: the encode's blocks fill the SIMDs the
    // last round of update waves leaves idle, so the value-per-lane balancing of
    // k_update_mixed only adds instructions here (same-box A/B on synth1m_256: 1172.7 vs
    // 1181.3 us, gpu_fused_ab.sh (r04 tree)). 24 rows per encode block: short blocks that
    // fill the slots the update's waves leave (a lane walks its group down the rows with
    // two loads in flight, so a block of hundreds of rows is a latency-bound straggler);
    // same-box A/B on synth1m_256: 1179 / 1170 us at 6 / 12 rows per block in r03; with
    // the encode's waves at priority 3 (r04) 1130 / 1097-1100 / 1084-1090 us at 6 / 12 /
    // 24, and 48 no better (r04 call a31, a32.sh).
    // (grid=lanes: the update's blocks a value per lane, for experiments on small windows)
    // Below four waves of group-per-lane update per SIMD (the N = 2 strong window: 2.7) the
    // update alone's SIMD-balanced split -- whole rounds of group-per-lane waves, the rest a
    // value per lane -- also under the encode's blocks (grid=balanced): synth1m_256's N = 2
    // window 635.3 -> 604.3 us, configs[4]'s N = 8 window 11.09 -> 10.05 ms, while the full
    // width (5.3 waves per SIMD) loses with it, 1106.6 -> 1159.8 us; one group-per-lane round
    // fewer loses at N = 2 (624.0 us) (r05 same-process A/B, profiles/r05/ab_fused_balanced.txt)
    const bool balanced =
        o.grid == StreamGrid::Balanced || (o.grid == StreamGrid::Auto && groups < 4LL * 64 * 4 * cus);
    stream_grid(&p, groups,
                o.grid == StreamGrid::Lanes ? o.grid : balanced ? StreamGrid::Balanced : StreamGrid::Plain, cus);
    // the encode's waves at priority 3 over the full width (r04, see k_update_encode), at 0
    // under the balanced split of a small window: there the update waves, 2.7 per SIMD, are
    // the critical path (the N = 2 window 588.9 -> 572.5 us, while the full width loses at 2,
    // 1083.7 -> 1108.4; r05 same-process A/B, profiles/r05/ab_stream_encode_prio.txt)
    auto_prio = balanced ? 0 : 3;
  }
  p.enc_gx = ceil_div(groups, p.threads);  // the encode's blocks are the update's size: a group per lane
  if (p.kind == UpdateKind::Pipe) {  // small buckets: the pipelined tiles, the encode's 320-lane blocks after them
    p.enc_rpb = encode_rows_per_block(p.enc_gx, M);
    p.enc_prio = 0;
  } else {
    // 24 rows per encode block, as in k_update_encode: each block copies the tile's
    // 14 KB of tables into LDS, so the standalone encode's ~65,536 blocks (2 rows each at
    // CIFAR sizes) spent the step on table copies -- the encode ran mostly after the
    // tiles, 230 us of it on cifar10_256 against 157 us alone (r05 residency trace)
    // (the woven tiles too: the standalone encode's rule gave their 64 * nw-lane blocks
    // one or two rows each, every block copying the tables for them)
    p.enc_rpb = std::min(M, o.tile_enc_rows > 0 ? o.tile_enc_rows : 24);
    p.enc_prio = o.tile_enc_prio >= 0 ? o.tile_enc_prio : auto_prio;
  }
  p.grid = p.blocks + p.enc_gx * ceil_div(M, p.enc_rpb);
  return p;
}

// The update's own launch plan with the side outputs: the pipelined tiles (side outputs
// from the producers, the reduce blocks in the same launch), the wide tiles (side
// outputs from the tile producers), or the stream kernel's SIMD-balanced grid
LaunchPlan plan_update_kardam(int64_t groups, int M, const PlanOverrides& o, int cus) {
  LaunchPlan p{};
  p.step = PlanStep::UpdateKardam;
  // Kardam's side outputs ride in the flat tiles at every tile size (kardam_items: narrow
  // widths 16 / 32 / 64 only, so another forced width is ignored here), never in the
  // classic or woven ones
  p.kind = pick_form(groups, o.update, 32LL * 1024);
  if (p.kind == UpdateKind::Tiled) p.kind = UpdateKind::Flat;
  const bool w2_fits = o.flat_w2 == 16 || o.flat_w2 == 32 || o.flat_w2 == 64;
  // the stream form on the plain grid unless a grid is asked for: value-per-lane waves
  // pay the per-client wave sums for a third of the values (synth1m_256: 1747 vs
  // 1724 us, r04 call a6)
  size_update(&p, groups, o.grid == StreamGrid::Auto ? StreamGrid::Plain : o.grid, w2_fits ? o.flat_w2 : 0, false, cus);
  const bool pipe = p.kind == UpdateKind::Pipe;
  // partial slots per client: a wave of the stream grid or a tile
  p.n_waves = p.kind == UpdateKind::Stream ? (int)p.blocks * 4 : (int)p.blocks;
  p.flag_slots = pipe ? (int)p.blocks * (kKdPipeNW - 1) : 0;  // the pipelined form's tile flags (per producer wave)
  p.norm_parts = 1;                                            // one pair per client
  if (pipe) {  // the tiles, then one reduce block per client
    p.threads = 64 * kKdPipeNW;
    p.grid = p.blocks + M;
  }
  p.reduce = pipe ? KardamReduce::InLaunch
             : p.n_waves <= 512 ? KardamReduce::Wave8
             : p.n_waves <= 2048 ? KardamReduce::Wave32
                                 : KardamReduce::Block32;
  return p;
}

std::string kernel_name(const LaunchPlan& p) {
  const std::string nw = std::to_string(p.nw);
  if (p.step == PlanStep::UpdateKardam)
    return p.kind == UpdateKind::Stream ? "k_update_mixed<256, true>"
           : p.kind == UpdateKind::Flat ? "k_update_flat_kd"
                                        : "k_update_pipe<16, 1, " + std::to_string(kKdPipeNW) + ", 0, true>";
  const std::string pipe = "k_update_pipe<16, 1, " + std::to_string(kPipeNW) + ", 0, false>";
  const bool enc = p.step == PlanStep::UpdateEncode;
  std::string name;
  switch (p.kind) {
    case UpdateKind::Stream: name = enc ? "k_update_encode<256>" : "k_update_mixed<256, false>"; break;
    case UpdateKind::Tiled: name = "k_update_tiled_encode<64>"; break;  // alone: its tiles, no encode blocks
    case UpdateKind::Weave: name = (enc ? "k_update_weave_encode<" : "k_update_weave<") + nw + ">"; break;
    case UpdateKind::Flat: name = "k_update_flat"; break;
    case UpdateKind::Pipe: name = enc ? pipe + " (with the encode's blocks)" : pipe; break;
  }
  return p.step == PlanStep::UpdateThenEncode ? name + " + k_encode_f32" : name;
}

}  // namespace fleet
