// fleet_amd/csrc/mledger_table.h -- the host bookkeeping of the Kardam model ledger
// (fleet_mledger_*): Kardam.java's `models` map (worker -> model, Kardam.java:114-125) over
// a slab of rows that belong to model VERSIONS, not to workers. Plain C++ (no HIP header):
// fleet_codec.cpp fills the rows and computes the norms the table asks for.
//
//   version id -> row, worker -> row, a reference count per row. "Storing" a worker's
//   model (models.put, :124) is a table update and copies nothing; workers at one version
//   share its row. The slab has workers + max_versions rows: at most `workers` rows are
//   referenced, and stage() keeps the unreferenced ones at `max_versions` by evicting the
//   one staged longest ago (staging a resident version renews its age).
//
//   One update = the picks' (version id, worker) in pick order. resolve() lists the
//   distinct ORDERED row pairs (cur, prev) whose norms setModel may ask for: a worker's
//   later pick in the same update depends on whether its earlier pick stored, which
//   depends on that pick's norm (:118-121), so the later pick gets a pair against every
//   row the worker may hold by then. A pair of a row with itself is listed like any other:
//   the rule is "norm == 0", not "same id". replay() then runs the reference's loop over
//   the norms that came back and commits; until then nothing has changed.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace fleet {

// fleet_mledger_update's status[k]
constexpr uint8_t kMlSkipped = 0, kMlFirst = 1, kMlIgnored = 2, kMlSet = 3;

class MledgerTable {
 public:
  MledgerTable(int workers, int max_versions);

  int workers() const { return workers_; }
  int max_versions() const { return max_versions_; }
  int rows() const { return (int)row_id_.size(); }

  int row_of_id(int64_t id) const;             // -1: not resident
  int row_of_worker(int worker) const;         // -1: models.containsKey is false (or no such worker)
  int64_t id_of_row(int row) const { return row_id_[(size_t)row]; }
  int refs_of_row(int row) const { return row_refs_[(size_t)row]; }

  // The row of version `id`. Resident: that row, its age renewed, *fresh = false. Otherwise
  // a free row, after evicting unreferenced rows (oldest first) while there are max_versions
  // of them; *fresh = true and the caller fills the row (unstage() when that fails).
  int stage(int64_t id, bool* fresh);
  void unstage(int64_t id);
  bool forget(int worker);  // models.remove(worker); false: it held none

  // One update's picks resolved against the tables, which do not change: false with *err
  // for a worker >= workers, a version that is not resident, or more distinct picked
  // versions that no worker holds than max_versions. worker[k] < 0: Kardam does not run
  // for pick k and id[k] is not looked at.
  bool resolve(const int64_t* id, const int32_t* worker, int K, std::string* err);
  const std::vector<int32_t>& pair_cur() const { return pair_cur_; }
  const std::vector<int32_t>& pair_prev() const { return pair_prev_; }
  int pick_row(int k) const { return k_row_[(size_t)k]; }  // -1: skipped
  int active() const { return active_; }                   // picks with a worker

  // Kardam.setModel for the resolved picks in order; pair_norm[i] = the norm of pair i.
  // Writes norm_diff[k] and status[k] for every pick and commits the tables.
  void replay(const double* pair_norm, double* norm_diff, uint8_t* status);

 private:
  int pair_index(int32_t cur, int32_t prev, bool add);

  int workers_, max_versions_;
  std::vector<int64_t> row_id_;
  std::vector<int32_t> row_refs_;
  std::vector<uint8_t> row_used_;
  std::vector<uint64_t> row_age_;
  uint64_t clock_ = 0;
  std::vector<int32_t> free_rows_;
  std::unordered_map<int64_t, int32_t> row_by_id_;
  std::vector<int32_t> worker_row_;
  // one update's resolution
  std::vector<int32_t> k_row_, k_worker_, pair_cur_, pair_prev_;
  std::unordered_map<uint64_t, int32_t> pair_by_rows_;
  int active_ = 0;
};

}  // namespace fleet
