// fleet_amd/csrc/mledger_table.cpp -- see mledger_table.h. Host code only.
#include "mledger_table.h"

#include <algorithm>
#include <cmath>
#include <map>

namespace fleet {

MledgerTable::MledgerTable(int workers, int max_versions)
    : workers_(workers), max_versions_(max_versions) {
  const size_t rows = (size_t)workers + (size_t)max_versions;
  row_id_.assign(rows, 0);
  row_refs_.assign(rows, 0);
  row_used_.assign(rows, 0);
  row_age_.assign(rows, 0);
  for (int r = (int)rows - 1; r >= 0; --r) free_rows_.push_back(r);
  worker_row_.assign((size_t)workers, -1);
}

int MledgerTable::row_of_id(int64_t id) const {
  const auto it = row_by_id_.find(id);
  return it == row_by_id_.end() ? -1 : it->second;
}

int MledgerTable::row_of_worker(int worker) const {
  return worker < 0 || worker >= workers_ ? -1 : worker_row_[(size_t)worker];
}

int MledgerTable::stage(int64_t id, bool* fresh) {
  const int have = row_of_id(id);
  if (have >= 0) {
    row_age_[(size_t)have] = ++clock_;
    *fresh = false;
    return have;
  }
  // at most max_versions rows that no worker holds, this one included
  for (;;) {
    int unref = 0, oldest = -1;
    for (int r = 0; r < rows(); ++r) {
      if (!row_used_[(size_t)r] || row_refs_[(size_t)r]) continue;
      ++unref;
      if (oldest < 0 || row_age_[(size_t)r] < row_age_[(size_t)oldest]) oldest = r;
    }
    if (unref < max_versions_) break;
    row_by_id_.erase(row_id_[(size_t)oldest]);
    row_used_[(size_t)oldest] = 0;
    free_rows_.push_back(oldest);
  }
  // referenced rows <= workers and unreferenced ones < max_versions: a row is free
  const int r = free_rows_.back();
  free_rows_.pop_back();
  row_id_[(size_t)r] = id, row_refs_[(size_t)r] = 0, row_used_[(size_t)r] = 1, row_age_[(size_t)r] = ++clock_;
  row_by_id_[id] = r;
  *fresh = true;
  return r;
}

void MledgerTable::unstage(int64_t id) {
  const int r = row_of_id(id);
  if (r < 0 || row_refs_[(size_t)r]) return;
  row_by_id_.erase(id);
  row_used_[(size_t)r] = 0;
  free_rows_.push_back(r);
}

bool MledgerTable::forget(int worker) {
  const int r = row_of_worker(worker);
  if (r < 0) return false;
  --row_refs_[(size_t)r];  // the row stays resident, unreferenced, until a stage evicts it
  worker_row_[(size_t)worker] = -1;
  return true;
}

int MledgerTable::pair_index(int32_t cur, int32_t prev, bool add) {
  const uint64_t key = ((uint64_t)(uint32_t)cur << 32) | (uint32_t)prev;
  const auto it = pair_by_rows_.find(key);
  if (it != pair_by_rows_.end()) return it->second;
  if (!add) return -1;
  const int32_t i = (int32_t)pair_cur_.size();
  pair_cur_.push_back(cur), pair_prev_.push_back(prev);
  pair_by_rows_[key] = i;
  return i;
}

bool MledgerTable::resolve(const int64_t* id, const int32_t* worker, int K, std::string* err) {
  k_row_.assign((size_t)K, -1);
  k_worker_.assign(worker, worker + K);
  pair_cur_.clear(), pair_prev_.clear(), pair_by_rows_.clear();
  active_ = 0;
  std::vector<int32_t> fresh;  // picked rows that no worker holds
  for (int k = 0; k < K; ++k) {
    if (worker[k] < 0) continue;  // Kardam does not run for this pick (CppNNUpdater.java:472-474)
    if (worker[k] >= workers_) {
      *err = "pick " + std::to_string(k) + " names worker " + std::to_string(worker[k]) + " of " + std::to_string(workers_);
      return false;
    }
    const int r = row_of_id(id[k]);
    if (r < 0) {
      *err = "pick " + std::to_string(k) + " names version " + std::to_string(id[k]) + ", which is not resident";
      return false;
    }
    k_row_[(size_t)k] = r;
    ++active_;
    if (!row_refs_[(size_t)r] && std::find(fresh.begin(), fresh.end(), r) == fresh.end()) fresh.push_back(r);
  }
  if ((int)fresh.size() > max_versions_) {
    *err = std::to_string(fresh.size()) + " picked versions that no worker holds, the ledger keeps " +
           std::to_string(max_versions_);
    return false;
  }
  // the rows a worker may hold when its next pick of this update comes (Kardam.java:115-124):
  // the one it holds now, and the row of each of its earlier picks, which stored or not
  std::map<int32_t, std::vector<int32_t>> may_hold;
  for (int k = 0; k < K; ++k) {
    const int32_t cur = k_row_[(size_t)k];
    if (cur < 0) continue;
    const int32_t w = worker[k];
    auto it = may_hold.find(w);
    if (it == may_hold.end()) {
      it = may_hold.emplace(w, std::vector<int32_t>()).first;
      if (worker_row_[(size_t)w] >= 0) it->second.push_back(worker_row_[(size_t)w]);
    }
    std::vector<int32_t>& c = it->second;
    for (int32_t prev : c) pair_index(cur, prev, true);
    // (no model yet: the first pick stores whatever its norm would be, :124)
    if (std::find(c.begin(), c.end(), cur) == c.end()) c.push_back(cur);
  }
  return true;
}

void MledgerTable::replay(const double* pair_norm, double* norm_diff, uint8_t* status) {
  std::map<int32_t, int32_t> hold;  // the touched workers' rows as the loop leaves them
  const int K = (int)k_row_.size();
  for (int k = 0; k < K; ++k) {
    const int32_t cur = k_row_[(size_t)k];
    if (cur < 0) {
      status[k] = kMlSkipped;
      norm_diff[k] = std::nan("");
      continue;
    }
    const int32_t w = k_worker_[(size_t)k];
    auto it = hold.find(w);
    if (it == hold.end()) it = hold.emplace(w, worker_row_[(size_t)w]).first;
    if (it->second >= 0) {  // models.containsKey (:115)
      const double norm = pair_norm[pair_index(cur, it->second, false)];
      if (norm == 0) {  // IGNORE: zero norm (:118-121); a NaN norm is not 0 and stores
        status[k] = kMlIgnored;
        norm_diff[k] = norm;
        continue;
      }
      status[k] = kMlSet;
      norm_diff[k] = norm;  // modelDiffNorm.put (:122)
    } else {
      status[k] = kMlFirst;
      norm_diff[k] = std::nan("");
    }
    it->second = cur;  // models.put (:124)
  }
  for (const auto& h : hold) {
    const int32_t was = worker_row_[(size_t)h.first];
    if (was == h.second) continue;
    if (was >= 0) --row_refs_[(size_t)was];
    ++row_refs_[(size_t)h.second];
    worker_row_[(size_t)h.first] = h.second;
  }
}

}  // namespace fleet
