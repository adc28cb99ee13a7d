// The message ranges a digest session has folded in (omr_digest_update): a set of disjoint
// half-open intervals [lo, hi) of global indices below `all`, kept sorted with touching intervals
// merged. Host only, no HIP: tests/host/digest_ranges_test.cpp builds it on its own.
#pragma once

#include <cstddef>
#include <iterator>
#include <map>

namespace omr {

class DigestRanges {
 public:
  explicit DigestRanges(size_t all) : all_(all) {}

  // Whether [offset, offset + D) lies inside [0, all) and meets no interval of the set. D = 0 is
  // accepted anywhere up to `all`; offset + D may not wrap.
  bool can_insert(size_t offset, size_t D) const {
    if (offset > all_ || D > all_ - offset) return false;
    if (D == 0) return true;
    const size_t hi = offset + D;
    auto it = iv_.upper_bound(offset);  // the first interval that starts after offset
    if (it != iv_.end() && it->first < hi) return false;
    if (it != iv_.begin() && std::prev(it)->second > offset) return false;
    return true;
  }

  // Adds [offset, offset + D) when can_insert allows it (the set is unchanged otherwise), merging it
  // with the intervals it touches.
  bool insert(size_t offset, size_t D) {
    if (!can_insert(offset, D)) return false;
    if (D == 0) return true;
    size_t lo = offset, hi = offset + D;
    auto next = iv_.upper_bound(offset);
    if (next != iv_.begin()) {
      auto prev = std::prev(next);
      if (prev->second == lo) {
        lo = prev->first;
        iv_.erase(prev);
      }
    }
    if (next != iv_.end() && next->first == hi) {
      hi = next->second;
      iv_.erase(next);
    }
    iv_[lo] = hi;
    covered_ += D;
    return true;
  }

  size_t all() const { return all_; }
  size_t covered() const { return covered_; }      // messages in the set
  size_t intervals() const { return iv_.size(); }  // disjoint, non-touching intervals
  bool contains(size_t i) const {
    auto it = iv_.upper_bound(i);
    return it != iv_.begin() && std::prev(it)->second > i;
  }

 private:
  size_t all_, covered_ = 0;
  std::map<size_t, size_t> iv_;  // lo -> hi
};

}  // namespace omr
